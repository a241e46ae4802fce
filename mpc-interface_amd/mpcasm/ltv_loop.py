"""The closed loop of a batch whose dynamics differ from step to step and from instance to instance (BASELINE
config C5), tick by tick on the device -- what :class:`mpcasm.walkers.WalkerFleet` is for the biped, for a
formulation compiled with ``ltv=``:

    window [t, t + N) of every instance's (A_k, B_k)   Assembler.bind_ltv_window   (a pointer, nothing copied)
    P, q, G, h                                         Assembler.assemble          (csrc/sweep.hip)
    x0, y0, z0, rho0 (warm=True only)                  engine.warm_start_qp        (csrc/warm.hip)
    x, status                                          engine.solve_qp_wide        (cold, OSQP's defaults)
    x polished where solved (polish=True only)         engine.polish_qp_wide       (csrc/polish_wide.hip)
    the solution into the warm store (warm=True only)  engine.warm_store_qp        (csrc/warm.hip)
    u = K x + v (feedback= only)                       Assembler.true_inputs       (csrc/feedback.hip)
    given <- x_1 = A_t x_0 + B_t u_0                   Assembler.advance           (csrc/rollout.hip)

-- the reference's tick (biped_mpc_loop.py:50-95: assemble, ``osqp_solve_qp``, ``preview_all`` +
``update_given_collector``) with per-step dynamics, nothing read back to the host.  The loop runs launch by
launch: the window's address changes every tick, which a captured graph would not follow."""
from .engine import (APPLY_ALL, APPLY_SOLVED, OSQP_RHO, WARM_SOLVED, Assembler, WarmStore, ltv_close, ltv_lqr,
                     polish_qp_wide, qp_polish_wide_info, qp_solve_wide_info, solve_qp_wide, warm_start_qp,
                     warm_store_qp)


class LtvLoop:
    """``batch`` instances of ``form`` whose dynamics ``name`` follows ``A_seq (B, T, n, n)`` / ``(T, n, n)``,
    ``B_seq (B, T, n, m)`` / ``(T, n, m)`` (contiguous float64 device tensors): tick ``t`` plans over the steps
    ``[t, t + N)`` and moves every instance one step along its own dynamics, so ``T - N + 1`` ticks can run.

    :attr:`given`: the ``(B, ng)`` device buffer of the instances' initial states -- write the start into it,
    read the states out of it.  ``on_unsolved`` is :class:`~mpcasm.walkers.WalkerFleet`'s rule for an instance
    whose QP did not come back solved (or out of iterations): ``"hold"`` leaves its row of ``given`` as it was
    (``APPLY_SOLVED``), ``"apply"`` applies whatever iterate came back unless it is NaN (``APPLY_ALL``).
    ``polish``: every solved QP is polished (:func:`~mpcasm.engine.polish_qp_wide`, OSQP's defaults) before its
    solution becomes the next ``given``; the results of a tick then carry ``"polish"``, the verdicts.
    ``warm`` (keyword only, default False): every solve starts from the instance's last solution moved one sample along -- every unknown and
    every row of a per-sample limit shifted, the other rows (the terminal box) copied -- with the step it ended
    with, where that solution was SOLVED; any other instance, and every one at the first tick, starts cold.  The
    results of a tick then carry ``"warm"``, which instances started warm.
    ``feedback`` (keyword only, default None: nothing changes): pre-stabilised prediction.  Over an unstable plant
    and a long horizon the condensed Hessian is rounding noise before the solver sees it (the pendulum at N = 100:
    every instance comes back ``NON_CVX``), so the plan is condensed over ``A_cl_k = A_k + B_k K_k`` instead, with
    ``u_k = K_k x_k + v_k``.  ``feedback`` is the gain -- a contiguous float64 device tensor ``(m, n)``, ``(B, m,
    n)`` or ``(B, T, m, n)`` -- or ``{"Q": .., "R": .., "terminal": ..}`` (``terminal`` optional), the weights of a
    Riccati sweep over every instance's whole sequence (:func:`~mpcasm.engine.ltv_lqr`), run once here;
    ``ValueError`` where that sweep fails for an instance (the one read-back of the loop).  ``A_cl_seq`` is built
    once and its windows are bound in ``A_seq``'s place; :attr:`K_seq` keeps the gains.  What this means for the
    formulation: THE UNKNOWNS ARE ``v`` -- a cost or a limit on the input variable is one on ``v``, the deviation
    from the feedback law, not on ``u``; costs and limits on states are unchanged, and so is the state the loop
    moves to (``A_cl_t x_0 + B_t v_0`` is the true ``A_t x_0 + B_t u_0``).  The results of a tick then carry
    ``"u"`` ``(B, axes, N, m)``, the true inputs of the plan just solved (:meth:`~mpcasm.engine.Assembler.
    true_inputs`).  ``warm`` and ``polish`` compose with it unchanged.
    ``solver_kwargs`` go to :func:`~mpcasm.engine.solve_qp_wide` (``eps_abs``, ``max_iter``, ...)."""

    def __init__(self, form, name, batch, A_seq, B_seq, on_unsolved="hold", polish=False, **solver_kwargs):
        # (`warm=` is a keyword of its own, taken out of the solver's: the positional order up to `polish` stays)
        warm = solver_kwargs.pop("warm", False)
        feedback = solver_kwargs.pop("feedback", None)
        if on_unsolved not in ("hold", "apply"):
            raise ValueError("on_unsolved: 'hold' or 'apply', got %r" % (on_unsolved,))
        self.on_unsolved = on_unsolved
        self._apply_mask = APPLY_SOLVED if on_unsolved == "hold" else APPLY_ALL
        self.name, self.batch = name, int(batch)
        self.asm = asm = Assembler(form, batch=self.batch, ltv=[name])
        torch = self._torch = asm._torch
        self.A_seq, self.B_seq = A_seq, B_seq
        self.horizon = asm.plan.ltv[0]["N"]
        asm.bind_ltv_window(name, A_seq, B_seq, 0)          # (the sequences' shapes are checked here)
        self.K_seq = None
        if feedback is not None:
            self._close(feedback)
        self.ticks_possible = A_seq.shape[-3] - self.horizon + 1
        self.t = 0
        f, i32 = dict(dtype=torch.float64, device=asm.device), dict(dtype=torch.int32, device=asm.device)
        B = self.batch
        self.given = torch.zeros((B, asm.ng), **f)
        # the solver's buffers, at fixed addresses for every tick
        self._qp = dict(x=torch.zeros((B, asm.no), **f), y=torch.zeros((B, asm.nc), **f),
                        z=torch.zeros((B, asm.nc), **f), status=torch.zeros(B, **i32), iters=torch.zeros(B, **i32),
                        res=torch.zeros((B, 2), **f), rho=torch.full((B,), OSQP_RHO, **f))
        self._solver_kwargs = dict(solver_kwargs)
        # where K^-1 does not fit on chip it is the solver's workspace: allocated once, unless the caller brings one
        if "kinv" not in solver_kwargs and not qp_solve_wide_info(asm.no, asm.nc)[1]:
            self._solver_kwargs["kinv"] = torch.empty((B, asm.no, asm.no), **f)
        # the polish's workspace and verdicts, allocated once
        self.polish = bool(polish)
        if self.polish:
            self._polish_work = torch.empty((max(qp_polish_wide_info(asm.no, asm.nc, B)[1], 16) // 8,), **f)
            self._polish_verdict = torch.zeros(B, **i32)
        # the warm store (a record per instance, no index) and the one shift map, built once
        self.warm = bool(warm)
        if self.warm:
            from .warm import shift_map
            rows = [n for _, n in asm.plan.limit_rows]
            col, row = shift_map(form, form, False, horizon=self.horizon, prev_rows=rows, new_rows=rows)
            self._col_src, self._row_src = (torch.as_tensor(v, device=asm.device) for v in (col, row))
            self._store = WarmStore(B, asm.no, asm.nc, asm.device)
            self._warm_flags = torch.zeros(B, **i32)

    def _close(self, feedback):
        """``feedback=``: the gains as ``K_seq (T, m, n)`` / ``(B, T, m, n)``, and ``A_cl_seq`` in ``A_seq``'s place."""
        torch, asm = self._torch, self.asm
        g = asm.plan.ltv[0]
        n, m, T = g["n"], g["m"], self.A_seq.shape[-3]
        if isinstance(feedback, dict):
            if not {"Q", "R"} <= set(feedback) <= {"Q", "R", "terminal"}:
                raise ValueError("feedback: the weights 'Q' and 'R' and, if wanted, 'terminal'; got %s"
                                 % sorted(feedback))
            K, Acl, info = ltv_lqr(self.A_seq, self.B_seq, feedback["Q"], feedback["R"], feedback.get("terminal"))
            failed = torch.nonzero(info >= 0).flatten().tolist()
            if failed:
                raise ValueError("feedback: the Riccati sweep met a pivot that is not positive for instance(s) %s "
                                 "(at step(s) %s)" % (failed[:8], info[failed[:8]].tolist()))
        else:
            shapes = ((m, n), (self.batch, m, n), (self.batch, T, m, n))
            if not (torch.is_tensor(feedback) and feedback.dtype == torch.float64 and feedback.device == asm.device
                    and feedback.is_contiguous() and tuple(feedback.shape) in shapes):
                raise ValueError("feedback: a contiguous float64 tensor of shape %s, %s or %s on %s, or the weights "
                                 "{'Q': .., 'R': ..} of a Riccati sweep" % (shapes + (asm.device,)))
            Acl = ltv_close(self.A_seq, self.B_seq, feedback)
            K = feedback
            if K.dim() < 4:      # (one gain for every step: true_inputs takes its window of a sequence)
                K = (K if K.dim() == 3 else K[None])[:, None].expand(-1, T, m, n).contiguous()
                K = K[0] if feedback.dim() == 2 else K
        self.K_seq, self.A_cl_seq = K, Acl
        self._u = torch.zeros((self.batch, asm.plan.sweep["axes"].shape[0], self.horizon, m), dtype=torch.float64,
                              device=asm.device)

    def step(self):
        """One tick on :attr:`given`: the window at ``t``, the assembly, a cold solve, the next ``given`` by the
        loop's ``on_unsolved`` rule; then ``t`` advances.  Nothing is read back: returns ``{"x", "status",
        "iters"}`` (a loop that polishes: and ``"polish"``; one with ``feedback``: and ``"u"``), device tensors in the loop's own buffers, valid until
        the next step."""
        if self.t >= self.ticks_possible:
            raise ValueError("the sequences hold %d steps: no window of %d steps starts at tick %d"
                             % (self.A_seq.shape[-3], self.horizon, self.t))
        asm, qp = self.asm, self._qp
        asm.bind_ltv_window(self.name, self.A_seq if self.K_seq is None else self.A_cl_seq, self.B_seq, self.t)
        P, q, G, h = asm.assemble(self.given)
        if self.warm:                      # (the tag is the tick + 1: a record is one tick old or not warm)
            warm_start_qp(self._store, G, h, self._col_src, self._row_src, self.t, warm_mask=WARM_SOLVED,
                          rho_cold=OSQP_RHO, out=(qp["x"], qp["y"], qp["z"], qp["rho"], self._warm_flags))
        else:
            qp["rho"].fill_(OSQP_RHO)      # (the reference builds a fresh solver every tick)
        sol = solve_qp_wide(P, q, G, h, rho=qp["rho"], out=tuple(qp[k] for k in ("x", "y", "z", "status", "iters",
                                                                                  "res")), warm=self.warm,
                            **self._solver_kwargs)
        if self.polish:
            polish_qp_wide(P, q, G, h, sol, status=sol.status, out=(self._polish_verdict, sol.res),
                           work=self._polish_work)
        if self.warm:
            warm_store_qp(self._store, sol, self.t + 1)
        if self.K_seq is not None:         # (from the tick's initial states: before they advance)
            asm.true_inputs(self.K_seq, self.t, self.given, sol.x, out=self._u)
        asm.advance(self.given, sol.x, status=sol.status, apply_mask=self._apply_mask)
        self.t += 1
        out = {"x": sol.x, "status": sol.status, "iters": sol.iters}
        if self.K_seq is not None:
            out["u"] = self._u
        if self.polish:
            out["polish"] = self._polish_verdict
        if self.warm:
            out["warm"] = self._warm_flags
        return out

    def run(self, ticks, record=False):
        """:meth:`step` ``ticks`` times; returns device tensors ``status`` and ``iters`` ``(ticks, batch)`` int32
        (a loop that polishes: and ``polish``, the verdicts, alike) and, with ``record``, ``given`` ``(ticks + 1, batch, ng)``: :attr:`given` before the first tick and after
        every tick (as :meth:`mpcasm.walkers.WalkerFleet.run` records them) and, in a loop with ``feedback``, ``u``
        ``(ticks, batch, axes, m)``: the true input every tick's plan begins with, ``u[:, :, 0]`` of its result."""
        torch, given = self._torch, self.given
        i32 = dict(dtype=torch.int32, device=given.device)
        status = torch.zeros((ticks, self.batch), **i32)
        iters = torch.zeros((ticks, self.batch), **i32)
        verdicts = torch.zeros((ticks, self.batch), **i32) if self.polish else None
        trail = torch.empty((ticks + 1,) + tuple(given.shape), dtype=given.dtype, device=given.device) \
            if record else None
        first = torch.empty((ticks,) + tuple(self._u[:, :, 0].shape), dtype=given.dtype, device=given.device) \
            if record and self.K_seq is not None else None
        if record:
            trail[0].copy_(given)
        for t in range(ticks):
            out = self.step()
            status[t].copy_(out["status"])
            iters[t].copy_(out["iters"])
            if self.polish:
                verdicts[t].copy_(out["polish"])
            if record:
                trail[t + 1].copy_(given)
            if first is not None:
                first[t].copy_(out["u"][:, :, 0])
        result = {"status": status, "iters": iters}
        if self.polish:
            result["polish"] = verdicts
        if record:
            result["given"] = trail
        if first is not None:
            result["u"] = first
        return result
