"""The closed loop of a batch whose dynamics differ from step to step and from instance to instance (BASELINE
config C5), tick by tick on the device -- what :class:`mpcasm.walkers.WalkerFleet` is for the biped, for a
formulation compiled with ``ltv=``:

    window [t, t + N) of every instance's (A_k, B_k)   Assembler.bind_ltv_window   (a pointer, nothing copied)
    P, q, G, h                                         Assembler.assemble          (csrc/sweep.hip)
    x0, y0, z0, rho0 (warm=True only)                  engine.warm_start_qp        (csrc/warm.hip)
    x, status                                          engine.solve_qp_wide        (cold, OSQP's defaults)
    x polished where solved (polish=True only)         engine.polish_qp_wide       (csrc/polish_wide.hip)
    the solution into the warm store (warm=True only)  engine.warm_store_qp        (csrc/warm.hip)
    given <- x_1 = A_t x_0 + B_t u_0                   Assembler.advance           (csrc/rollout.hip)

-- the reference's tick (biped_mpc_loop.py:50-95: assemble, ``osqp_solve_qp``, ``preview_all`` +
``update_given_collector``) with per-step dynamics, nothing read back to the host.  The loop runs launch by
launch: the window's address changes every tick, which a captured graph would not follow."""
from .engine import (APPLY_ALL, APPLY_SOLVED, OSQP_RHO, WARM_SOLVED, Assembler, WarmStore, polish_qp_wide,
                     qp_polish_wide_info, qp_solve_wide_info, solve_qp_wide, warm_start_qp, warm_store_qp)


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
    ``solver_kwargs`` go to :func:`~mpcasm.engine.solve_qp_wide` (``eps_abs``, ``max_iter``, ...)."""

    def __init__(self, form, name, batch, A_seq, B_seq, on_unsolved="hold", polish=False, **solver_kwargs):
        # (`warm=` is a keyword of its own, taken out of the solver's: the positional order up to `polish` stays)
        warm = solver_kwargs.pop("warm", False)
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

    def step(self):
        """One tick on :attr:`given`: the window at ``t``, the assembly, a cold solve, the next ``given`` by the
        loop's ``on_unsolved`` rule; then ``t`` advances.  Nothing is read back: returns ``{"x", "status",
        "iters"}`` (a loop that polishes: and ``"polish"``), device tensors in the loop's own buffers, valid until
        the next step."""
        if self.t >= self.ticks_possible:
            raise ValueError("the sequences hold %d steps: no window of %d steps starts at tick %d"
                             % (self.A_seq.shape[-3], self.horizon, self.t))
        asm, qp = self.asm, self._qp
        asm.bind_ltv_window(self.name, self.A_seq, self.B_seq, self.t)
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
        asm.advance(self.given, sol.x, status=sol.status, apply_mask=self._apply_mask)
        self.t += 1
        out = {"x": sol.x, "status": sol.status, "iters": sol.iters}
        if self.polish:
            out["polish"] = self._polish_verdict
        if self.warm:
            out["warm"] = self._warm_flags
        return out

    def run(self, ticks, record=False):
        """:meth:`step` ``ticks`` times; returns device tensors ``status`` and ``iters`` ``(ticks, batch)`` int32
        (a loop that polishes: and ``polish``, the verdicts, alike) and, with ``record``, ``given`` ``(ticks + 1, batch, ng)``: :attr:`given` before the first tick and after
        every tick (as :meth:`mpcasm.walkers.WalkerFleet.run` records them)."""
        torch, given = self._torch, self.given
        i32 = dict(dtype=torch.int32, device=given.device)
        status = torch.zeros((ticks, self.batch), **i32)
        iters = torch.zeros((ticks, self.batch), **i32)
        verdicts = torch.zeros((ticks, self.batch), **i32) if self.polish else None
        trail = torch.empty((ticks + 1,) + tuple(given.shape), dtype=given.dtype, device=given.device) \
            if record else None
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
        result = {"status": status, "iters": iters}
        if self.polish:
            result["polish"] = verdicts
        if record:
            result["given"] = trail
        return result
