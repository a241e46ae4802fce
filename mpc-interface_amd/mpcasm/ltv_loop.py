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
      (true_input=True: u is a state of the plan -- At, Bt, Kt by engine.ltv_augment, once)
    given <- x_1 = A_t x_0 + B_t u_0                   Assembler.advance           (csrc/rollout.hip)

-- the reference's tick (biped_mpc_loop.py:50-95: assemble, ``osqp_solve_qp``, ``preview_all`` +
``update_given_collector``) with per-step dynamics, nothing read back to the host.  The four rows from the warm start
to the warm store are the loop's solve stage (:class:`mpcasm.solve_stage.SolveStage`).  The loop runs launch by
launch: the window's address changes every tick, which a captured graph would not follow."""
import numpy as np

from .engine import Assembler, _ltv_sequences, ltv_augment, ltv_close, ltv_lqr
from .solve_stage import SolveStage, stage_options


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
    formulation WITHOUT ``true_input``: the unknowns are ``v`` -- a cost or a limit on the input variable is one on
    ``v``, the deviation from the feedback law, not on ``u``; costs and limits on states are unchanged, and so is
    the state the loop moves to (``A_cl_t x_0 + B_t v_0`` is the true ``A_t x_0 + B_t u_0``).  The results of a tick
    then carry ``"u"`` ``(B, axes, N, m)``, the true inputs of the plan just solved (:meth:`~mpcasm.engine.
    Assembler.true_inputs`).  ``warm`` and ``polish`` compose with it unchanged.
    ``true_input`` (keyword only, default False: nothing changes; needs ``feedback``): costs and limits on the TRUE
    input.  ``form`` is then written on the plant augmented by one delay, ``z = [x ; u_prev]`` with input ``v``
    (``mpcasm.problems.augment_matrices``, ``lipm_ltv_true_input``): sample ``k`` of its last ``m`` states is ``u_k
    = K_k x_k + v_k``, so a cost or a limit on those states is one on ``u`` -- input saturation among them.
    ``A_seq``, ``B_seq`` and the gains stay the PLANT's, ``n`` states and ``m`` inputs with ``n + m <= 4``;
    :func:`~mpcasm.engine.ltv_augment` builds ``At_seq``, ``Bt_seq`` and ``Kt_seq = [K | 0]`` once and their windows
    are bound every tick.  ``ValueError`` without ``feedback``, for a plan whose ``n`` is not the plant's ``n + m``,
    and for a dynamics whose nominal matrices do not have the augmented structure (the last ``m`` columns of ``A``
    zero, the last ``m`` rows of ``B`` the identity).  :attr:`given` is ``(B, axes (n + m))``: the last ``m`` slots
    of an axis hold the input applied at the last tick (zero before the first) -- they must be finite and are
    otherwise without influence on the plan, their columns of ``At`` being zero; after a tick an applied instance
    finds ``out["u"][:, :, 0]`` there, bit for bit, a held one what it had.  What stays out: ``n + m > 4``; limits
    on the input's RATE (they mix two steps' states); and the augmented pendulum runs the sweep kernel's generic
    instantiation, not the one compiled for 3 states.
    ``soft`` (keyword only, default None: nothing changes): soft limits (``engine.solve_qp_wide(soft=...)``).  A pair
    of scalars ``(lin, quad)`` makes every row soft -- a violation ``t > 0`` costs ``lin t + 1/2 quad t^2``; a
    callable gets the loop's :class:`~mpcasm.engine.Assembler` and returns ``(lin, quad)``, scalars or ``(nc,)``
    vectors (``asm.soft_rows({limit index: (lin, quad)})``; ``inf`` keeps a row hard).  The vectors are built once
    and passed at stride 0 on every tick.  ``warm`` composes unchanged; with ``polish`` it is a ``ValueError``.
    ``solver_kwargs`` go to :func:`~mpcasm.engine.solve_qp_wide` (``eps_abs``, ``max_iter``, ...)."""

    def __init__(self, form, name, batch, A_seq, B_seq, on_unsolved="hold", polish=False, **solver_kwargs):
        # (`warm=` is a keyword of its own, taken out of the solver's: the positional order up to `polish` stays)
        warm = solver_kwargs.pop("warm", False)
        feedback = solver_kwargs.pop("feedback", None)
        self.true_input = bool(solver_kwargs.pop("true_input", False))
        soft = solver_kwargs.pop("soft", None)
        self._apply_mask = stage_options(on_unsolved, polish, soft)
        if self.true_input:               # (decided on the host, from the formulation: before anything is compiled)
            self._check_true_input(form, name, A_seq, B_seq, feedback)
        self.on_unsolved = on_unsolved
        self.name, self.batch = name, int(batch)
        self.asm = asm = Assembler(form, batch=self.batch, ltv=[name])
        torch = self._torch = asm._torch
        self.A_seq, self.B_seq = A_seq, B_seq
        self.horizon = asm.plan.ltv[0]["N"]
        self.K_seq = None
        self._win = (A_seq, B_seq)          # (the sequences whose windows are bound: closed or augmented below)
        if self.true_input:
            self._augment(form, feedback)
        else:
            asm.bind_ltv_window(name, A_seq, B_seq, 0)      # (the sequences' shapes are checked here)
            if feedback is not None:
                self._close(feedback)
        self.ticks_possible = A_seq.shape[-3] - self.horizon + 1
        self.t = 0
        self.given = torch.zeros((self.batch, asm.ng), dtype=torch.float64, device=asm.device)
        # the solve stage (mpcasm.solve_stage): the wide solver's buffers, workspaces and warm store (a record per
        # instance, no index), at fixed addresses for every tick
        self.polish, self.warm = bool(polish), bool(warm)
        self.stage = SolveStage(asm, self.batch, wide=True, on_unsolved=on_unsolved, polish=polish, warm=warm,
                                soft=soft, **solver_kwargs)
        self._groups = ()
        if self.warm:                       # (the one shift map, built once: every instance is one group)
            from .warm import shift_map
            rows = [n for _, n in asm.plan.limit_rows]
            col, row = shift_map(form, form, False, horizon=self.horizon, prev_rows=rows, new_rows=rows)
            self._groups = [(0, self.batch) + tuple(torch.as_tensor(v, device=asm.device) for v in (col, row))]

    @staticmethod
    def _check_true_input(form, name, A_seq, B_seq, feedback):
        """``true_input=True``: ``ValueError`` without ``feedback``, for a dynamics whose states are not the
        plant's and its inputs, and for nominal matrices without the augmented structure."""
        if feedback is None:
            raise ValueError("true_input: the true input is a state of the plant closed by `feedback=`, which is "
                             "missing")
        mats = form.dynamics[name].matrices     # (U_j[0][0][i] = B[i][j], S[0][j][i] = A[i][j]: tools.py:14-33)
        nz, mz = np.asarray(mats[-1]).shape[-1], len(mats) - 1
        shape = lambda seq: tuple(getattr(seq, "shape", ()))
        n, m = (shape(A_seq) or (0,))[-1], (shape(B_seq) or (0,))[-1]
        if nz != n + m or mz != m:
            raise ValueError("true_input: the dynamics %r has %d states and %d input(s); the plant's %d states and "
                             "its %d input(s) make %d and %d" % (name, nz, mz, n, m, n + m, m))
        At = np.asarray(mats[-1])[0].T
        Bt = np.stack([np.asarray(mats[j])[0, 0, :] for j in range(m)], axis=1)
        if np.any(At[:, n:] != 0) or not np.array_equal(Bt[n:], np.eye(m)):
            raise ValueError("true_input: the nominal matrices of the dynamics %r are not those of a plant augmented "
                             "by its input (mpcasm.problems.augment_matrices): the last %d column(s) of A must be "
                             "zero and the last %d row(s) of B the identity" % (name, m, m))

    def _gains(self, feedback, n, m, close):
        """``feedback=`` on a plant of ``n`` states and ``m`` inputs: ``(K, K_seq, A_cl_seq)`` -- the gains as they
        were brought or swept, the same as a sequence ``(T, m, n)`` / ``(B, T, m, n)``, and with ``close`` ``A + B K``
        (else ``None``)."""
        torch, asm = self._torch, self.asm
        T = self.A_seq.shape[-3]
        if isinstance(feedback, dict):
            if not {"Q", "R"} <= set(feedback) <= {"Q", "R", "terminal"}:
                raise ValueError("feedback: the weights 'Q' and 'R' and, if wanted, 'terminal'; got %s"
                                 % sorted(feedback))
            K, Acl, info = ltv_lqr(self.A_seq, self.B_seq, feedback["Q"], feedback["R"], feedback.get("terminal"),
                                   want_closed=close)
            failed = torch.nonzero(info >= 0).flatten().tolist()
            if failed:
                raise ValueError("feedback: the Riccati sweep met a pivot that is not positive for instance(s) %s "
                                 "(at step(s) %s)" % (failed[:8], info[failed[:8]].tolist()))
            return K, K, Acl
        shapes = ((m, n), (self.batch, m, n), (self.batch, T, m, n))
        if not (torch.is_tensor(feedback) and feedback.dtype == torch.float64 and feedback.device == asm.device
                and feedback.is_contiguous() and tuple(feedback.shape) in shapes):
            raise ValueError("feedback: a contiguous float64 tensor of shape %s, %s or %s on %s, or the weights "
                             "{'Q': .., 'R': ..} of a Riccati sweep" % (shapes + (asm.device,)))
        Acl = ltv_close(self.A_seq, self.B_seq, feedback) if close else None
        K = feedback
        if K.dim() < 4:      # (one gain for every step: true_inputs takes its window of a sequence)
            K = (K if K.dim() == 3 else K[None])[:, None].expand(-1, T, m, n).contiguous()
            K = K[0] if feedback.dim() == 2 else K
        return feedback, K, Acl

    def _close(self, feedback):
        """``feedback=``: the gains as ``K_seq (T, m, n)`` / ``(B, T, m, n)``, and ``A_cl_seq`` in ``A_seq``'s place."""
        torch, asm = self._torch, self.asm
        g = asm.plan.ltv[0]
        _, self.K_seq, self.A_cl_seq = self._gains(feedback, g["n"], g["m"], True)
        self._win = (self.A_cl_seq, self.B_seq)
        self._gain_seq = self.K_seq
        self._u = torch.zeros((self.batch, asm.plan.sweep["axes"].shape[0], self.horizon, g["m"]),
                              dtype=torch.float64, device=asm.device)

    def _augment(self, form, feedback):
        """``true_input=True``: the gains on the plant's ``(n, m)``, and ``At_seq``, ``Bt_seq``,
        ``Kt_seq`` (:func:`~mpcasm.engine.ltv_augment`, once) in ``A_seq``'s, ``B_seq``'s and the gains' place."""
        torch, asm = self._torch, self.asm
        n, m = _ltv_sequences(torch, self.A_seq, self.B_seq)[:2]
        K, self.K_seq, _ = self._gains(feedback, n, m, False)
        self.At_seq, self.Bt_seq, self.Kt_seq = ltv_augment(self.A_seq, self.B_seq, K)
        self._win = (self.At_seq, self.Bt_seq)
        self._gain_seq = self.Kt_seq
        asm.bind_ltv_window(self.name, self.At_seq, self.Bt_seq, 0)
        axes = np.asarray(asm.plan.sweep["axes"])
        self._u = torch.zeros((self.batch, axes.shape[0], self.horizon, m), dtype=torch.float64, device=asm.device)
        # the slots of `given` that hold the last input of every axis, and which statuses the advance applies
        slots = [int(c0) + n + j for c0 in axes[:, 0] for j in range(m)]
        self._slots = torch.as_tensor(slots, dtype=torch.int64, device=asm.device)
        self._applies = torch.as_tensor([bool((self._apply_mask >> bit) & 1) for bit in range(32)] + [False],
                                        device=asm.device)

    def step(self):
        """One tick on :attr:`given`: the window at ``t``, the assembly, a cold solve, the next ``given`` by the
        loop's ``on_unsolved`` rule; then ``t`` advances.  Nothing is read back: returns ``{"x", "status",
        "iters"}`` (a loop that polishes: and ``"polish"``; one with ``feedback``: and ``"u"``), device tensors in the loop's own buffers, valid until
        the next step."""
        if self.t >= self.ticks_possible:
            raise ValueError("the sequences hold %d steps: no window of %d steps starts at tick %d"
                             % (self.A_seq.shape[-3], self.horizon, self.t))
        asm = self.asm
        asm.bind_ltv_window(self.name, self._win[0], self._win[1], self.t)
        P, q, G, h = asm.assemble(self.given)
        if G is None:                      # (a plan without limits: the solver takes G and h of no rows)
            G, h = P.new_empty((self.batch, 0, asm.no)), P.new_empty((self.batch, 0))
        # (the tag is the tick + 1: a record is one tick old or not warm)
        out = self.stage.run(P, q, G, h, groups=self._groups, expect_tag=self.t, tag=self.t + 1)
        if self.K_seq is not None:         # (from the tick's initial states: before they advance)
            asm.true_inputs(self._gain_seq, self.t, self.given, out["x"], out=self._u)
            out["u"] = self._u
        asm.advance(self.given, out["x"], status=out["status"], apply_mask=self._apply_mask)
        if self.true_input:
            # the advance's own K x_0 + v_0 sums the same products in another order (its last bit may differ):
            # an applied instance's slots get the very numbers the results report
            applied = self._applies[out["status"].abs().clamp_(max=32).long()]
            self.given[:, self._slots] = self._torch.where(applied[:, None], self._u[:, :, 0].reshape(self.batch, -1),
                                                           self.given[:, self._slots])
        self.t += 1
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
