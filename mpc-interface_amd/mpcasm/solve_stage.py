"""The solve stage of a closed loop: what :class:`mpcasm.walkers.WalkerFleet` (one stage per structure bucket, the
narrow solver) and :class:`mpcasm.ltv_loop.LtvLoop` (one stage, the wide solver) do between a tick's assembly and
its next ``given``, in this order:

    x0, y0, z0, rho0, one launch per shift group (warm)    start      engine.warm_start_qp
      ... or rho <- OSQP's default (not warm)
    x, y, z, status, iters, res                             solve      engine.solve_qp / solve_qp_wide
    x, y, z, res polished where solved (polish)             polish     engine.polish_qp / polish_qp_wide
    the solution into the warm store (warm)                 store      engine.warm_store_qp

Every step is a method of its own (a timing tool puts its events between them); :meth:`SolveStage.run` is the four in
order.  A launch covers the first ``count`` rows of the buffers -- all of them for the LTV loop; for the fleet a
bucket's walkers at this place of the step cycle, with their ``index`` into the warm store, on the bucket's stream."""
import contextlib

from .engine import (APPLY_ALL, APPLY_SOLVED, OSQP_RHO, WARM_SOLVED, WarmStore, polish_qp, polish_qp_wide,
                     qp_polish_wide_info, qp_solve_wide_info, qp_solve_wide_soft_info, soft_pair, solve_qp,
                     solve_qp_wide, warm_start_qp, warm_store_qp)


def stage_options(on_unsolved, polish, soft):
    """The checks of a loop's ``on_unsolved``, ``polish`` and ``soft`` (``ValueError``), on the host and before
    anything is compiled; returns the ``apply_mask`` of the loop's next ``given`` under ``on_unsolved``."""
    if soft is not None and polish:
        raise ValueError("polish= with soft=: the polish's active-set model is the hard problem's")
    if soft is not None and not callable(soft) and not (isinstance(soft, (tuple, list)) and len(soft) == 2):
        raise ValueError("soft: a pair (lin, quad) or a callable that takes an Assembler and returns one")
    if on_unsolved not in ("hold", "apply"):
        raise ValueError("on_unsolved: 'hold' or 'apply', got %r" % (on_unsolved,))
    return APPLY_SOLVED if on_unsolved == "hold" else APPLY_ALL


class SolveStage:
    """The solver's side of a closed loop on the QPs of ``asm`` (an :class:`~mpcasm.engine.Assembler`), ``rows``
    instances at most, everything at fixed addresses for every tick and every captured graph.

    ``wide``: :func:`~mpcasm.engine.solve_qp_wide` and :func:`~mpcasm.engine.polish_qp_wide`, with ``K^-1`` in a
    workspace of the stage's where it does not fit on chip (unless ``solver_kwargs`` bring a ``kinv``) and the
    polish's workspace.  ``on_unsolved``, ``polish``, ``warm``, ``soft``: the loops' options of these names
    (:func:`stage_options`); ``soft`` a pair or a callable that gets ``asm``, made one pair of ``(nc,)`` rows here.
    ``store``: the :class:`~mpcasm.engine.WarmStore` of a warm stage -- the fleet's, shared by its buckets; None:
    one of the stage's own, a record per row.  ``solver_kwargs`` go to the solver (``eps_abs``, ``max_iter``, ...).

    :attr:`buffers`: the tensors by name -- ``x (rows, no)``, ``y``, ``z (rows, nc)``, ``rho (rows,)``, ``res
    (rows, 2)`` float64, ``status``, ``iters (rows,)`` int32, with ``polish`` the verdicts ``polish (rows,)`` int32,
    with ``warm`` the flags ``warm (rows,)`` int32.  :attr:`solver_kwargs`: what every solve is called with beside
    its operands, ``rho``, ``out`` and ``warm`` (``soft``: the pair of rows; ``kinv``: the workspace).
    :attr:`polish_work`: the wide polish's workspace (None without).  :attr:`apply_mask`: see :func:`stage_options`."""

    def __init__(self, asm, rows, wide=False, on_unsolved="hold", polish=False, warm=False, soft=None, store=None,
                 **solver_kwargs):
        self.apply_mask = stage_options(on_unsolved, polish, soft)
        torch = self._torch = asm._torch
        self.wide, self.polishes, self.warm = bool(wide), bool(polish), bool(warm)
        f, i32 = dict(dtype=torch.float64, device=asm.device), dict(dtype=torch.int32, device=asm.device)
        B, no, nc = int(rows), asm.no, asm.nc
        self.buffers = dict(x=torch.zeros((B, no), **f), y=torch.zeros((B, nc), **f), z=torch.zeros((B, nc), **f),
                            status=torch.zeros(B, **i32), iters=torch.zeros(B, **i32), res=torch.zeros((B, 2), **f),
                            rho=torch.full((B,), OSQP_RHO, **f))
        self.solver_kwargs = dict(solver_kwargs)
        if soft is not None:      # (one pair of rows for every instance and tick)
            self.solver_kwargs["soft"] = soft_pair(soft(asm) if callable(soft) else soft, nc, asm.device)
        info = qp_solve_wide_info if soft is None else qp_solve_wide_soft_info
        if self.wide and "kinv" not in solver_kwargs and not info(no, nc)[1]:
            self.solver_kwargs["kinv"] = torch.empty((B, no, no), **f)
        self.polish_work = self.warm_store = None
        if self.polishes:
            self.buffers["polish"] = torch.zeros(B, **i32)
            if self.wide:
                self.polish_work = torch.empty((max(qp_polish_wide_info(no, nc, B)[1], 16) // 8,), **f)
        if self.warm:
            self.buffers["warm"] = torch.zeros(B, **i32)
            self.warm_store = store if store is not None else WarmStore(B, no, nc, asm.device)

    def start(self, G, h, groups, expect_tag, index=None, count=None, stream=None):
        """Where the solve starts.  Warm: per shift group ``(first, last + 1, col_src, row_src)`` of ``groups`` one
        :func:`~mpcasm.engine.warm_start_qp` on its rows, from the records tagged ``expect_tag`` (``index``: the
        rows' records in the store; None: record ``b`` for row ``b``).  Not warm: ``rho`` back to OSQP's default
        (the reference builds a fresh solver every tick)."""
        buf = self.buffers
        if not self.warm:
            with self._torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                buf["rho"][:count].fill_(OSQP_RHO)
            return
        for a, b, col_src, row_src in groups:
            warm_start_qp(self.warm_store, G[a:b], h[a:b], col_src, row_src, expect_tag,
                          index=index[a:b] if index is not None else None, warm_mask=WARM_SOLVED, rho_cold=OSQP_RHO,
                          stream=stream, out=tuple(buf[k][a:b] for k in ("x", "y", "z", "rho", "warm")))

    def solve(self, P, q, G, h, count=None, stream=None):
        """The solve of rows ``[:count]`` into the stage's buffers: a :class:`~mpcasm.engine.QpSolution` of views."""
        buf = self.buffers
        return (solve_qp_wide if self.wide else solve_qp)(
            P, q, G, h, rho=buf["rho"][:count], stream=stream, warm=self.warm,
            out=tuple(buf[k][:count] for k in ("x", "y", "z", "status", "iters", "res")), **self.solver_kwargs)

    def polish(self, P, q, G, h, sol, stream=None):
        """The polish of ``sol`` (of :meth:`solve`) where it is solved, in place; the verdicts into ``polish``."""
        out = (self.buffers["polish"][:sol.x.shape[0]], sol.res)
        if self.wide:
            return polish_qp_wide(P, q, G, h, sol, status=sol.status, stream=stream, out=out, work=self.polish_work)
        return polish_qp(P, q, G, h, sol, status=sol.status, stream=stream, out=out)

    def store(self, sol, tag, index=None, stream=None):
        """``sol`` into the warm store under ``tag``, whatever its status (``index`` as for :meth:`start`)."""
        warm_store_qp(self.warm_store, sol, tag, index=index, stream=stream)

    def run(self, P, q, G, h, groups=(), expect_tag=0, tag=0, index=None, count=None, stream=None):
        """:meth:`start`, :meth:`solve`, and where they are on :meth:`polish` and :meth:`store`, in this order.
        Returns ``{"x", "status", "iters"}`` -- with ``polish`` also ``"polish"``, with ``warm`` also ``"warm"`` --
        views of rows ``[:count]`` of the buffers, valid until the next run."""
        self.start(G, h, groups, expect_tag, index=index, count=count, stream=stream)
        sol = self.solve(P, q, G, h, count=count, stream=stream)
        if self.polishes:
            self.polish(P, q, G, h, sol, stream=stream)
        if self.warm:
            self.store(sol, tag, index=index, stream=stream)
        out = {"x": sol.x, "status": sol.status, "iters": sol.iters}
        for key in ("polish", "warm"):
            if key in self.buffers:
                out[key] = self.buffers[key][:count]
        return out
