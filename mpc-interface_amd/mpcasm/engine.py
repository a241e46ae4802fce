"""Batched QP assembly on one MI355X: torch-ROCm tensors as device buffers, the
kernels of libmpcasm.so through the C ABI (``mpcasm.capi``).

* :func:`fill_su` -- K1, batched ``tools.extend_matrices`` (tools.py:14-33)
* :class:`Assembler` -- K2+K3+K4 for a batch of instances of one Formulation
  structure: ``assemble(given)`` returns the qpsolvers blocks
  ``P (B,no,no), q (B,no), G (B,nc,no), h (B,nc)`` (body.py:333-348) and
  ``preview_matrices()`` the stacked ``[Mg | Mo]`` of every definition
  (body.py:149-193).

torch is used for memory, streams and ``data_ptr()`` only; nothing here
computes on the host and nothing falls back to the CPU.
"""
import collections
import contextlib
import ctypes

import numpy as np

from . import capi
from .plan import compile_plan, is_causal, rollout_rows, rollout_sizes, soft_rows


def _torch():
    import torch

    return torch


def require_device():
    """The torch module, after checking that a HIP device is usable."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError(
            "mpcasm: no HIP device is visible; the QP-assembly path runs only on the GPU "
            "(there is no CPU fallback)")
    capi.load()
    return torch


def _stream_handle(torch, stream):
    if stream is None:      # (the raw handle of the current stream: no Stream object per launch)
        try:
            return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))
        except AttributeError:
            stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def _as_device(torch, x, device):
    """float64 contiguous device tensor from a tensor or array."""
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=device)


def _tensor(torch, t, dtype, shape, device, what, at_least=False):
    """``t`` where it is a contiguous tensor of ``dtype`` and ``shape`` on ``device``, else ``ValueError(what)`` -- or,
    for a caller with more to ask and a text of its own, None where ``what`` is None.  ``shape``: None for any, or a
    tuple whose None entries stand for any size; ``at_least``: ``shape[0]`` is the fewest rows.  ``device``: None for
    any HIP device."""
    ok = isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous() \
        and (t.is_cuda if device is None else t.device == device)
    if ok and shape is not None:
        ok = t.dim() == len(shape) and all(
            want is None or have == want or (at_least and i == 0 and have > want)
            for i, (have, want) in enumerate(zip(t.shape, shape)))
    if not ok and what is not None:
        raise ValueError(what)
    return t if ok else None


def _iterates(sol_or_xyz):
    """``x, y, z, res`` of a :class:`QpSolution` or of ``(x, y, z)`` (``res`` None)."""
    if isinstance(sol_or_xyz, (QpSolution, PolishedQpSolution)):
        return sol_or_xyz.x, sol_or_xyz.y, sol_or_xyz.z, sol_or_xyz.res
    x, y, z = sol_or_xyz
    return x, y, z, None


def _wide_work(torch, info, no, nc, batch, work, device):
    """The workspace of a wide KKT solve as the entry takes it, ``(address, bytes)``: sized by ``info`` (the entry's
    ``*_wide_info``), allocated when ``work`` is None."""
    need = info(no, nc, batch)[1]
    if work is None:
        work = torch.empty((max(need, 16) // 8,), dtype=torch.float64, device=device)
    if _tensor(torch, work, torch.uint8, None, device, None) is None:
        _tensor(torch, work, torch.float64, None, device, "work: a contiguous uint8 or float64 tensor on P's device")
    return work.data_ptr(), work.numel() * work.element_size()


def _query(entry, args, *outs):
    """A host-only size query of the C boundary: ``entry`` called with the integers ``args`` and one out-parameter
    per ctypes type of ``outs``; ``MpcasmError`` where it refuses, else the values it wrote, as ints."""
    outs = [kind() for kind in outs]
    capi.check(getattr(capi.load(), entry)(*(int(a) for a in args), *(ctypes.byref(o) for o in outs)), entry)
    return tuple(int(o.value) for o in outs)


# --------------------------------------------------------------------------
# K1
# --------------------------------------------------------------------------
def fill_su(A, B, N, ltv=False, out=None, stream=None, device=None):
    """Horizon matrices of a batch of systems (``mpcasm_fill_su``).

    ``A``: ``(B, n, n)`` and ``B``: ``(B, n, m)`` (or ``(B, N, n, n)`` /
    ``(B, N, n, m)`` when ``ltv``).  Returns device tensors ``S (B, N, n, n)``
    and ``U (B, m, N, N, n)`` with ``U[b, j]`` = the reference's ``U[j]``.
    """
    torch = require_device()
    if device is None:
        device = A.device if isinstance(A, torch.Tensor) and A.is_cuda else torch.device(
            "cuda", torch.cuda.current_device())
    A = _as_device(torch, A, device)
    Bm = _as_device(torch, B, device)
    N = int(N)
    if ltv:
        if A.dim() != 4 or Bm.dim() != 4 or A.shape[1] != N or Bm.shape[1] != N:
            raise ValueError("ltv fill needs A (B,N,n,n) and B (B,N,n,m)")
        batch, _, n, m = Bm.shape
    else:
        if A.dim() != 3 or Bm.dim() != 3:
            raise ValueError("fill needs A (B,n,n) and B (B,n,m)")
        batch, n, m = Bm.shape
    if A.shape[-2:] != (n, n) or A.shape[0] != batch:
        raise ValueError("A %s does not match B %s" % (tuple(A.shape), tuple(Bm.shape)))
    if out is None:
        S = torch.empty((batch, N, n, n), dtype=torch.float64, device=device)
        U = torch.empty((batch, m, N, N, n), dtype=torch.float64, device=device)
    else:
        S, U = out
    with torch.cuda.device(device):
        rc = capi.load().mpcasm_fill_su(
            A.data_ptr(), Bm.data_ptr(), S.data_ptr(), U.data_ptr(), batch, N, n, m,
            1 if ltv else 0, _stream_handle(torch, stream))
    capi.check(rc, "mpcasm_fill_su")
    return S, U


FillRoute = collections.namedtuple("FillRoute", "kernel arg flags spw lshift grid lds whole_lds")


def fill_route(batch, N, n, m, ltv=False, aligned16=True):
    """What :func:`fill_su` launches for ``batch`` systems of these sizes -- ``mpcasm_fill_route``, the launch's
    own decision, no device needed.  ``aligned16``: whether ``S`` and ``U`` both start on a 16-byte boundary
    (tensors of their own do; views at an odd element offset do not).  A :class:`FillRoute`: ``kernel`` one of
    ``capi.FILL_*``; ``arg`` the kernel's integer template argument (``NS`` or ``TPI``); ``flags`` of
    ``capi.FILL_GENERIC | FILL_PAD | FILL_WHOLE_LINES``; ``spw`` systems per wavefront; ``lshift`` of the quad
    kernel; ``grid`` workgroups; ``lds`` bytes and ``whole_lds`` (more than 64 KB).  Raises
    :class:`capi.MpcasmError` with ``MPCASM_ERR_LIMIT`` where the launch refuses the sizes."""
    out = (ctypes.c_int32 * 8)()
    capi.check(capi.load().mpcasm_fill_route(int(batch), int(N), int(n), int(m), 1 if ltv else 0,
                                             1 if aligned16 else 0, out), "mpcasm_fill_route")
    return FillRoute(*(int(x) for x in out))


def fill_su_numpy(A, B, N, ltv=False):
    """:func:`fill_su` with numpy in / numpy out (single-instance drop-in path)."""
    S, U = fill_su(A, B, N, ltv=ltv)
    return S.cpu().numpy(), U.cpu().numpy()


# --------------------------------------------------------------------------
# K5: the solve after the assembly (the "or")
# --------------------------------------------------------------------------
OSQP_RHO, OSQP_SIGMA, OSQP_ALPHA = 0.1, 1e-6, 1.6     # OSQP's default steps


def _qp_operands(torch, P, q, G, h, x, y, z, kinv, kinv_valid):
    """The checks :func:`admm` and :func:`solve_qp` share: ``batch, no, nc, warm, x, y, z`` with the
    iterates of a cold start allocated."""
    for t in (P, q, G, h):
        _tensor(torch, t, torch.float64, None, None, "P, q, G, h: contiguous float64 device tensors")
    if P.dim() != 3 or P.shape[1] != P.shape[2] or q.shape != P.shape[:2] or G.dim() != 3 or \
            G.shape[0] != P.shape[0] or G.shape[2] != P.shape[1] or h.shape != G.shape[:2]:
        raise ValueError("shapes: P (B, no, no), q (B, no), G (B, nc, no), h (B, nc)")
    batch, no, nc = P.shape[0], P.shape[1], G.shape[1]
    warm = x is not None or y is not None or z is not None
    if warm:
        if x is None or y is None or z is None:
            raise ValueError("a warm start takes x, y and z")
        for t, shape in ((x, (batch, no)), (y, (batch, nc)), (z, (batch, nc))):
            _tensor(torch, t, torch.float64, shape, P.device,
                    "x (B, no), y (B, nc), z (B, nc): contiguous float64 tensors on P's device")
    else:
        x = torch.empty((batch, no), dtype=torch.float64, device=P.device)
        y = torch.empty((batch, nc), dtype=torch.float64, device=P.device)
        z = torch.empty((batch, nc), dtype=torch.float64, device=P.device)
    if kinv is not None:
        _tensor(torch, kinv, torch.float64, (batch, no, no), P.device,
                "kinv: a contiguous float64 (B, no, no) tensor on P's device")
    if kinv_valid and kinv is None:
        raise ValueError("kinv_valid without kinv")
    return batch, no, nc, warm, x, y, z


def admm(P, q, G, h, x=None, y=None, z=None, iters=50, rho=OSQP_RHO, sigma=OSQP_SIGMA, alpha=OSQP_ALPHA,
         residuals=True, stream=None, kinv=None, kinv_valid=False):
    """``iters`` iterations of OSQP's ADMM on a batch of dense QPs ``min 1/2 x'Px + q'x s.t. Gx <= h``
    (``mpcasm_admm``) -- the solver call of the walking loop, ``osqp_solve_qp(P=Q, q=q, G=A, h=h)``
    (biped_mpc_loop.py:60), on the device tensors :meth:`Assembler.assemble` returns: ``P (B, no, no)``,
    ``q (B, no)``, ``G (B, nc, no)``, ``h (B, nc)``.  ``x, y, z``: the iterates of a warm start (all three,
    device tensors, updated IN PLACE) or None for a cold start.  Returns ``x, y, z, res`` with
    ``res (B, 2)`` = OSQP's primal and dual residuals (None when ``residuals`` is off).
    ``kinv``: a ``(B, no, no)`` device tensor for the inverse of ``P + sigma I + rho G'G`` -- written by this call,
    or, with ``kinv_valid``, read instead of factoring (``P``, ``G``, ``rho``, ``sigma`` unchanged since the call that
    wrote it: a new ``given`` on the same model changes ``q`` and ``h`` only)."""
    torch = require_device()
    batch, no, nc, warm, x, y, z = _qp_operands(torch, P, q, G, h, x, y, z, kinv, kinv_valid)
    res = torch.empty((batch, 2), dtype=torch.float64, device=P.device) if residuals else None
    with torch.cuda.device(P.device):
        rc = capi.load().mpcasm_admm(no, nc, P.data_ptr(), q.data_ptr(), G.data_ptr(), h.data_ptr(),
                                     x.data_ptr(), y.data_ptr(), z.data_ptr(),
                                     res.data_ptr() if residuals else None, float(rho), float(sigma),
                                     float(alpha), int(iters), 1 if warm else 0, batch,
                                     kinv.data_ptr() if kinv is not None else None, 1 if kinv_valid else 0,
                                     _stream_handle(torch, stream))
    capi.check(rc, "mpcasm_admm")
    return x, y, z, res


QP_SOLVED, QP_MAX_ITER, QP_PRIMAL_INFEASIBLE, QP_DUAL_INFEASIBLE, QP_NON_CVX = (
    capi.QP_SOLVED, capi.QP_MAX_ITER, capi.QP_PRIMAL_INFEASIBLE, capi.QP_DUAL_INFEASIBLE, capi.QP_NON_CVX)
POLISH_DONE, POLISH_SKIPPED, POLISH_REJECTED = capi.POLISH_DONE, capi.POLISH_SKIPPED, capi.POLISH_REJECTED
OSQP_DELTA, OSQP_POLISH_REFINE = 1e-6, 3              # OSQP's defaults for the polishing step


class QpSolution(collections.namedtuple("QpSolution", "x y z status iters res rho")):
    """What :func:`solve_qp` returns; ``polish`` is None: nothing was polished."""
    __slots__ = ()
    polish = None


class PolishedQpSolution(collections.namedtuple("QpSolution", "x y z status iters res rho polish")):
    """:class:`QpSolution` of ``solve_qp(..., polish=True)``: a trailing field ``polish``, the ``(B,)`` int32 verdicts
    ``POLISH_*`` of :func:`polish_qp`."""
    __slots__ = ()


def solve_qp(P, q, G, h, x=None, y=None, z=None, rho=OSQP_RHO, eps_abs=1e-3, eps_rel=1e-3, eps_prim_inf=1e-4,
             eps_dual_inf=1e-4, max_iter=4000, check_every=25, adaptive_rho_interval=100, sigma=OSQP_SIGMA,
             alpha=OSQP_ALPHA, kinv=None, kinv_valid=False, stream=None, out=None, polish=False, warm=False,
             soft=None):
    """A batch of dense QPs ``min 1/2 x'Px + q'x s.t. Gx <= h`` solved to tolerance on the device
    (``mpcasm_qp_solve``): :func:`admm`'s iteration with OSQP's termination tests and adaptive rho, every
    instance stopping on its own, nothing read back to the host (a tick can be captured in a graph).
    Operands, warm start and ``kinv`` as for :func:`admm`, except that ``P`` is read also with ``kinv_valid``.
    ``rho``: a float, or a ``(B,)`` float64 device tensor of per-instance steps, updated IN PLACE to the step
    each instance ended with (``kinv`` then holds the inverse for it: pass both to the next tick).
    The defaults are OSQP's, except ``adaptive_rho_interval``: OSQP picks its interval from timing, a fixed
    one keeps the result deterministic (0: rho stays).  Returns a :class:`QpSolution`
    ``(x, y, z, status, iters, res, rho)``: ``status`` and ``iters`` ``(B,)`` int32 (``QP_*``), ``res`` ``(B, 2)``
    the primal and dual residuals of the returned iterate.
    ``out``: for a COLD start, the caller's ``(x, y, z, status, iters, res)`` to write instead of new tensors
    (``(B, no)``, ``(B, nc)``, ``(B, nc)``, ``(B,)`` int32 twice, ``(B, 2)``: a loop that replays a graph keeps
    them at fixed addresses); ``x, y, z`` are not read -- unless ``warm``: then ``out``'s ``x, y, z`` hold the
    start, as :func:`warm_start_qp` wrote it (cold instances among them), and ``rho`` the steps beside it.
    ``polish``: :func:`polish_qp` with OSQP's defaults after the solve, on the solved instances; ``x, y, z`` and
    ``res`` of an instance whose polished point is accepted are that point's, and the solution grows a trailing field
    ``polish``, the ``(B,)`` int32 verdicts ``POLISH_*`` (a :class:`PolishedQpSolution`; without polish ``sol.polish``
    is None and the solution has the seven fields it always had).
    ``soft``: ``(lin, quad)``, soft limits through ``mpcasm_qp_solve_soft`` -- row ``i`` may be violated by
    ``t = (Gx - h)_i > 0`` at the price ``lin_i t + 1/2 quad_i t^2``; each a scalar or a tensor or array of shape
    ``(nc,)`` (one pair for the batch) or ``(B, nc)``; ``lin_i = inf`` keeps row ``i`` hard.  A soft row takes no part
    in the primal-infeasibility verdict; an instance with a negative or NaN penalty, or an infinite ``quad``, is
    ``QP_NON_CVX``.  None: today's entry with today's arguments.  Not with ``polish`` (``ValueError``): the polish
    models the hard problem.  Scalars and arrays are copied to the device here, on torch's current stream, in
    tensors that are freed on return: a caller that passes ``stream=`` or captures a graph must pass contiguous
    float64 DEVICE tensors (:meth:`Assembler.soft_rows`), which are handed on as they are."""
    return _solve_qp("mpcasm_qp_solve", P, q, G, h, x, y, z, rho, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf,
                     max_iter, check_every, adaptive_rho_interval, sigma, alpha, kinv, kinv_valid, stream, out,
                     warm_out=warm, soft=soft, polish=polish_qp if polish else None)


def polish_qp(P, q, G, h, sol_or_xyz, status=None, delta=OSQP_DELTA, refine_iters=OSQP_POLISH_REFINE, stream=None,
              out=None):
    """OSQP's solution polishing on a batch of iterates (``mpcasm_qp_polish``): per instance, the active set
    guessed from the iterate (row ``i`` iff ``h_i - z_i < y_i``), the KKT system of the equality-constrained QP
    on it solved with the regularisation ``delta`` and ``refine_iters`` steps of iterative refinement, and the
    result kept when OSQP's rule calls it the better point and no multiplier is negative.
    ``sol_or_xyz``: a :class:`QpSolution` or ``(x, y, z)`` -- device tensors, updated IN PLACE where a polished
    point is accepted, untouched elsewhere.  ``status``: ``(B,)`` int32, only ``QP_SOLVED`` instances are
    polished (None: every instance).  Returns ``(x, y, z, polish, res)``: ``polish`` ``(B,)`` int32
    (``POLISH_DONE`` / ``POLISH_SKIPPED`` / ``POLISH_REJECTED``) and ``res`` ``(B, 2)``, written for accepted
    instances only.  ``res`` is the solution's own when one is passed (else a new tensor of NaN).
    ``out``: the caller's ``(polish, res)`` to write instead (fixed addresses for a replayed graph)."""
    return _polish_qp("mpcasm_qp_polish", P, q, G, h, sol_or_xyz, status, delta, refine_iters, stream, out)


def qp_polish_lds_bytes(no, nc):
    """LDS bytes one instance of :func:`polish_qp` takes; ``MpcasmError`` with ``ERR_LIMIT`` when that is more
    than a workgroup may have (``mpcasm_qp_polish_lds_bytes``)."""
    return _query("mpcasm_qp_polish_lds_bytes", (no, nc), ctypes.c_int64)[0]


def polish_qp_wide(P, q, G, h, sol_or_xyz, status=None, delta=OSQP_DELTA, refine_iters=OSQP_POLISH_REFINE,
                   stream=None, out=None, work=None):
    """:func:`polish_qp` for QPs whose matrices do not fit on chip (``mpcasm_qp_polish_wide``): the same arguments,
    steps, verdicts and return value, up to 512 unknowns and 2 048 limits, for the iterates of
    :func:`solve_qp_wide`.  ``G`` and ``P`` are read in place; the matrices of the KKT solve live in ``work``, a
    contiguous uint8 or float64 device tensor of at least ``qp_polish_wide_info(no, nc, B)[1]`` bytes -- sized by
    the launch's workgroups, not by the batch -- allocated here when None (a loop that replays a graph keeps one at
    a fixed address; calls that may run at once need one each).  The polished points equal :func:`polish_qp`'s up
    to rounding."""
    return _polish_qp("mpcasm_qp_polish_wide", P, q, G, h, sol_or_xyz, status, delta, refine_iters, stream, out,
                      wide=True, work=work)


def _polish_qp(entry, P, q, G, h, sol_or_xyz, status, delta, refine_iters, stream, out, wide=False, work=None):
    """:func:`polish_qp` and :func:`polish_qp_wide` through the C entry ``entry``; ``wide``: the entry takes the
    workspace ``work`` (allocated when None) and its size in bytes."""
    torch = require_device()
    x, y, z, res = _iterates(sol_or_xyz)
    if x is None or y is None or z is None:
        raise ValueError("%s takes the iterates x, y and z" % ("polish_qp_wide" if wide else "polish_qp"))
    batch, no, nc, _warm, x, y, z = _qp_operands(torch, P, q, G, h, x, y, z, None, False)
    verdict = None
    if out is not None:
        verdict, res = out
    if verdict is None:
        verdict = torch.empty((batch,), dtype=torch.int32, device=P.device)
    if res is None:
        res = torch.full((batch, 2), float("nan"), dtype=torch.float64, device=P.device)
    for t, dtype, shape in ((verdict, torch.int32, (batch,)), (res, torch.float64, (batch, 2))) + \
            (((status, torch.int32, (batch,)),) if status is not None else ()):
        _tensor(torch, t, dtype, shape, P.device,
                "status, polish (B,) int32 and res (B, 2) float64: contiguous, on P's device")
    extra = _wide_work(torch, qp_polish_wide_info, no, nc, batch, work, P.device) if wide else ()
    with torch.cuda.device(P.device):
        rc = getattr(capi.load(), entry)(no, nc, P.data_ptr(), q.data_ptr(), G.data_ptr(), h.data_ptr(),
                                         x.data_ptr(), y.data_ptr(), z.data_ptr(),
                                         status.data_ptr() if status is not None else None, float(delta),
                                         int(refine_iters), verdict.data_ptr(), res.data_ptr(), batch, *extra,
                                         _stream_handle(torch, stream))
    capi.check(rc, entry)
    return x, y, z, verdict, res


def qp_polish_wide_info(no, nc, batch):
    """``(lds_bytes, work_bytes, workgroups)`` of :func:`polish_qp_wide` on ``batch`` instances: the LDS of a
    workgroup, the workspace the call needs and the workgroups it launches, ``min(batch, capi.POLISH_WIDE_CAP)``;
    ``MpcasmError`` with ``ERR_LIMIT`` past its size limit (``mpcasm_qp_polish_wide_info``).  Needs no device."""
    return _query("mpcasm_qp_polish_wide_info", (no, nc, batch), ctypes.c_int64, ctypes.c_int64, ctypes.c_int32)


# ---- the derivative of a solve: one more solve with the polish's KKT system --------------------------------------
SENS_DONE, SENS_SKIPPED, SENS_SINGULAR = capi.SENS_DONE, capi.SENS_SKIPPED, capi.SENS_SINGULAR

QpSensitivity = collections.namedtuple("QpSensitivity", "u w gP gG verdict lres")
QpVjp = collections.namedtuple("QpVjp", "gq gh gP gG verdict")
QpJvp = collections.namedtuple("QpJvp", "dx dy verdict")


def qp_sensitivity(P, G, h, sol_or_xyz, rx, ry, status=None, delta=OSQP_DELTA, refine_iters=OSQP_POLISH_REFINE,
                   want_P=False, want_G=False, out=None, stream=None):
    """The sensitivity solve of a batch of solved QPs (``mpcasm_qp_sens``): per instance, the active set guessed
    from the iterate by the polish's test (row ``i`` iff ``h_i - z_i < y_i``), ``K = [[P, G_A'], [G_A, 0]]``, and
    ``[u; w_A] = K^-1 [rx; ry_A]`` by the polish's regularised solve with ``refine_iters`` steps of refinement;
    ``w`` is 0 off the active set.  ``K`` is symmetric, so this one solve is the adjoint (:func:`qp_vjp`) and the
    forward derivative (:func:`qp_jvp`) alike.
    ``sol_or_xyz``: a :class:`QpSolution` or ``(x, y, z)``, only read -- best a polished one: the derivative is the
    active-set model's at that point.  ``rx (B, no)``, ``ry (B, nc)``: contiguous float64 device tensors.
    ``status``: ``(B,)`` int32, only ``QP_SOLVED`` instances are taken (None: every instance).
    Returns a :class:`QpSensitivity` ``(u, w, gP, gG, verdict, lres)``: ``u (B, no)``, ``w (B, nc)``; with
    ``want_P`` / ``want_G`` the dense ``gP = -1/2 (u x' + x u')`` ``(B, no, no)`` and ``gG`` ``(B, nc, no)``, row ``i``
    ``-(y_i u' + w_i x')`` on active rows and 0 elsewhere (else None); ``verdict (B,)`` int32 (``SENS_DONE`` /
    ``SENS_SKIPPED`` / ``SENS_SINGULAR``); ``lres (B,)`` the residual ``|r - K t|_inf`` of the solve: large where the
    active rows are dependent or a row is weakly active, and ``w`` then depends on ``delta``.  An instance that is
    not ``SENS_DONE`` is not written; tensors allocated here start at zero, so it reads as a zero gradient.
    ``out``: the caller's ``(u, w, gP, gG, verdict, lres)`` to write instead (fixed addresses for a replayed graph;
    a None among them is allocated here, ``gP`` / ``gG`` only when wanted)."""
    return _qp_sens("mpcasm_qp_sens", P, G, h, sol_or_xyz, rx, ry, status, delta, refine_iters, want_P, want_G, out,
                    stream)


def qp_sensitivity_wide(P, G, h, sol_or_xyz, rx, ry, status=None, delta=OSQP_DELTA, refine_iters=OSQP_POLISH_REFINE,
                        want_P=False, want_G=False, out=None, stream=None, work=None):
    """:func:`qp_sensitivity` for QPs whose matrices do not fit on chip (``mpcasm_qp_sens_wide``), the iterates of
    :func:`solve_qp_wide`: the same arguments and results with :func:`polish_qp_wide`'s method and ``work``, at least
    ``qp_sens_wide_info(no, nc, B)[1]`` bytes (allocated here when None)."""
    return _qp_sens("mpcasm_qp_sens_wide", P, G, h, sol_or_xyz, rx, ry, status, delta, refine_iters, want_P, want_G,
                    out, stream, wide=True, work=work)


def _qp_sens(entry, P, G, h, sol_or_xyz, rx, ry, status, delta, refine_iters, want_P, want_G, out, stream, wide=False,
             work=None):
    """:func:`qp_sensitivity` and :func:`qp_sensitivity_wide` through the C entry ``entry``."""
    torch = require_device()
    x, y, z, _ = _iterates(sol_or_xyz)
    for t in (P, G, h):
        _tensor(torch, t, torch.float64, None, None, "P, G, h: contiguous float64 device tensors")
    if P.dim() != 3 or P.shape[1] != P.shape[2] or G.dim() != 3 or G.shape[0] != P.shape[0] or \
            G.shape[2] != P.shape[1] or h.shape != G.shape[:2]:
        raise ValueError("shapes: P (B, no, no), G (B, nc, no), h (B, nc)")
    batch, no, nc = P.shape[0], P.shape[1], G.shape[1]
    f64, i32 = dict(dtype=torch.float64, device=P.device), dict(dtype=torch.int32, device=P.device)
    u = w = gP = gG = verdict = lres = None
    if out is not None:
        u, w, gP, gG, verdict, lres = out
    u = torch.zeros((batch, no), **f64) if u is None else u
    w = torch.zeros((batch, nc), **f64) if w is None else w
    if gP is None and want_P:
        gP = torch.zeros((batch, no, no), **f64)
    if gG is None and want_G:
        gG = torch.zeros((batch, nc, no), **f64)
    verdict = torch.zeros((batch,), **i32) if verdict is None else verdict
    lres = torch.zeros((batch,), **f64) if lres is None else lres
    checked = [(x, torch.float64, (batch, no)), (y, torch.float64, (batch, nc)), (z, torch.float64, (batch, nc)),
               (rx, torch.float64, (batch, no)), (ry, torch.float64, (batch, nc)), (u, torch.float64, (batch, no)),
               (w, torch.float64, (batch, nc)), (verdict, torch.int32, (batch,)), (lres, torch.float64, (batch,))]
    checked += [(status, torch.int32, (batch,))] if status is not None else []
    checked += [(gP, torch.float64, (batch, no, no))] if gP is not None else []
    checked += [(gG, torch.float64, (batch, nc, no))] if gG is not None else []
    for t, dtype, shape in checked:
        _tensor(torch, t, dtype, shape, P.device,
                "x, rx, u (B, no), y, z, ry, w (B, nc), gP (B, no, no), gG (B, nc, no), lres (B,) float64 "
                "and status, verdict (B,) int32: contiguous, on P's device")
    extra = _wide_work(torch, qp_sens_wide_info, no, nc, batch, work, P.device) if wide else ()
    ptr = lambda t: t.data_ptr() if t is not None else None
    with torch.cuda.device(P.device):
        rc = getattr(capi.load(), entry)(no, nc, P.data_ptr(), G.data_ptr(), h.data_ptr(), x.data_ptr(), y.data_ptr(),
                                         z.data_ptr(), ptr(status), rx.data_ptr(), ry.data_ptr(), float(delta),
                                         int(refine_iters), u.data_ptr(), w.data_ptr(), ptr(gP), ptr(gG),
                                         verdict.data_ptr(), lres.data_ptr(), batch, *extra,
                                         _stream_handle(torch, stream))
    capi.check(rc, entry)
    return QpSensitivity(u, w, gP, gG, verdict, lres)


def qp_sens_lds_bytes(no, nc):
    """LDS bytes one instance of :func:`qp_sensitivity` takes -- :func:`qp_polish_lds_bytes`' figure and limit
    (``mpcasm_qp_sens_lds_bytes``).  Needs no device."""
    return _query("mpcasm_qp_sens_lds_bytes", (no, nc), ctypes.c_int64)[0]


def qp_sens_wide_info(no, nc, batch):
    """``(lds_bytes, work_bytes, workgroups)`` of :func:`qp_sensitivity_wide` on ``batch`` instances --
    :func:`qp_polish_wide_info`'s figures and limit (``mpcasm_qp_sens_wide_info``).  Needs no device."""
    return _query("mpcasm_qp_sens_wide_info", (no, nc, batch), ctypes.c_int64, ctypes.c_int64, ctypes.c_int32)


def qp_vjp(P, G, h, sol_or_xyz, gx, gy, status=None, delta=OSQP_DELTA, refine_iters=OSQP_POLISH_REFINE, want_P=False,
           want_G=False, wide=False, stream=None, work=None):
    """The adjoint of a solve: for a loss with ``dL/dx = gx (B, no)`` and ``dL/dy = gy (B, nc)`` at the solution
    ``sol_or_xyz``, a :class:`QpVjp` ``(gq, gh, gP, gG, verdict)`` = ``(-u, w, -1/2 (u x' + x u'), -(y u' + w x') on
    the active rows, SENS_*)`` of one :func:`qp_sensitivity` call (``wide``: :func:`qp_sensitivity_wide`); ``gP`` is
    the gradient with respect to a symmetric ``P``.  An instance that is not ``SENS_DONE`` has zero gradients."""
    call = qp_sensitivity_wide if wide else qp_sensitivity
    kw = dict(work=work) if wide else {}
    s = call(P, G, h, sol_or_xyz, gx, gy, status=status, delta=delta, refine_iters=refine_iters, want_P=want_P,
             want_G=want_G, stream=stream, **kw)
    return QpVjp(-s.u, s.w, s.gP, s.gG, s.verdict)


def qp_jvp(P, G, h, sol_or_xyz, dq, dh, dP=None, dG=None, status=None, delta=OSQP_DELTA,
           refine_iters=OSQP_POLISH_REFINE, wide=False, stream=None, work=None):
    """The forward derivative of a solve: how ``x*, y*`` move along ``(dq (B, no), dh (B, nc), dP (B, no, no)
    symmetric, dG (B, nc, no))`` (None: no change), a :class:`QpJvp` ``(dx, dy, verdict)``, so that
    ``x*(q + dq, ...) ~ x* + dx`` while the active set stays.  The right-hand side ``rx = -(dq + dP x + dG_A'y_A)``,
    ``ry = dh - dG x`` is formed with torch ops (the active mask is ``(h - z) < y``) on the stream of the solve --
    ``stream`` where one is passed, else torch's current one -- and the solve is one :func:`qp_sensitivity` call (``wide``: :func:`qp_sensitivity_wide`)."""
    torch = require_device()
    x, y, z, _ = _iterates(sol_or_xyz)
    # (the torch ops run on the stream the solve is launched on: `stream` where one is passed)
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        rx, ry = -dq, dh.clone()
        if dP is not None:
            rx = rx - torch.bmm(dP, x.unsqueeze(2)).squeeze(2)
        if dG is not None:
            ya = torch.where((h - z) < y, y, torch.zeros_like(y))
            rx = rx - torch.bmm(dG.transpose(1, 2), ya.unsqueeze(2)).squeeze(2)
            ry = ry - torch.bmm(dG, x.unsqueeze(2)).squeeze(2)
        rx, ry = rx.contiguous(), ry.contiguous()
    call = qp_sensitivity_wide if wide else qp_sensitivity
    kw = dict(work=work) if wide else {}
    s = call(P, G, h, (x, y, z), rx, ry, status=status, delta=delta,
             refine_iters=refine_iters, stream=stream, **kw)
    return QpJvp(s.u, s.w, s.verdict)


def _solve_qp(entry, P, q, G, h, x, y, z, rho, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, max_iter, check_every,
              adaptive_rho_interval, sigma, alpha, kinv, kinv_valid, stream, out, workspace=False, warm_out=False,
              soft=None, polish=None):
    """:func:`solve_qp` and :func:`solve_qp_wide` through the C entry ``entry``; ``workspace``: allocate
    ``kinv`` when it is None (the wide path's K^-1 off chip); ``warm_out``: ``out``'s iterates hold the start;
    ``soft``: the penalties, through ``entry`` + ``_soft``; ``polish``: the polish to run after the solve."""
    if polish is not None and soft is not None:
        raise ValueError("polish= with soft=: the polish's active-set model is the hard problem's")
    if warm_out and out is None:
        raise ValueError("warm=True is for out=: pass x, y, z for a warm start into new tensors")
    torch = require_device()
    if out is not None:
        if x is not None or y is not None or z is not None:
            raise ValueError("out is for a cold start: pass x, y, z for a warm one")
        x, y, z, status, iters, res = out
        batch = P.shape[0]
        for t, dtype, shape in ((status, torch.int32, (batch,)), (iters, torch.int32, (batch,)),
                                (res, torch.float64, (batch, 2))):
            _tensor(torch, t, dtype, shape, P.device,
                    "out: status, iters (B,) int32 and res (B, 2) float64, contiguous, on P's device")
    batch, no, nc, warm, x, y, z = _qp_operands(torch, P, q, G, h, x, y, z, kinv, kinv_valid)
    warm = warm and (out is None or bool(warm_out))
    if isinstance(rho, torch.Tensor):
        _tensor(torch, rho, torch.float64, (batch,), P.device,
                "rho: a float or a contiguous float64 (B,) tensor on P's device")
    else:
        rho = torch.full((batch,), float(rho), dtype=torch.float64, device=P.device)
    if out is None:
        status = torch.empty((batch,), dtype=torch.int32, device=P.device)
        iters = torch.empty((batch,), dtype=torch.int32, device=P.device)
        res = torch.empty((batch, 2), dtype=torch.float64, device=P.device)
    if workspace and kinv is None:
        lds, on = ctypes.c_int64(), ctypes.c_int32()
        info = capi.load().mpcasm_qp_solve_wide_info if soft is None else capi.load().mpcasm_qp_solve_wide_soft_info
        if info(no, nc, ctypes.byref(lds), ctypes.byref(on)) == 0 and not on.value:
            kinv = torch.empty((batch, no, no), dtype=torch.float64, device=P.device)
    extra = ()
    if soft is not None:
        lin, quad, stride = _soft_operands(torch, soft, batch, nc, P.device)
        entry, extra = entry + "_soft", (lin.data_ptr(), quad.data_ptr(), stride)
    with torch.cuda.device(P.device):
        rc = getattr(capi.load(), entry)(no, nc, P.data_ptr(), q.data_ptr(), G.data_ptr(), h.data_ptr(),
                                         x.data_ptr(), y.data_ptr(), z.data_ptr(), 1 if warm else 0,
                                         rho.data_ptr(), float(sigma), float(alpha), float(eps_abs),
                                         float(eps_rel), float(eps_prim_inf), float(eps_dual_inf), int(max_iter),
                                         int(check_every), int(adaptive_rho_interval), status.data_ptr(),
                                         iters.data_ptr(), res.data_ptr(), batch,
                                         kinv.data_ptr() if kinv is not None else None, 1 if kinv_valid else 0,
                                         _stream_handle(torch, stream), *extra)
    capi.check(rc, entry)
    sol = QpSolution(x, y, z, status, iters, res, rho)
    if polish is None:
        return sol
    return PolishedQpSolution(*sol, polish(P, q, G, h, sol, status=sol.status, stream=stream)[3])


def _soft_operands(torch, soft, batch, nc, device):
    """``soft=(lin, quad)`` as the C entries take it: two contiguous float64 tensors on ``device`` and their stride,
    0 for one pair of rows ``(nc,)`` (scalars are spread over the rows), ``nc`` for ``(B, nc)``.  A tensor that is
    already there is passed as it is (a loop that replays a graph keeps it at a fixed address)."""
    try:
        lin, quad = soft
    except (TypeError, ValueError):
        raise ValueError("soft: a pair (lin, quad)") from None
    out = []
    for v in (lin, quad):
        if not isinstance(v, torch.Tensor):
            v = torch.as_tensor(np.asarray(v, dtype=np.float64))
        if v.dim() == 0:
            v = v.expand(nc)
        out.append(v.to(device=device, dtype=torch.float64).contiguous())
    lin, quad = out
    if lin.shape != quad.shape or tuple(lin.shape) not in ((nc,), (batch, nc)):
        raise ValueError("soft: lin and quad scalars, (nc,) or (B, nc), both alike")
    return lin, quad, (0 if lin.dim() == 1 else nc)


def soft_pair(soft, nc, device):
    """``soft=(lin, quad)`` of a loop, once: two ``(nc,)`` float64 tensors on ``device`` that every tick passes at
    stride 0 (scalars spread over the rows).  ``ValueError`` for anything but scalars or ``(nc,)`` vectors."""
    torch = require_device()
    lin, quad, stride = _soft_operands(torch, soft, 1, nc, device)
    if stride != 0:
        raise ValueError("soft: a loop takes scalars or (nc,) vectors, one pair of rows for all instances")
    return lin, quad


def qp_solve_soft_lds_bytes(no, nc):
    """:func:`qp_solve_lds_bytes` for ``solve_qp(soft=...)`` (``mpcasm_qp_solve_soft_lds_bytes``)."""
    return _query("mpcasm_qp_solve_soft_lds_bytes", (no, nc), ctypes.c_int64)[0]


def qp_solve_wide_soft_info(no, nc):
    """:func:`qp_solve_wide_info` for ``solve_qp_wide(soft=...)`` (``mpcasm_qp_solve_wide_soft_info``)."""
    lds, on = _query("mpcasm_qp_solve_wide_soft_info", (no, nc), ctypes.c_int64, ctypes.c_int32)
    return lds, bool(on)


def qp_solve_lds_bytes(no, nc):
    """LDS bytes one instance of :func:`solve_qp` (and of :func:`admm`) takes; ``MpcasmError`` with
    ``ERR_LIMIT`` when that is more than a workgroup may have (``mpcasm_qp_solve_lds_bytes``)."""
    return _query("mpcasm_qp_solve_lds_bytes", (no, nc), ctypes.c_int64)[0]


def solve_qp_wide(P, q, G, h, x=None, y=None, z=None, rho=OSQP_RHO, eps_abs=1e-3, eps_rel=1e-3, eps_prim_inf=1e-4,
                  eps_dual_inf=1e-4, max_iter=4000, check_every=25, adaptive_rho_interval=100, sigma=OSQP_SIGMA,
                  alpha=OSQP_ALPHA, kinv=None, kinv_valid=False, stream=None, out=None, polish=False, warm=False,
                  soft=None):
    """:func:`solve_qp` for QPs whose matrices do not fit on chip (``mpcasm_qp_solve_wide``): the same
    arguments, rules and :class:`QpSolution`, up to 512 unknowns and 2 048 limits (:func:`qp_solve_wide_info`).
    ``G`` is read in place once per iteration; ``K^-1`` lives in LDS where it fits, else in ``kinv`` -- a
    ``(B, no, no)`` workspace allocated here when the caller passes none (the environment variable
    ``MPCASM_QP_WIDE_KINV`` = ``lds`` / ``global`` overrides where it lives).
    ``polish``: :func:`polish_qp_wide` with OSQP's defaults after the solve, on the solved instances, as
    :func:`solve_qp` does with :func:`polish_qp`: a :class:`PolishedQpSolution`.
    ``soft``: as for :func:`solve_qp`, through ``mpcasm_qp_solve_wide_soft``."""
    return _solve_qp("mpcasm_qp_solve_wide", P, q, G, h, x, y, z, rho, eps_abs, eps_rel, eps_prim_inf,
                     eps_dual_inf, max_iter, check_every, adaptive_rho_interval, sigma, alpha, kinv, kinv_valid,
                     stream, out, workspace=True, warm_out=warm, soft=soft, polish=polish_qp_wide if polish else None)


def qp_solve_wide_info(no, nc):
    """``(lds_bytes, kinv_on_chip)`` of one instance of :func:`solve_qp_wide`; ``MpcasmError`` with ``ERR_LIMIT``
    past its size limit (``mpcasm_qp_solve_wide_info``)."""
    lds, on = _query("mpcasm_qp_solve_wide_info", (no, nc), ctypes.c_int64, ctypes.c_int32)
    return lds, bool(on)


# --------------------------------------------------------------------------
# the loops' warm start: the store after a solve, the shifted start before the next
# --------------------------------------------------------------------------
WARM_SOLVED = capi.qp_bit(QP_SOLVED)      # warm_mask: only a solved record starts the next tick warm


class WarmStore:
    """The warm store of a closed loop (``mpcasm_qp_warm_store`` / ``mpcasm_qp_warm_start``): one record per row
    (per walker, in walker order) on ``device`` -- ``x (rows, no_max)`` and ``y (rows, nc_max)`` float64, padded
    with zeros, ``rho (rows,)`` float64 and ``meta (rows, 2)`` int32, the solve's status and a tag of the
    caller's choice.  The tags start at -1, the statuses at 0 (no ``QP_*`` value) and rho at 0: nothing is warm
    before its first store."""

    def __init__(self, rows, no_max, nc_max, device=None):
        torch = require_device()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        rows, no_max, nc_max = int(rows), int(no_max), int(nc_max)
        if rows < 0 or not 1 <= no_max <= 512 or not 0 <= nc_max <= 2048:
            raise ValueError("WarmStore: rows >= 0, 1 <= no_max <= 512, 0 <= nc_max <= 2048")
        self.rows, self.no, self.nc = rows, no_max, nc_max
        self.x = torch.zeros((rows, no_max), dtype=torch.float64, device=device)
        self.device = device = self.x.device
        self.y = torch.zeros((rows, nc_max), dtype=torch.float64, device=device)
        self.rho = torch.zeros((rows,), dtype=torch.float64, device=device)
        self.meta = torch.zeros((rows, 2), dtype=torch.int32, device=device)
        self.reset()

    def reset(self):
        """Forget every record (a loop that starts over): tags -1, statuses 0, rho 0; asynchronous."""
        self.meta.zero_()
        self.meta[:, 1] = -1
        self.rho.zero_()

    def _args(self):
        return (self.x.data_ptr(), self.y.data_ptr() if self.nc else None, self.rho.data_ptr(),
                self.meta.data_ptr(), self.rows, self.no, self.nc)


def _warm_tensor(torch, t, dtype, shape, device, what):
    return _tensor(torch, t, dtype, shape, device, "%s: a contiguous %s tensor of shape %s on the store's device"
                   % (what, str(dtype).replace("torch.", ""), tuple(shape)))


def _warm_index(torch, store, index, count):
    """A device index as it is (int32, ``count`` entries: the caller vouches for it, as for ``next_given``), one
    from the host checked and copied."""
    if index is None:
        if store.rows < count:
            raise ValueError("a store of %d rows takes no launch of %d instances without an index"
                             % (store.rows, count))
        return None
    if not isinstance(index, torch.Tensor):
        index = torch.as_tensor(checked_index(index, store.rows), device=store.device)
    return _warm_tensor(torch, index, torch.int32, (count,), store.device, "index")


def warm_store_qp(store, sol, tag, index=None, stream=None):
    """After a solve: instance ``b`` of ``sol`` (a :class:`QpSolution`, or ``(x, y, rho, status)``) into row
    ``index[b]`` of ``store`` (None: row ``b``) with ``tag``, whatever its status (``mpcasm_qp_warm_store``).
    ``index``: an int32 device tensor of distinct rows in range, or a host array (checked here)."""
    torch = require_device()
    x, y, rho, status = (sol.x, sol.y, sol.rho, sol.status) if hasattr(sol, "status") else sol
    count, no = x.shape
    nc = y.shape[1]
    dev = store.device
    _warm_tensor(torch, x, torch.float64, (count, no), dev, "x")
    _warm_tensor(torch, y, torch.float64, (count, nc), dev, "y")
    _warm_tensor(torch, rho, torch.float64, (count,), dev, "rho")
    _warm_tensor(torch, status, torch.int32, (count,), dev, "status")
    index = _warm_index(torch, store, index, count)
    with torch.cuda.device(dev):
        rc = capi.load().mpcasm_qp_warm_store(no, nc, x.data_ptr(), y.data_ptr() if nc else None, rho.data_ptr(),
                                              status.data_ptr(), int(tag), *store._args(),
                                              index.data_ptr() if index is not None else None, count,
                                              _stream_handle(torch, stream))
    capi.check(rc, "mpcasm_qp_warm_store")


WarmStart = collections.namedtuple("WarmStart", "x y z rho warm")


def warm_start_qp(store, G, h, col_src, row_src, expect_tag, index=None, warm_mask=WARM_SOLVED, rho_cold=OSQP_RHO,
                  stream=None, out=None):
    """Before a solve: the iterates and the step it starts from (``mpcasm_qp_warm_start``), for the assembled
    ``G (B, nc, no)``, ``h (B, nc)``.  Instance ``b`` is warm when the record in row ``index[b]`` of ``store``
    (None: row ``b``) carries ``expect_tag`` and a status in ``warm_mask``, a rho inside [1e-6, 1e6] and finite
    values wherever the tables read it: then ``x0``, ``y0`` are the record's, gathered through ``col_src (no,)``
    and ``row_src (nc,)`` (int32 device tensors, :func:`mpcasm.warm.shift_map`; -1: zero), ``z0 = min(G x0, h)``
    and ``rho0`` the record's.  Otherwise the start is the cold one: ``0, 0, min(0, h)``, ``rho_cold``.
    Returns a :class:`WarmStart` ``(x, y, z, rho, warm)``, ``warm (B,)`` int32 -- pass ``x, y, z, rho`` to
    :func:`solve_qp`.  ``out``: the caller's ``(x, y, z, rho, warm)`` to write instead of new tensors."""
    torch = require_device()
    dev = store.device
    if not (isinstance(G, torch.Tensor) and G.dim() == 3):
        raise ValueError("G: a (B, nc, no) device tensor")
    count, nc, no = G.shape
    _warm_tensor(torch, G, torch.float64, (count, nc, no), dev, "G")
    _warm_tensor(torch, h, torch.float64, (count, nc), dev, "h")
    _warm_tensor(torch, col_src, torch.int32, (no,), dev, "col_src")
    _warm_tensor(torch, row_src, torch.int32, (nc,), dev, "row_src")
    if out is None:
        f = dict(dtype=torch.float64, device=dev)
        out = (torch.empty((count, no), **f), torch.empty((count, nc), **f), torch.empty((count, nc), **f),
               torch.empty((count,), **f), torch.empty((count,), dtype=torch.int32, device=dev))
    x, y, z, rho, warm = out
    _warm_tensor(torch, x, torch.float64, (count, no), dev, "x")
    _warm_tensor(torch, y, torch.float64, (count, nc), dev, "y")
    _warm_tensor(torch, z, torch.float64, (count, nc), dev, "z")
    _warm_tensor(torch, rho, torch.float64, (count,), dev, "rho")
    _warm_tensor(torch, warm, torch.int32, (count,), dev, "warm")
    index = _warm_index(torch, store, index, count) if index is not None else None
    nul = lambda t: t.data_ptr() if nc else None
    with torch.cuda.device(dev):
        rc = capi.load().mpcasm_qp_warm_start(no, nc, nul(G), nul(h), *store._args(),
                                              index.data_ptr() if index is not None else None,
                                              col_src.data_ptr(), nul(row_src), int(expect_tag), int(warm_mask),
                                              float(rho_cold), x.data_ptr(), nul(y), nul(z), rho.data_ptr(),
                                              warm.data_ptr(), count, _stream_handle(torch, stream))
    capi.check(rc, "mpcasm_qp_warm_start")
    return WarmStart(x, y, z, rho, warm)


# every outcome but NON_CVX (whose iterates are NaN) / the solved ones and those out of iterations: the
# apply_mask of Assembler.next_given under WalkerFleet's "apply" / "hold" rule
APPLY_ALL = sum(capi.qp_bit(s) for s in (QP_SOLVED, QP_MAX_ITER, QP_PRIMAL_INFEASIBLE, QP_DUAL_INFEASIBLE))
APPLY_SOLVED = capi.qp_bit(QP_SOLVED) | capi.qp_bit(QP_MAX_ITER)


def given_map_records(plan, rules):
    """The records of a given map (``mpcasm_given_map_compile``) for ``plan``: ``(rows, values)``, one entry
    per column of ``given`` -- a row of the plan's preview program (``plan.pm_rows``), ``capi.GIVEN_CONST``
    with the value in ``values``, or ``capi.GIVEN_KEEP``.  ``rules``: given variable (a key of
    ``form.given_ID``) -> a list with one ``(definition, sample)`` pair per component of the variable (None:
    that component is kept), or a float: every component becomes that constant.  Variables not named are
    kept.  Host only: no device needed."""
    rows = np.full(plan.ng, capi.GIVEN_KEEP, dtype=np.int32)
    values = np.zeros(plan.ng, dtype=np.float64)
    for var, rule in rules.items():
        if var not in plan.given_ID:
            raise KeyError("%r is not a given variable of this plan (%s)" % (var, ", ".join(plan.given_ID)))
        cols = plan.given_ID[var]
        if isinstance(rule, (int, float, np.floating, np.integer)):
            if not np.isfinite(rule):
                raise ValueError("%r: a constant must be finite" % var)
            rows[cols.start:cols.stop] = capi.GIVEN_CONST
            values[cols.start:cols.stop] = float(rule)
            continue
        rule = list(rule)
        if len(rule) != len(cols):
            raise ValueError("%r has %d components, the rule names %d" % (var, len(cols), len(rule)))
        for c, pair in zip(cols, rule):
            if pair is None:
                continue
            definition, sample = pair
            if definition not in plan.pm_rows:
                raise KeyError("%r is not a definition of this plan" % (definition,))
            r0, n = plan.pm_rows[definition]
            if not 0 <= int(sample) < n:
                raise ValueError("%r has %d samples, the rule asks for sample %d" % (definition, n, sample))
            rows[c] = r0 + int(sample)
    return rows, values


GivenMap = collections.namedtuple("GivenMap", "table words rows values plan")


def param_map_records(plan, rules, columns):
    """The records of a parameter map (``mpcasm_params_map``) for ``plan``: ``(recs, coef)``, int32 ``(nrecs, 4)``
    ``(dst, col, flags, 0)`` and float64 ``(nrecs, 2)`` ``(c0, c1)`` -- record ``r`` makes element ``dst`` of every
    instance's parameter row ``[c0 +] (c1 [* sign]) * command[col]``.  ``columns``: the names of the command
    columns, in order.  ``rules``: a key of ``plan.param_slots`` (``(kind, name, field)``, e.g.
    ``("cost", "track vel_x", "aim")`` or ``("limit", 3, "center")``) -> one entry per element of the slot, as a
    ``(rows, cols)`` nest or flat in row-major order: ``None`` (the element is kept), a column name, or a dict
    ``{"column": name, "c1": 1.0, "signed": False, "c0": None}`` (``c0`` None: no constant is added).
    ``KeyError``: a slot or a column that is not there; ``ValueError``: a wrong number of entries, a coefficient
    that is not finite, two entries that reach one element.  Host only: no device needed."""
    columns = list(columns)
    if len(set(columns)) != len(columns):
        raise ValueError("columns: the names must differ")
    recs, coef, seen = [], [], set()
    for key, rule in rules.items():
        if key not in plan.param_slots:
            raise KeyError("%r is not a parameter slot of this plan" % (key,))
        start, rows, cols = plan.param_slots[key]
        rule = list(rule) if isinstance(rule, (list, tuple)) else [rule]
        nested = [isinstance(entry, (list, tuple)) for entry in rule]
        if any(nested):      # (a nest is rows of cols entries, a flat list the same in row-major order)
            if not all(nested) or len(rule) != rows or any(len(entry) != cols for entry in rule):
                raise ValueError("%r has %d x %d elements, the rule is not shaped so" % (key, rows, cols))
            flat = [entry for row in rule for entry in row]
        else:
            flat = rule
        if len(flat) != rows * cols:
            raise ValueError("%r has %d x %d elements, the rule names %d" % (key, rows, cols, len(flat)))
        for e, entry in enumerate(flat):
            if entry is None:
                continue
            if not isinstance(entry, dict):
                entry = {"column": entry}
            unknown = set(entry) - {"column", "c1", "signed", "c0"}
            if unknown or "column" not in entry:
                raise ValueError("%r: an entry is None, a column or a dict with 'column' and optionally 'c1', "
                                 "'signed', 'c0'; got %r" % (key, entry))
            if entry["column"] not in columns:
                raise KeyError("%r is not a command column (%s)" % (entry["column"], ", ".join(map(str, columns))))
            c0, c1 = entry.get("c0"), float(entry.get("c1", 1.0))
            if not np.isfinite(c1) or (c0 is not None and not np.isfinite(c0)):
                raise ValueError("%r: the coefficients must be finite" % (key,))
            dst = start + e
            if dst in seen:
                raise ValueError("%r: element %d of the parameters is reached twice" % (key, dst))
            seen.add(dst)
            flags = (capi.PMAP_SIGNED if entry.get("signed", False) else 0) | (capi.PMAP_CONST if c0 is not None else 0)
            recs.append((dst, columns.index(entry["column"]), flags, 0))
            coef.append((0.0 if c0 is None else float(c0), c1))
    return (np.asarray(recs, dtype=np.int32).reshape(-1, 4), np.asarray(coef, dtype=np.float64).reshape(-1, 2))


ParamMap = collections.namedtuple("ParamMap", "recs coef nrecs ncmd signed columns plan host_recs host_coef")


def check_param_map_sign(recs, sign):
    """``ValueError`` when the records ``recs`` of a parameter map hold a signed one and ``sign`` is None: the
    launch would leave those elements unwritten (mpcasm.h), which no caller means.  Host only."""
    recs = np.asarray(recs).reshape(-1, 4)
    if sign is None and recs.size and (recs[:, 2] & capi.PMAP_SIGNED).any():
        raise ValueError("sign: this map has a signed record, it needs a sign per instance")


def checked_index(idx, rows):
    """``idx`` as the int32 index of a launch that writes (or reads) rows of a ``rows``-row buffer by it:
    ValueError unless its entries are distinct and in ``[0, rows)`` (mpcasm.h: the kernels do not check)."""
    idx = np.asarray(idx)
    if idx.size and (idx.min() < 0 or idx.max() >= rows or np.unique(idx).size != idx.size):
        raise ValueError("an index of rows must hold distinct entries in [0, %d)" % rows)
    return idx.astype(np.int32)


# --------------------------------------------------------------------------
# K2 + K3 + K4
# --------------------------------------------------------------------------
HALF_CU_LDS = 80 * 1024      # two workgroups of the persistent kernel share a CU's 160 KB


def _table_args(plan):
    """The four leading arguments of every entry that takes a plan's tables.  The arrays' ``.ctypes`` objects pass
    as their addresses and keep the arrays alive as long as the tuple lives: hold it across the call."""
    itab, dtab = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab)
    return itab.ctypes, itab.size, dtab.ctypes if dtab.size else None, dtab.size


def _stride_arg(plan, src_stride):
    """``h_src_stride`` of a host-only query: one entry per source of ``plan`` (None: every source shared)."""
    n = len(plan.sources)
    return (ctypes.c_int64 * max(n, 1))(*([0] * n if src_stride is None else [int(x) for x in src_stride]))


def resident_lds_bytes(plan):
    """LDS bytes a workgroup of the persistent kernel needs for ``plan`` -- with ``P`` handed over
    directly, with ``P`` collected in LDS (``mpcasm_resident_lds_bytes``; 0: not on that kernel)."""
    out = (ctypes.c_int64 * 2)()
    capi.check(capi.load().mpcasm_resident_lds_bytes(*_table_args(plan), out), "mpcasm_resident_lds_bytes")
    return int(out[0]), int(out[1])


def preview_route(plan, src_stride=None, nterms=0, ngoals=0):
    """The kernel ``mpcasm_preview_direct`` (``ngoals == 0``) or ``mpcasm_preview_goal_distance`` (a goal
    table of ``nterms`` records for ``ngoals`` goals) launches for ``plan`` when its sources have the strides
    ``src_stride`` (default: every source shared by the batch) -- ``mpcasm_preview_route``, no device needed:
    ``(route, E1, R1, E2, R2, DIST, LDS bytes, whole LDS)`` with ``route`` one of ``capi.PREVIEW_*``, or
    ``None`` where the launch returns ``MPCASM_ERR_LIMIT``."""
    out = (ctypes.c_int32 * 8)()
    rc = capi.load().mpcasm_preview_route(*_table_args(plan), _stride_arg(plan, src_stride), int(nterms),
                                          int(ngoals), out)
    if rc == capi.ERR_LIMIT:
        return None
    capi.check(rc, "mpcasm_preview_route")
    return tuple(int(x) for x in out)


AdjointInfo = collections.namedtuple("AdjointInfo", "lds whole_lds index_words per_cu")


def adjoint_info(plan, src_stride=None):
    """What ``mpcasm_assemble_jvp`` / ``mpcasm_assemble_vjp`` launch for ``plan`` when its sources have the strides
    ``src_stride`` (default: every source shared) -- ``mpcasm_assemble_adjoint_info``, the launches' own decision,
    no device needed: an :class:`AdjointInfo` ``(LDS bytes of a workgroup, whole LDS, words of the transposed index,
    resident workgroups per CU)``.  Raises :class:`capi.MpcasmError` with ``MPCASM_ERR_LIMIT`` where the launches
    refuse the plan (compiled with ``ltv=``, or one instance beyond a CU's LDS)."""
    out = (ctypes.c_int32 * 4)()
    capi.check(capi.load().mpcasm_assemble_adjoint_info(*_table_args(plan), _stride_arg(plan, src_stride), out),
               "mpcasm_assemble_adjoint_info")
    return AdjointInfo(*(int(x) for x in out))


def params_adjoint_info(plan, src_stride=None):
    """:func:`adjoint_info` for ``mpcasm_assemble_params_vjp`` (``mpcasm_assemble_params_vjp_info``): an
    :class:`AdjointInfo` whose ``index_words`` are the words of the parameter index.  Raises
    :class:`capi.MpcasmError` with ``MPCASM_ERR_LIMIT`` where the launch refuses the plan."""
    out = (ctypes.c_int32 * 4)()
    capi.check(capi.load().mpcasm_assemble_params_vjp_info(*_table_args(plan), _stride_arg(plan, src_stride), out),
               "mpcasm_assemble_params_vjp_info")
    return AdjointInfo(*(int(x) for x in out))


def sweep_route(plan):
    """What ``mpcasm_assemble`` launches for a plan with a dynamics compiled as ``ltv`` -- ``mpcasm_sweep_route``,
    the launch's own decision, no device needed: ``(CPT, specialised, PAIR, per_line, reg_lines, LR, LDS bytes,
    whole LDS)`` of ``ltv_sweep_kernel<CPT, NS, MS, AS, PAIR>`` (``specialised``: ``NS, MS, AS = 3, 1, 2``).
    Raises :class:`capi.MpcasmError` with ``MPCASM_ERR_LIMIT`` where the launch refuses the plan, with
    ``MPCASM_ERR_ARG`` for a plan that does not run on the sweep kernel."""
    out = (ctypes.c_int32 * 8)()
    capi.check(capi.load().mpcasm_sweep_route(*_table_args(plan), out), "mpcasm_sweep_route")
    return tuple(int(x) for x in out)


TiledRoute = collections.namedtuple(
    "TiledRoute", "form fused kp cb rows_in_lds whole_lines lds whole_lds tables tg sym")


def tiled_route(plan, batch, src_stride=None, want=capi.WANT_COST | capi.WANT_CONSTRAINTS, path=0):
    """What ``mpcasm_assemble`` launches for a plan on the tiled path (csrc/tiled.hip) -- ``mpcasm_tiled_route``,
    the launch's own decision, no device needed -- for ``batch`` instances whose sources have the strides
    ``src_stride`` (default: every source shared by the batch; the slots of a dynamics compiled with ``lti=``
    carry its ``(A, B)``), the halves ``want`` (``capi.WANT_COST | capi.WANT_CONSTRAINTS``) and
    ``MPCASM_OPT_PATH`` ``path`` (``-1``: the process-wide value).  A :class:`TiledRoute`: ``form`` one of
    ``capi.TILED_*``; for the scan form ``fused``, the instantiation ``toeplitz_scan_kernel<kp, cb>``,
    ``rows_in_lds`` and ``whole_lines``; ``lds`` bytes of the scan or Toeplitz kernel and ``whole_lds`` (more than
    64 KB); ``tables`` one of ``capi.TILED_TABLES_*``; ``tg`` of ``shared_p_kernel<tg>``; ``sym``.  Raises
    :class:`capi.MpcasmError` with ``MPCASM_ERR_LIMIT`` where the launch refuses the plan, with ``MPCASM_ERR_ARG``
    for a plan that does not run on the tiled path."""
    out = (ctypes.c_int32 * 16)()
    capi.check(capi.load().mpcasm_tiled_route(*_table_args(plan), _stride_arg(plan, src_stride), int(batch),
                                              int(want), int(path), out), "mpcasm_tiled_route")
    return TiledRoute(*(int(x) for x in out[:11]))


AssembleRoute = collections.namedtuple("AssembleRoute", "kernel lds p_direct")


def assemble_route(plan, batch, path=0, aligned=True, indexed=False):
    """Which kernel family ``mpcasm_assemble`` (``indexed``: ``mpcasm_assemble_indexed``) runs ``batch`` instances
    of ``plan`` on under ``MPCASM_OPT_PATH`` ``path`` (``-1``: the process-wide value), with the launch's inputs
    aligned for the persistent kernel's 16-byte loads or not -- ``mpcasm_assemble_route``, the launch's own
    decision, no device needed.  An :class:`AssembleRoute`: ``kernel`` one of ``capi.KERNEL_*`` (the persistent
    kernel always as ``capi.KERNEL_RESIDENT``, the tiled path as ``capi.KERNEL_TILED``), the dynamic LDS bytes of
    the persistent or fused kernel, and whether the persistent kernel hands ``P`` over directly at this batch.
    Raises :class:`capi.MpcasmError` with ``MPCASM_ERR_LIMIT`` where the launch refuses."""
    out = (ctypes.c_int32 * 4)()
    capi.check(capi.load().mpcasm_assemble_route(*_table_args(plan), int(batch), int(path), int(aligned),
                                                 int(indexed), out), "mpcasm_assemble_route")
    return AssembleRoute(*(int(x) for x in out[:3]))


StagedRoute = collections.namedtuple(
    "StagedRoute", "hessian sym nb npairs nbr nbc whole_lines max_axes grid_k2 grid_k3 grid_gradient grid_k4")


def staged_route(plan, batch, want_cost=True, want_constraints=True):
    """What the staged pipeline (csrc/assemble.hip; ``MPCASM_OPT_PATH`` 2, and every plan no other kernel takes)
    launches for ``batch`` instances of ``plan`` with these halves wanted -- ``mpcasm_staged_route``, the launch's
    own decision, no device needed.  A :class:`StagedRoute`: ``hessian`` one of ``capi.STAGED_*``; ``sym``, ``nb``,
    ``npairs`` of ``hessian_gemm_kernel`` (128 unknowns or more), or the block rows and columns ``nbr``, ``nbc`` of
    ``hessian_kernel``; ``whole_lines`` of ``constraints_kernel``; the most axes of a limit; the workgroups of the
    four launches (0: not launched).  Raises :class:`capi.MpcasmError` with ``MPCASM_ERR_LIMIT`` where the launch
    refuses (a limit of more than 8 axes with the constraints wanted), with ``MPCASM_ERR_ARG`` for a plan the
    pipeline cannot run (``ltv=``, ``lti=``, ``csc=``)."""
    out = (ctypes.c_int32 * 8)()
    capi.check(capi.load().mpcasm_staged_route(*_table_args(plan), int(bool(want_cost)), int(bool(want_constraints)),
                                               int(batch), out), "mpcasm_staged_route")
    form, flags, a, b, k2, k3, grad, k4 = (int(x) for x in out)
    gemm = form == capi.STAGED_GEMM
    return StagedRoute(form, flags & capi.STAGED_SYM, a if gemm else 0, b if gemm else 0, 0 if gemm else a,
                       0 if gemm else b, (flags & capi.STAGED_WHOLE_LINES) >> 1, flags >> 8, k2, k3, grad, k4)


def rollout_table(plan, records=None, cvec=None, sizes=None):
    """The words of the row table ``mpcasm_ltv_rollout`` and ``mpcasm_ltv_advance`` read for ``plan`` (compiled
    with ``ltv=``), an int32 array -- ``mpcasm_ltv_rollout_compile``, host only, no device needed.  ``records``,
    ``cvec``: :func:`mpcasm.plan.rollout_rows`'s (the default; ``ValueError`` there for a definition that is none
    of its three kinds); ``sizes``: what they were made for (default: the plan's).  :class:`capi.MpcasmError` with
    ``MPCASM_ERR_ARG`` for a plan without a dynamics compiled as ``ltv``, sizes that are not the plan's or
    records that do not fit it."""
    if records is None:
        records, cvec = rollout_rows(plan)
    records = np.ascontiguousarray(records, dtype=np.int32).reshape(-1, capi.ROLL_REC_WORDS)
    cvec = np.ascontiguousarray(cvec, dtype=np.float64).reshape(-1, 4)
    if sizes is None:
        sw = plan.sweep or {}
        sizes = rollout_sizes(plan) if sw else np.zeros(7, dtype=np.int32)
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    lib, words = capi.load(), ctypes.c_int64()
    args = _table_args(plan) + (sizes.ctypes.data, records.ctypes.data, records.shape[0],
                                cvec.ctypes.data if cvec.size else None, cvec.shape[0])
    capi.check(lib.mpcasm_ltv_rollout_compile(*args, None, 0, ctypes.byref(words)), "mpcasm_ltv_rollout_compile")
    host = np.zeros(words.value, dtype=np.int32)
    capi.check(lib.mpcasm_ltv_rollout_compile(*args, host.ctypes.data, host.size, ctypes.byref(words)),
               "mpcasm_ltv_rollout_compile")
    return host


def rollout_info(plan, rows=True, count=1, table_words=None):
    """``(group, lds_bytes, workgroups)`` of the launch ``mpcasm_ltv_rollout`` (``rows``) or ``mpcasm_ltv_advance``
    (not ``rows``) makes for ``count`` instances of ``plan`` (compiled with ``ltv=``): the instances of a workgroup,
    its dynamic LDS bytes, the workgroups -- ``mpcasm_ltv_rollout_info``, host only, no device needed.
    ``table_words``: the words of the row table (default: :func:`rollout_table`'s).  :class:`capi.MpcasmError` with
    the launch's own ``MPCASM_ERR_ARG`` / ``MPCASM_ERR_LIMIT``."""
    if table_words is None:
        table_words = rollout_table(plan).size
    group, lds, groups = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
    capi.check(capi.load().mpcasm_ltv_rollout_info(
        *_table_args(plan), int(table_words), 1 if rows else 0, int(count), ctypes.byref(group), ctypes.byref(lds),
        ctypes.byref(groups)), "mpcasm_ltv_rollout_info")
    return group.value, lds.value, groups.value


# --------------------------------------------------------------------------
# pre-stabilised prediction (csrc/feedback.hip)
# --------------------------------------------------------------------------
def _ltv_sequences(torch, A_seq, B_seq):
    """``n, m, T, batch (None: both shared), device`` of a pair of sequences ``(T, n, n)`` / ``(B, T, n, n)`` and
    ``(T, n, m)`` / ``(B, T, n, m)``, checked as :meth:`Assembler.bind_ltv_window` checks them."""
    for what, seq in (("A_seq", A_seq), ("B_seq", B_seq)):
        if _tensor(torch, seq, torch.float64, None, None, None) is None or seq.dim() not in (3, 4):
            raise ValueError("%s: a contiguous float64 device tensor of 3 or 4 dimensions" % what)
    n, m, T = A_seq.shape[-1], B_seq.shape[-1], A_seq.shape[-3]
    if A_seq.shape[-2] != n or tuple(B_seq.shape[-3:-1]) != (T, n) or B_seq.device != A_seq.device:
        raise ValueError("A_seq (.., T, n, n) and B_seq (.., T, n, m) on one device, got %s and %s"
                         % (tuple(A_seq.shape), tuple(B_seq.shape)))
    batches = {seq.shape[0] for seq in (A_seq, B_seq) if seq.dim() == 4}
    if len(batches) > 1:
        raise ValueError("A_seq and B_seq of %d and %d instances" % (A_seq.shape[0], B_seq.shape[0]))
    if not (1 <= n <= 4 and 1 <= m <= 4):
        raise ValueError("1 <= n <= 4 states and 1 <= m <= 4 inputs (the sweep kernel's sizes), got n = %d, m = %d"
                         % (n, m))
    return n, m, T, (batches.pop() if batches else None), A_seq.device


def _seq_stride(seq):
    return int(np.prod(seq.shape[1:])) if seq.dim() == 4 else 0


def _ltv_gain(torch, K, n, m, T, batch, device):
    """``batch (None: everything shared), k_stride, k_step_stride`` of a gain ``(m, n)``, ``(B, m, n)`` or ``(B, T,
    m, n)`` beside sequences of ``batch`` instances (:func:`_ltv_sequences`)."""
    if not (_tensor(torch, K, torch.float64, None, device, None) is not None
            and K.dim() in (2, 3, 4) and tuple(K.shape[-2:]) == (m, n) and (K.dim() < 4 or K.shape[1] == T)
            and (K.dim() == 2 or batch in (None, K.shape[0]))):
        raise ValueError("K: a contiguous float64 tensor of shape (%d, %d), (B, %d, %d) or (B, %d, %d, %d) on %s, "
                         "got %s" % (m, n, m, n, T, m, n, device,
                                     tuple(K.shape) if torch.is_tensor(K) else type(K).__name__))
    if K.dim() > 2:
        batch = K.shape[0]
    return (batch,) + {2: (0, 0), 3: (m * n, 0), 4: (T * m * n, m * n)}[K.dim()]


def ltv_lqr(A_seq, B_seq, Q, R, terminal=None, want_closed=True, stream=None):
    """The gains that pre-stabilise per-step plants (``mpcasm_ltv_lqr``, csrc/feedback.hip): the backward Riccati
    sweep ``K_k = -(R + B_k^T P B_k)^-1 B_k^T P A_k``, ``P <- Q + A_k^T P (A_k + B_k K_k)`` from ``P = terminal``
    (default ``Q``) over every instance's own sequence.  ``A_seq (T, n, n)`` / ``(B, T, n, n)``, ``B_seq (T, n, m)``
    / ``(B, T, n, m)``: contiguous float64 device tensors; ``Q (n, n)``, ``R (m, m)``, ``terminal (n, n)``
    symmetric, shared by the batch (tensors or arrays).  Returns ``(K, A_cl, info)``: ``K (B, T, m, n)``,
    ``A_cl = A + B K (B, T, n, n)`` (``None`` unless ``want_closed``) -- without the leading ``B`` where both
    sequences are shared -- and ``info`` int32 ``(B,)``: -1, or the step whose pivot was not positive (its rows of
    ``K`` and ``A_cl`` and every earlier step's are NaN).  Nothing is read back."""
    torch = _torch()
    n, m, T, batch, device = _ltv_sequences(torch, A_seq, B_seq)
    lead = () if batch is None else (batch,)
    mats = []
    for what, mat, size in (("Q", Q, n), ("R", R, m), ("terminal", terminal, n)):
        if mat is not None:
            mat = _as_device(torch, mat, device)
            if tuple(mat.shape) != (size, size):
                raise ValueError("%s: (%d, %d), got %s" % (what, size, size, tuple(mat.shape)))
        mats.append(mat)
    f = dict(dtype=torch.float64, device=device)
    K = torch.empty(lead + (T, m, n), **f)
    Acl = torch.empty(lead + (T, n, n), **f) if want_closed else None
    info = torch.empty((batch or 1,), dtype=torch.int32, device=device)
    ptr = lambda t: t.data_ptr() if t is not None else None
    with torch.cuda.device(device):
        rc = capi.load().mpcasm_ltv_lqr(n, m, T, batch or 1, A_seq.data_ptr(), _seq_stride(A_seq), B_seq.data_ptr(),
                                        _seq_stride(B_seq), ptr(mats[0]), ptr(mats[1]), ptr(mats[2]), K.data_ptr(),
                                        ptr(Acl), info.data_ptr(), _stream_handle(torch, stream))
    capi.check(rc, "mpcasm_ltv_lqr")
    return K, Acl, info


def ltv_close(A_seq, B_seq, K, stream=None):
    """``A_cl = A + B K`` for gains the caller brings (``mpcasm_ltv_close``): ``K`` ``(m, n)`` -- one gain --,
    ``(B, m, n)`` -- one per instance -- or ``(B, T, m, n)`` -- one per instance and step --, a contiguous float64
    tensor on the sequences' device; ``A_seq``, ``B_seq`` as for :func:`ltv_lqr`.  Returns ``(B, T, n, n)``, or
    ``(T, n, n)`` where the sequences and the gain are shared."""
    torch = _torch()
    n, m, T, batch, device = _ltv_sequences(torch, A_seq, B_seq)
    batch, k_stride, k_step = _ltv_gain(torch, K, n, m, T, batch, device)
    Acl = torch.empty((() if batch is None else (batch,)) + (T, n, n), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        rc = capi.load().mpcasm_ltv_close(n, m, T, batch or 1, A_seq.data_ptr(), _seq_stride(A_seq), B_seq.data_ptr(),
                                          _seq_stride(B_seq), K.data_ptr(), k_stride, k_step, Acl.data_ptr(),
                                          _stream_handle(torch, stream))
    capi.check(rc, "mpcasm_ltv_close")
    return Acl


def ltv_augment(A_seq, B_seq, K, want_gain=True, stream=None):
    """The closed loop with the true input as a state (``mpcasm_ltv_augment``): ``z_k = [x_k ; u_{k-1}]`` with
    ``u_k = K_k x_k + v_k``, so ``At_k = [[A_k + B_k K_k, 0], [K_k, 0]]`` and ``Bt_k = [[B_k], [I]]`` -- a formulation
    on ``(At, Bt)`` whose input is ``v`` sees ``u`` as its last ``m`` states, and costs and limits on them are costs
    and limits on the true input.  ``A_seq``, ``B_seq`` and ``K`` exactly as for :func:`ltv_close`; ``n + m <= 4``.
    Returns ``(At_seq, Bt_seq, Kt_seq)``: ``(B, T, n + m, n + m)``, ``(B, T, n + m, m)`` and ``Kt = [K | 0]`` ``(B, T,
    m, n + m)``, the gains :meth:`Assembler.true_inputs` takes on the augmented plan (``None`` unless ``want_gain``)
    -- without the leading ``B`` where the sequences and the gain are shared.  The ``A + B K`` block is
    :func:`ltv_close`'s result bit for bit."""
    torch = _torch()
    n, m, T, batch, device = _ltv_sequences(torch, A_seq, B_seq)
    batch, k_stride, k_step = _ltv_gain(torch, K, n, m, T, batch, device)
    if n + m > 4:
        raise ValueError("n + m <= 4 states of the augmented plant (the sweep kernel's sizes), got n = %d, m = %d"
                         % (n, m))
    lead = () if batch is None else (batch,)
    f = dict(dtype=torch.float64, device=device)
    At, Bt = torch.empty(lead + (T, n + m, n + m), **f), torch.empty(lead + (T, n + m, m), **f)
    Kt = torch.empty(lead + (T, m, n + m), **f) if want_gain else None
    with torch.cuda.device(device):
        rc = capi.load().mpcasm_ltv_augment(n, m, T, batch or 1, A_seq.data_ptr(), _seq_stride(A_seq),
                                            B_seq.data_ptr(), _seq_stride(B_seq), K.data_ptr(), k_stride, k_step,
                                            At.data_ptr(), Bt.data_ptr(), Kt.data_ptr() if want_gain else None,
                                            _stream_handle(torch, stream))
    capi.check(rc, "mpcasm_ltv_augment")
    return At, Bt, Kt


STREAMING_LAUNCH_BYTES = 560e6    # results per launch from which P is collected in LDS (resident.hip)


def plan_for_device(form, workspace="auto", batch=None, **kw):
    """``compile_plan`` plus the one decision that needs the kernel's own LDS layout: with
    ``workspace="auto"`` a plan whose dense workspace leaves room for ONE workgroup per CU is compiled
    with the compact workspace when that fits two -- judged with ``P`` handed over directly, and, for
    an assembler whose capacity makes its launches streaming ones, first with ``P`` in LDS, which is
    how such launches run (same box, one process, `tools/ab_workspace.py`: the biped at N = 24 with
    S, U read from memory 0.076 -> 0.064 ms at 4 096 instances, 0.276 -> 0.264 at 16 384; with its
    matrices built on chip 0.230 -> 0.219 at 16 384, where the dense plan would be 7 % faster at 4 096)."""
    plan = compile_plan(form, workspace=workspace, **kw)
    if workspace != "auto" or plan.workspace.compact:
        return plan
    dense = resident_lds_bytes(plan)
    if max(dense) <= HALF_CU_LDS:
        return plan
    per_instance = 8 * (plan.no * plan.no + plan.no + plan.nc * plan.no + plan.nc)
    streaming = batch is not None and per_instance * batch >= STREAMING_LAUNCH_BYTES
    small, lds = None, None
    for in_lds in ((1, 0) if streaming else (0,)):
        if dense[in_lds] > HALF_CU_LDS:
            if small is None:
                small = compile_plan(form, workspace="compact", **kw)
                lds = resident_lds_bytes(small)
            if small.workspace.compact and 0 < lds[in_lds] <= HALF_CU_LDS:
                return small
    return plan


def _checked_out(torch, out, shape, device, what):
    """A caller's result buffer: float64, contiguous, on the assembler's device, at least ``shape``."""
    return _tensor(torch, out, torch.float64, shape, device, "%s: out must be a contiguous float64 tensor on %s of "
                   "shape (>= %d, %s)" % (what, device, shape[0], ", ".join(str(x) for x in shape[1:])), at_least=True)


class Assembler:
    """Batched assembly of one Formulation structure on one device.

    Per-instance numbers:
      * ``given``  ``(B, ng)``  -- argument of :meth:`assemble`;
      * parameters (weight / aim / cross_aim of every Cost, arrow / center /
        extreme of every Constraint) -- start as the Formulation's current
        values broadcast over the batch, override with :meth:`set_param`;
      * horizon matrices -- shared by default (the Formulation's own arrays),
        bind a ``(B, N, p, n)`` tensor with :meth:`bind_source` for per-instance
        dynamics (e.g. the output of :func:`fill_su`);
      * or, for the dynamics named in ``lti``, no horizon matrices at all: the kernel
        builds them on chip from the system's ``(A, B)`` (K1 fused into the assembly) --
        shared by default (recovered from the Formulation's ``S, U``), per instance with
        :meth:`bind_lti`.
    """

    def __init__(self, form, batch=1, device=None, costs=None, limits=None, lti=(), csc=None,
                 workspace="auto", ltv=()):
        torch = require_device()
        self._torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        self.batch = int(batch)
        # csc = "upper" / "full": :meth:`assemble` returns the CSC ``data`` arrays of P (its upper
        # triangle / all of it) and G instead of the dense matrices -- ``(B, nnz)`` each, on the
        # pattern of :meth:`csc_pattern` -- written by the assembly kernel itself
        # (biped_mpc_loop.py:57-58 without a second pass).  ValueError / RuntimeError when the
        # problem does not run on the persistent kernel: assemble dense and use export_csc.
        # workspace = "auto": the persistent kernel's workspace is kept compact (plan.py Workspace)
        # when it is big (the plan compiler's rule: C3) or when that is what lets a second
        # workgroup share the CU's LDS (plan_for_device: the biped at N = 24 with S, U read from
        # memory); "dense" / "compact" force one.
        # ltv = [name]: the dynamics ``name`` has its own (A_k, B_k) at every step, per instance
        # (:meth:`bind_ltv`; BASELINE config C5): the sweep kernel assembles without horizon matrices
        self.plan = plan_for_device(form, costs=costs, limits=limits, lti=tuple(lti), csc=csc,
                                    workspace=workspace, batch=self.batch, ltv=tuple(ltv))
        self.csc = self.plan.csc
        p = self.plan
        self.ng, self.no, self.nc = p.ng, p.no, p.nc

        lib = capi.load()
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = lib.mpcasm_plan_create(*_table_args(p), ctypes.byref(self._handle))
        capi.check(rc, "mpcasm_plan_create")

        # sources: shared copies of the formulation's horizon matrices
        self._src = [_as_device(torch, s.array, self.device) for s in p.sources]
        self._src_stride = [0] * len(p.sources)
        self._src_index = {s.key: i for i, s in enumerate(p.sources)}
        self._lti = {g["name"]: g for g in p.lti}
        for g in p.lti:     # S[0][j][i] = A[i][j], U_j[0][0][i] = B[i][j]  (tools.py:14-33)
            ids = g["ids"]
            A = p.sources[ids[-1]].array[0].T
            Bm = np.stack([p.sources[ids[j]].array[0, 0, :] for j in range(g["m"])], axis=1)
            self.bind_lti(g["name"], A, Bm)

        self._ltv = {g["name"]: g for g in p.ltv}
        self._bind_ltv_nominal([s.array for s in p.sources])

        base = torch.as_tensor(p.params, dtype=torch.float64, device=self.device)
        self.params = base.unsqueeze(0).repeat(self.batch, 1).contiguous()

        self._work = None
        self._workspace()
        self._out = None
        # what a launch at this capacity would compile, now (not in the middle of a control loop)
        with torch.cuda.device(self.device):
            capi.check(lib.mpcasm_plan_prepare(self._handle, self.batch), "mpcasm_plan_prepare")
        self._csc = {}

    def __del__(self):
        handle = getattr(self, "_handle", None)
        if handle:
            try:
                capi.load().mpcasm_plan_destroy(handle)
            except Exception:
                pass
            self._handle = None

    def _workspace(self):
        """The scratch buffer of a launch, as large as the kernels the options in force pick
        ask for (``mpcasm_workspace_bytes``: a wide problem needs a few KB per instance on the
        tiled kernel, its whole preview-matrix workspace on the staged pipeline)."""
        nbytes = ctypes.c_size_t()
        capi.check(capi.load().mpcasm_workspace_bytes(self._handle, self.batch, ctypes.byref(nbytes)),
                   "mpcasm_workspace_bytes")
        need = max(nbytes.value // 8, 1)
        if self._work is None or self._work.numel() < need:
            self._work = None
            self._work = self._torch.empty(need, dtype=self._torch.float64, device=self.device)
        return self._work

    def set_option(self, option, value):
        """This assembler's own kernel path (``capi.OPT_PATH``), per-plan compilation
        (``capi.OPT_JIT``) or workgroups per CU (``capi.OPT_RESIDENT_PER_CU``); ``-1``: the
        process-wide value again.  Plan state, unlike ``mpcasm_set_option``."""
        capi.check(capi.load().mpcasm_plan_set_option(self._handle, int(option), int(value)),
                   "mpcasm_plan_set_option")
        if int(option) == capi.OPT_PATH:
            self._opt_path = int(value)

    # ---- per-instance numbers -------------------------------------------------
    def refresh_params(self):
        """Re-read weights / aims / arrows / centres / extremes from the Cost and
        Constraint objects the plan was compiled from and broadcast them over the
        batch.  Returns False when a field changed shape (recompile needed)."""
        values = self.plan.current_params()
        if values is None:
            return False
        if self.batch == 1:   # (the drop-in tick: one upload straight into place, no broadcast kernel)
            self.params.copy_(self._torch.from_numpy(
                np.ascontiguousarray(values, dtype=np.float64)).reshape(self.params.shape))
            return True
        base = self._torch.as_tensor(values, dtype=self._torch.float64, device=self.device)
        self.params[:] = base.unsqueeze(0)
        return True

    def source_keys(self):
        return list(self._src_index.keys())

    def rebind_sources(self, form, frozen=None):
        """Re-read every horizon matrix / coefficient block from ``form`` (``frozen``: the
        snapshot of the horizon matrices taken by ``make_preview_matrices``) into this
        assembler's shared source slots -- what a tick changes when the structure stays.
        Returns False when a block no longer is what the plan compiled it as (recompile)."""
        fresh = []
        for s in self.plan.sources:
            block = s.getter(form, frozen) if s.getter is not None else s.array
            if block is None:
                return False
            fresh.append(np.ascontiguousarray(block, dtype=np.float64))
        # a U_j the plan's tile masks / CSC patterns took as causal (zeros above the diagonal,
        # tools.py:27-31) no longer is: the tables do not hold for it
        if any(not is_causal(fresh[i]) for i in self.plan.causal_assumed):
            return False
        generated = {i for g in self.plan.lti + self.plan.ltv for i in g["ids"]}
        # all blocks side by side in one device arena, filled by ONE copy from a pinned staging
        # buffer (a tick of the walking loop is copy-bound: ~20 us per separate upload)
        torch = self._torch
        shared = [i for i in range(len(fresh)) if i not in generated]
        starts = np.cumsum([0] + [fresh[i].size + (fresh[i].size & 1) for i in shared])   # (16-byte aligned)
        arena = getattr(self, "_src_arena", None)
        if arena is None or arena[0].numel() != int(starts[-1]):
            arena = self._src_arena = (
                torch.empty(int(starts[-1]), dtype=torch.float64, device=self.device),
                torch.empty(int(starts[-1]), dtype=torch.float64).pin_memory())
        stage = arena[1].numpy()
        for a, i in zip(starts, shared):
            stage[a:a + fresh[i].size] = fresh[i].ravel()
        arena[0].copy_(arena[1])
        for a, i in zip(starts, shared):
            self._src[i] = arena[0][a:a + fresh[i].size].view(fresh[i].shape)
            self._src_stride[i] = 0
        for g in self.plan.lti:     # S[0][j][i] = A[i][j], U_j[0][0][i] = B[i][j]  (tools.py:14-33)
            ids = g["ids"]
            A = fresh[ids[-1]][0].T
            Bm = np.stack([fresh[ids[j]][0, 0, :] for j in range(g["m"])], axis=1)
            self.bind_lti(g["name"], A, Bm)
        self._bind_ltv_nominal(fresh)
        return True

    def bind_source(self, key, tensor, check=True):
        """Use ``tensor`` for the horizon matrix ``key = (dynamics name, k)``:
        shape ``(N, p, n)`` (shared) or ``(B, N, p, n)`` (one per instance).

        Where the plan's tables rely on the matrix being causal -- ``U_j[k][l] = 0`` for ``l > k``,
        as ``tools.extend_matrices`` / :func:`fill_su` produce it: the tile masks of the tiled kernel
        (wide problems) and the CSC patterns -- a tensor that is not raises ``ValueError`` (one
        reduction on the device per call; ``check=False`` for a caller that guarantees it)."""
        torch = self._torch
        i = self._src_index[key]
        if key[0] in self._lti or key[0] in self._ltv:
            raise ValueError("the horizon matrices of %r are generated on chip: bind_lti / bind_ltv" % key[0])
        shape = tuple(self.plan.sources[i].array.shape)
        t = _as_device(torch, tensor, self.device)
        if check and i in self.plan.causal_assumed and tuple(t.shape)[-3:] == shape:
            N = shape[0]
            above = torch.triu(torch.ones(N, N, dtype=torch.bool, device=self.device), diagonal=1)
            if bool((t[..., above, :] != 0).any().item()):
                raise ValueError(
                    "source %r: the plan was compiled for a causal horizon matrix (zeros above the "
                    "diagonal, as tools.extend_matrices produces it); compile a plan from a "
                    "formulation that holds such a matrix to bind this one" % (key,))
        if tuple(t.shape) == shape:
            self._src[i], self._src_stride[i] = t, 0
        elif tuple(t.shape) == (self.batch,) + shape:
            self._src[i], self._src_stride[i] = t, int(np.prod(shape))
        else:
            raise ValueError("source %r expects %s or %s, got %s"
                             % (key, shape, (self.batch,) + shape, tuple(t.shape)))

    def _bind_ltv_nominal(self, arrays):
        """Until :meth:`bind_ltv` says otherwise: at every step the pair the horizon matrices in
        ``arrays`` were extended from, S[0][j][i] = A[i][j], U_j[0][0][i] = B[i][j] (tools.py:14-33)."""
        keys = [s.key for s in self.plan.sources]
        for g in self.plan.ltv:
            m = g["m"]
            A = arrays[keys.index((g["name"], m))][0].T
            Bm = np.stack([arrays[keys.index((g["name"], j))][0, 0, :] for j in range(m)], axis=1)
            self.bind_ltv(g["name"], np.broadcast_to(A, (g["N"],) + A.shape).copy(),
                          np.broadcast_to(Bm, (g["N"],) + Bm.shape).copy())

    def bind_ltv(self, name, A, B):
        """Per-step system matrices of a dynamics compiled as ``ltv``: ``A`` ``(N, n, n)`` /
        ``(B, N, n, n)`` and ``B`` ``(N, n, m)`` / ``(B, N, n, m)``, ``x_{k+1} = A_k x_k + B_k u_k``.
        They travel in the slots of the dynamics' first two horizon matrices (include/mpcasm.h)."""
        torch = self._torch
        g = self._ltv[name]
        n, m, N = g["n"], g["m"], g["N"]
        for slot, (t, shape) in enumerate(((A, (N, n, n)), (B, (N, n, m)))):
            t = _as_device(torch, t, self.device)
            i = g["ids"][slot]
            if tuple(t.shape) == shape:
                self._src[i], self._src_stride[i] = t, 0
            elif tuple(t.shape) == (self.batch,) + shape:
                self._src[i], self._src_stride[i] = t, int(np.prod(shape))
            else:
                raise ValueError("%s of %r expects %s or %s, got %s"
                                 % ("AB"[slot], name, shape, (self.batch,) + shape, tuple(t.shape)))

    def bind_ltv_window(self, name, A_seq, B_seq, t):
        """The steps ``[t, t + N)`` of a longer sequence as the per-step matrices of a dynamics compiled as ``ltv``
        -- ``A_seq`` ``(T, n, n)`` / ``(B, T, n, n)`` and ``B_seq`` ``(T, n, m)`` / ``(B, T, n, m)``, contiguous
        float64 tensors on this assembler's device, ``t + N <= T`` -- bound by pointer offset, nothing copied:
        instance ``b`` reads its ``N`` steps from ``t`` on, a batch stride of ``T n n`` (``T n m``) apart.  The
        receding horizon of a loop is one call per tick (:class:`mpcasm.ltv_loop.LtvLoop`); :meth:`bind_ltv` is
        for a window that lies on its own."""
        torch = self._torch
        g = self._ltv[name]
        n, m, N = g["n"], g["m"], g["N"]
        t = int(t)
        T = A_seq.shape[-3] if torch.is_tensor(A_seq) and A_seq.dim() >= 3 else -1
        if not 0 <= t <= T - N:
            raise ValueError("the window [%d, %d) does not lie in the %d steps of the sequence" % (t, t + N, T))
        for slot, (seq, tail) in enumerate(((A_seq, (T, n, n)), (B_seq, (T, n, m)))):
            if _tensor(torch, seq, torch.float64, None, self.device, None) is None \
                    or tuple(seq.shape) not in (tail, (self.batch,) + tail):
                raise ValueError("%s_seq of %r: a contiguous float64 tensor of shape %s or %s on %s"
                                 % ("AB"[slot], name, tail, (self.batch,) + tail, self.device))
            i = g["ids"][slot]
            # (a view that starts at step t: its data_ptr is the window's, the tensor keeps the sequence alive)
            self._src[i] = seq[..., t:, :, :]
            self._src_stride[i] = int(np.prod(tail)) if seq.dim() == 4 else 0

    def bind_lti(self, name, A, B):
        """System matrices of a dynamics compiled as ``lti``: ``A`` ``(n, n)`` / ``(B, n, n)``
        and ``B`` ``(n, m)`` / ``(B, n, m)``, x+ = A x + B u.  They travel in the slots of
        the group's first two horizon matrices (include/mpcasm.h)."""
        torch = self._torch
        g = self._lti[name]
        n, m = g["n"], g["m"]
        for slot, (t, shape) in enumerate(((A, (n, n)), (B, (n, m)))):
            t = _as_device(torch, t, self.device)
            i = g["ids"][slot]
            if tuple(t.shape) == shape:
                self._src[i], self._src_stride[i] = t.contiguous(), 0
            elif tuple(t.shape) == (self.batch,) + shape:
                self._src[i], self._src_stride[i] = t.contiguous(), shape[0] * shape[1]
            else:
                raise ValueError("%s of %r expects %s or %s, got %s" % (
                    "AB"[slot], name, shape, (self.batch,) + shape, tuple(t.shape)))

    def param_slice(self, kind, name, field):
        """Columns of :attr:`params` holding one field, e.g.
        ``("cost", "track vel_x", "aim")`` or ``("limit", 3, "center")``."""
        start, rows, cols = self.plan.param_slots[(kind, name, field)]
        return slice(start, start + rows * cols), (rows, cols)

    def soft_rows(self, rules):
        """:func:`plan.soft_rows` of this assembler's plan on its device: ``(lin, quad)``, two ``(nc,)`` float64
        tensors for ``solve_qp(soft=...)``."""
        lin, quad = soft_rows(self.plan, rules)
        return (self._torch.as_tensor(lin, device=self.device), self._torch.as_tensor(quad, device=self.device))

    def set_param(self, kind, name, field, values):
        """``values``: shape ``(rows, cols)`` (all instances) or ``(B, rows, cols)``."""
        torch = self._torch
        sl, (rows, cols) = self.param_slice(kind, name, field)
        v = _as_device(torch, values, self.device).reshape(-1, rows * cols)
        if v.shape[0] not in (1, self.batch):
            raise ValueError("expected 1 or %d instances, got %d" % (self.batch, v.shape[0]))
        self.params[:, sl] = v

    # ---- launches ---------------------------------------------------------------
    def _src_args(self):
        # (rebuilt only when a source has been bound to another tensor since the last launch)
        key = tuple(t.data_ptr() for t in self._src) + tuple(self._src_stride)
        if getattr(self, "_src_key", None) != key:
            n = len(self._src)
            ptrs = (ctypes.c_void_p * max(n, 1))(*key[:n])
            strides = (ctypes.c_int64 * max(n, 1))(*self._src_stride)
            self._src_key, self._src_ctypes = key, (ptrs, strides)
        return self._src_ctypes

    def _call_rc(self, name, *args, stream=None):
        """The status of the entry ``name`` called the way every entry that takes the plan and its sources is:
        ``name(plan, h_src, h_src_stride, *args, stream)`` with this assembler's device current."""
        torch = self._torch
        ptrs, strides = self._src_args()
        with torch.cuda.device(self.device):
            return getattr(capi.load(), name)(self._handle, ptrs, strides, *args, _stream_handle(torch, stream))

    def _call(self, name, *args, stream=None):
        """:meth:`_call_rc`, a status that is not ``MPCASM_OK`` raised."""
        capi.check(self._call_rc(name, *args, stream=stream), name)

    def assemble(self, given=None, out=None, stream=None, want_cost=True, want_constraints=True,
                 count=None, index=None, params=None):
        """Assemble the batch; returns ``(P, q, G, h)`` device tensors (``None`` for a
        skipped half).  ``given``: ``(B, ng)`` or ``(ng,)``.  ``count`` < batch assembles
        only the first ``count`` instances (buffers keep their full capacity).
        ``index`` (int32 device tensor, ``count`` entries): instance ``b`` reads row ``index[b]`` of
        ``given`` -- which may then have any number of rows, e.g. a whole fleet's -- and row ``b`` of
        everything else (``mpcasm_assemble_indexed``; a gather in front where the plan does not run
        on the persistent kernel).  ``params``: a ``(B, n_params)`` tensor to read the parameters
        from instead of :attr:`params` (a fleet keeps one per place in its step cycle)."""
        torch = self._torch
        B, ng, no, nc = self.batch, self.ng, self.no, self.nc
        n_run = B if count is None else int(count)
        if not 0 <= n_run <= B:
            raise ValueError("count must lie in [0, %d]" % B)
        if index is not None:
            if _tensor(torch, index, torch.int32, None, self.device, None) is None or index.numel() < n_run or not ng:
                raise ValueError("index: a contiguous int32 tensor of %d entries on %s" % (n_run, self.device))
            g = _as_device(torch, given, self.device).reshape(-1, ng)
        elif ng:
            g = _as_device(torch, given, self.device).reshape(-1, ng)
            if g.shape[0] == 1 and B > 1:
                g = g.repeat(B, 1)
            if g.shape[0] < n_run or (count is None and g.shape[0] != B):
                raise ValueError("given must have %d rows, got %d" % (n_run, g.shape[0]))
        else:
            g = None
        self._params_arg(params)
        if out is None:
            if self._out is None:
                f = dict(dtype=torch.float64, device=self.device)
                pshape = (B, self.csc["pnnz"]) if self.csc else (B, no, no)
                gshape = (B, self.csc["gnnz"]) if self.csc else (B, nc, no)
                self._out = (torch.empty(pshape, **f), torch.empty((B, no), **f),
                             torch.empty(gshape, **f), torch.empty((B, nc), **f))
            out = self._out
        P, q, G, h = out
        if not want_cost:
            P = q = None
        if not want_constraints or nc == 0:
            G = h = None
        self._launch(g, (P, q, G, h), n_run, stream, index, params)
        return P, q, G, h

    def _launch(self, g, out, n_run, stream, index=None, params=None):
        torch = self._torch
        ptrs, strides = self._src_args()
        ptr = lambda t: t.data_ptr() if t is not None else None
        work = self._workspace()
        prm = self.params if params is None else params
        with torch.cuda.device(self.device):
            if index is not None:
                rc = capi.load().mpcasm_assemble_indexed(
                    self._handle, ptrs, strides, prm.data_ptr(), ptr(g), index.data_ptr(),
                    *(ptr(t) for t in out), work.data_ptr(), n_run, _stream_handle(torch, stream))
                if rc == capi.ERR_LIMIT:     # (not on the persistent kernel: gather, then as ever)
                    g = g.index_select(0, index[:n_run].long())
                    index = None
            if index is None:
                rc = capi.load().mpcasm_assemble(
                    self._handle, ptrs, strides, prm.data_ptr(), ptr(g), *(ptr(t) for t in out),
                    work.data_ptr(), n_run, _stream_handle(torch, stream))
        capi.check(rc, "mpcasm_assemble")

    def last_kernel(self):
        """Name of the kernel(s) the latest :meth:`assemble` launched (``mpcasm_plan_last_kernel``)."""
        return capi.KERNEL_NAMES.get(capi.load().mpcasm_plan_last_kernel(self._handle), "?")

    # ---- sparse hand-off (f3) ------------------------------------------------------
    def csc_pattern(self, which, upper=False):
        """``(indptr, indices)`` (numpy int32) of the batch-wide CSC pattern of ``"P"`` or
        ``"G"``: every entry that can be non-zero for this structure, whatever the numbers
        (``upper``: only the upper triangle, as OSQP wants P).  Dense when the plan is too
        large for the structural analysis."""
        from .plan import csc_pattern

        if self.csc:      # the pattern the assembly itself writes
            return self.csc[which]
        key = (which, bool(upper))
        if key not in self._csc:
            mask = {"P": self.plan.P_pattern, "G": self.plan.G_pattern}[which]
            if mask is None:
                mask = np.ones((self.no, self.no) if which == "P" else (self.nc, self.no), dtype=bool)
            indptr, indices, flat = csc_pattern(mask, upper)
            self._csc[key] = (indptr, indices,
                              self._torch.as_tensor(flat, dtype=self._torch.int32, device=self.device))
        return self._csc[key][0], self._csc[key][1]

    def export_csc(self, which, dense=None, upper=False, count=None, stream=None):
        """``(B, nnz)`` device tensor: the ``data`` arrays of ``scipy.sparse.csc_matrix(M)`` for
        every instance's ``M = P`` or ``G`` on the pattern of :meth:`csc_pattern`
        (biped_mpc_loop.py:57-58, batched).  ``dense`` defaults to the last :meth:`assemble`."""
        torch = self._torch
        if self.csc:
            raise ValueError("this assembler writes the CSC form itself: assemble() returns it")
        self.csc_pattern(which, upper)
        index = self._csc[(which, bool(upper))][2]
        if dense is None:
            dense = self._out[0 if which == "P" else 2]
        n = self.batch if count is None else int(count)
        out = torch.empty((n, index.numel()), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = capi.load().mpcasm_gather(
                dense.data_ptr(), dense[0].numel(), index.data_ptr(), index.numel(),
                out.data_ptr(), n, _stream_handle(torch, stream))
        capi.check(rc, "mpcasm_gather")
        return out

    def preview_matrices(self, stream=None):
        """``(B, preview_rows, ng+no)`` device tensor; rows of definition ``v`` are
        ``plan.pm_rows[v]``, columns ``[:ng]`` = Mg, ``[ng:]`` = Mo."""
        torch = self._torch
        W = self.ng + self.no
        PM = torch.empty((self.batch, self.plan.pmrows, W), dtype=torch.float64,
                         device=self.device)
        self._call("mpcasm_preview_matrices", PM.data_ptr(), self.batch, stream=stream)
        return PM

    def preview_rows(self, given, optim, out=None, stream=None, count=None):
        """``Mg @ given + Mo @ optim`` for every row of every definition (body.py:209-219)
        without a preview matrix in memory (``mpcasm_preview_direct``): ``(B, preview_rows)``;
        rows of definition ``v`` are ``plan.pm_rows[v]``.  ``given``: ``(B, ng)``, ``optim``:
        ``(B, no)`` (the solver's answer)."""
        torch = self._torch
        n = self.batch if count is None else int(count)
        if not 0 <= n <= self.batch:         # (the scratch and the result are sized for the batch)
            raise ValueError("count must lie in 0 .. %d, got %d" % (self.batch, n))
        g = _as_device(torch, given, self.device).reshape(-1, self.ng) if self.ng else None
        x = _as_device(torch, optim, self.device).reshape(-1, self.no) if self.no else None
        for t, name in ((g, "given"), (x, "optim")):
            if t is not None and t.shape[0] < n:
                raise ValueError("%s must have %d rows, got %d" % (name, n, t.shape[0]))
        if out is None:
            out = torch.empty((self.batch, self.plan.pmrows), dtype=torch.float64, device=self.device)
        else:
            _checked_out(torch, out, (n, self.plan.pmrows), self.device, "preview_rows")
        self._call("mpcasm_preview_direct", g.data_ptr() if g is not None else None,
                   x.data_ptr() if x is not None else None, out.data_ptr(), self._workspace().data_ptr(), n,
                   stream=stream)
        return out

    # ---- the derivative of the assembly with respect to `given` ---------------------------------
    def _adjoint_args(self, what, count, tensors):
        """The instances a call runs and its operands checked: ``tensors`` is ``(tensor or None, width, name)``."""
        torch = self._torch
        n = self.batch if count is None else int(count)
        if not 0 <= n <= self.batch:
            raise ValueError("count must lie in 0 .. %d, got %d" % (self.batch, n))
        checked = []
        for t, width, name in tensors:
            if t is not None:
                t = _as_device(torch, t, self.device).reshape(-1, width).contiguous() if width else None
                if t is not None and t.shape[0] < n:
                    raise ValueError("%s: %s must have %d rows, got %d" % (what, name, n, t.shape[0]))
            checked.append(t)
        return n, checked

    def _params_arg(self, params):
        """:attr:`params`, or the caller's tensor in their place, checked as :meth:`assemble` checks it."""
        if params is None:
            return self.params
        return _tensor(self._torch, params, self._torch.float64, self.params.shape, self.device,
                       "params: a contiguous float64 tensor of shape %s on %s"
                       % (tuple(self.params.shape), self.device))

    def given_jvp(self, d, out=None, count=None, stream=None, params=None):
        """How ``q`` and ``h`` of :meth:`assemble` move along a change ``d (B, ng)`` of ``given``:
        ``(dq (B, no), dh (B, nc))``, ``dq = J_q d``, ``dh = -cMg d`` (``mpcasm_assemble_jvp``; ``P`` and ``G`` do not
        depend on ``given``), with this assembler's :attr:`params` and sources, matrix-free.  ``out``: the caller's
        ``(dq, dh)``, a None among them skipped (not both).  ``params``: a ``(B, n_params)`` tensor to read instead of
        :attr:`params`, as :meth:`assemble` takes it.  Refused (``ERR_LIMIT``) for a plan compiled with ``ltv=``."""
        torch = self._torch
        prm = self._params_arg(params)
        n, (d,) = self._adjoint_args("given_jvp", count, [(d, self.ng, "d")])
        if out is None:
            f = dict(dtype=torch.float64, device=self.device)
            out = (torch.zeros((self.batch, self.no), **f), torch.zeros((self.batch, self.nc), **f))
        dq, dh = out
        if dq is None and dh is None:
            raise ValueError("given_jvp: out holds neither dq nor dh")
        if dq is not None:
            _checked_out(torch, dq, (n, self.no), self.device, "given_jvp dq")
        if dh is not None:
            _checked_out(torch, dh, (n, self.nc), self.device, "given_jvp dh")
        ptr = lambda t: t.data_ptr() if t is not None else None
        self._call("mpcasm_assemble_jvp", prm.data_ptr(), ptr(d), ptr(dq), ptr(dh), self._workspace().data_ptr(), n,
                   stream=stream)
        return dq, dh

    def given_vjp(self, gq, gh, out=None, count=None, stream=None, params=None):
        """``dL/dgiven (B, ng) = J_q' gq + J_h' gh`` for ``gq = dL/dq (B, no)`` and ``gh = dL/dh (B, nc)`` of
        :meth:`assemble`'s ``q`` and ``h`` (``mpcasm_assemble_vjp``); a None cotangent is zero (not both).  Same
        conventions as :meth:`given_jvp`; ``out``: the caller's ``ggiven``."""
        torch = self._torch
        prm = self._params_arg(params)
        if gq is None and gh is None:
            raise ValueError("given_vjp: neither gq nor gh")
        n, (gq, gh) = self._adjoint_args("given_vjp", count, [(gq, self.no, "gq"), (gh, self.nc, "gh")])
        if out is None:
            out = torch.zeros((self.batch, self.ng), dtype=torch.float64, device=self.device)
        else:
            _checked_out(torch, out, (n, self.ng), self.device, "given_vjp")
        if gq is None and gh is None:      # (no rows of G and no gq: nothing depends on given)
            out[:n].zero_()
            return out
        ptr = lambda t: t.data_ptr() if t is not None else None
        self._call("mpcasm_assemble_vjp", prm.data_ptr(), ptr(gq), ptr(gh), out.data_ptr(),
                   self._workspace().data_ptr(), n, stream=stream)
        return out

    def adjoint_info(self):
        """What :meth:`given_jvp` / :meth:`given_vjp` launch with the sources bound now (:func:`adjoint_info`)."""
        return adjoint_info(self.plan, self._src_stride)

    # ---- ... and with respect to the parameters ---------------------------------------------------
    def params_vjp(self, given, x, u, y, w, verdict=None, active=None, params=None, out=None, count=None,
                   stream=None):
        """``dL/dparams (B, n_params)`` of a loss on the solution of the assembled QP (``mpcasm_assemble_params_vjp``):
        ``x (B, no)`` the solution, ``y (B, nc)`` its multipliers, ``u (B, no)`` and ``w (B, nc)`` what
        :func:`qp_sensitivity` returned for the loss -- they stand for ``dL/dP = -1/2 (u x' + x u')``, ``dL/dq = -u``,
        ``dL/dG_R = -(y_R u' + w_R x')``, ``dL/dh = w``, which are never formed.  ``y`` must be zero off the active set:
        ``active`` (bool ``(B, nc)``) zeroes it there first.  ``verdict`` (int32 ``(B,)``, the sensitivity's): an
        instance that is not ``SENS_DONE`` gets an exactly zero row and none of its vectors is read.  ``given``: the
        ``(B, ng)`` the QP was assembled from; ``params``: the tensor it was assembled with (default :attr:`params`).
        Use :meth:`param_grad` to read a field's gradient.  Refused (``ERR_LIMIT``) for a plan compiled with
        ``ltv=``."""
        torch = self._torch
        prm = self._params_arg(params)
        if active is not None:
            y = _as_device(torch, y, self.device).reshape(-1, self.nc) * active.reshape(-1, self.nc)
        n, (given, x, u, y, w) = self._adjoint_args("params_vjp", count, [
            (given, self.ng, "given"), (x, self.no, "x"), (u, self.no, "u"), (y, self.nc, "y"), (w, self.nc, "w")])
        for t, name, need in ((given, "given", self.ng), (x, "x", self.no), (u, "u", self.no), (y, "y", self.nc),
                              (w, "w", self.nc)):
            if need and t is None:
                raise ValueError("params_vjp: %s is missing" % name)
        if verdict is not None and (_tensor(torch, verdict, torch.int32, None, self.device, None) is None
                                    or verdict.numel() < n):
            raise ValueError("params_vjp: verdict is a contiguous int32 tensor of %d entries on %s" % (n, self.device))
        width = int(self.params.shape[1])
        if out is None:
            out = torch.zeros((self.batch, width), dtype=torch.float64, device=self.device)
        else:
            _checked_out(torch, out, (n, width), self.device, "params_vjp")
        ptr = lambda t: t.data_ptr() if t is not None else None
        self._call("mpcasm_assemble_params_vjp", prm.data_ptr(), ptr(given), ptr(x), ptr(u), ptr(y), ptr(w),
                   ptr(verdict), out.data_ptr(), self._workspace().data_ptr(), n, stream=stream)
        return out

    def params_adjoint_info(self):
        """What :meth:`params_vjp` launches with the sources bound now (:func:`params_adjoint_info`)."""
        return params_adjoint_info(self.plan, self._src_stride)

    def param_grad(self, gparams, kind, name, field):
        """The ``(B, rows, cols)`` view of one field in a ``(B, n_params)`` gradient that :meth:`params_vjp` made --
        the counterpart of :meth:`set_param`, through ``plan.param_slots``."""
        sl, (rows, cols) = self.param_slice(kind, name, field)
        return gparams[:, sl].view(gparams.shape[0], rows, cols)

    def preview_route(self, goals=False):
        """What :meth:`preview_rows` -- with ``goals`` (the Formulation whose goals :meth:`goal_terms` lists)
        the fused kernel of :meth:`full_goal_distances` -- launches with the sources bound now
        (:func:`preview_route`); ``None``: no kernel fuses the distances, :meth:`full_goal_distances` falls back."""
        nterms = ngoals = 0
        if goals is not False and goals is not None:
            table, names = self.goal_terms(goals)
            nterms, ngoals = int(table.shape[0]), len(names)
        return preview_route(self.plan, self._src_stride, nterms, ngoals)

    def sweep_route(self):
        """The instantiation of the sweep kernel :meth:`assemble` launches for this plan (:func:`sweep_route`)."""
        return sweep_route(self.plan)

    def staged_route(self, want_cost=True, want_constraints=True, count=None):
        """What the staged pipeline launches for this plan where :meth:`assemble` reaches it
        (:func:`staged_route`)."""
        return staged_route(self.plan, self.batch if count is None else int(count), want_cost,
                            want_constraints and bool(self.nc))

    def tiled_route(self, want_cost=True, want_constraints=True, count=None):
        """What :meth:`assemble` launches on the tiled path with the sources bound now and this assembler's
        ``capi.OPT_PATH`` (:func:`tiled_route`)."""
        want = (capi.WANT_COST if want_cost else 0) | (capi.WANT_CONSTRAINTS if want_constraints and self.nc else 0)
        return tiled_route(self.plan, self.batch if count is None else int(count), self._src_stride, want,
                           getattr(self, "_opt_path", -1))

    def param_map(self, rules, columns):
        """The device tables of a parameter map for this assembler's plan (rules and columns as
        :func:`param_map_records`): what :meth:`apply_param_map` reads.  A map belongs to one plan -- the buckets
        of a fleet each build their own."""
        torch = self._torch
        recs, coef = param_map_records(self.plan, rules, columns)
        signed = bool(recs.size and (recs[:, 2] & capi.PMAP_SIGNED).any())
        return ParamMap(torch.as_tensor(recs, device=self.device), torch.as_tensor(coef, device=self.device),
                        int(recs.shape[0]), len(list(columns)), signed, tuple(columns), self.plan, recs, coef)

    def apply_param_map(self, pmap, commands, index=None, sign=None, count=None, params=None, stream=None):
        """Per-instance commands into the parameters, IN PLACE (``mpcasm_params_map``; what the callbacks of
        ``Formulation.update`` do on the host, body.py:142-147): for the first ``count`` rows ``b`` of ``params``
        (default :attr:`params`) every record of ``pmap`` (:meth:`param_map`) writes its element from row
        ``index[b]`` of ``commands`` -- ``(rows, ncmd)`` float64, e.g. a whole fleet's; ``(ncmd,)``: one row
        shared by all -- times ``sign[b]`` where the record is signed.  ``index``: contiguous int32 device tensor,
        ``count`` entries inside ``commands`` (None: instance ``b`` reads row ``b``; the caller that builds it
        vouches for it, an index from the host is checked and copied).  ``sign``: ``(>= count,)`` float64, required
        when the map has a signed record (``ValueError``).  Everything no record names stays bit for bit.
        Nothing is read back.  Returns ``params``."""
        torch = self._torch
        n = self.batch if count is None else int(count)
        if not 0 <= n <= self.batch:
            raise ValueError("count must lie in 0 .. %d, got %d" % (self.batch, n))
        if not isinstance(pmap, ParamMap) or pmap.plan is not self.plan:
            raise ValueError("pmap: a map this assembler's param_map built")
        prm = self._params_arg(params)
        if _tensor(torch, commands, torch.float64, None, self.device, None) is None \
                or commands.dim() not in (1, 2) or commands.shape[-1] != pmap.ncmd:
            raise ValueError("commands: a contiguous float64 (rows, %d) or (%d,) tensor on %s"
                             % (pmap.ncmd, pmap.ncmd, self.device))
        shared = commands.dim() == 1
        if index is not None and shared:
            raise ValueError("index: one shared command row takes none")
        if index is not None and not torch.is_tensor(index):
            index = np.asarray(index)
            if index.ndim != 1 or index.size < n:
                raise ValueError("index: %d entries" % n)
            if index.size and (index[:n].min() < 0 or index[:n].max() >= commands.shape[0]):
                raise ValueError("index: entries in [0, %d)" % commands.shape[0])
            index = torch.as_tensor(index[:n].astype(np.int32), device=self.device)
        if index is not None:
            _tensor(torch, index, torch.int32, (n,), self.device,
                    "index: a contiguous int32 tensor of >= %d entries on %s" % (n, self.device), at_least=True)
        if index is None and not shared and commands.shape[0] < n:
            raise ValueError("commands must have %d rows, got %d" % (n, commands.shape[0]))
        check_param_map_sign(pmap.host_recs, sign)
        if sign is not None:
            _tensor(torch, sign, torch.float64, (n,), self.device,
                    "sign: a contiguous float64 tensor of >= %d entries on %s" % (n, self.device), at_least=True)
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):
            rc = capi.load().mpcasm_params_map(
                prm.data_ptr(), prm.shape[1], pmap.recs.data_ptr(), pmap.coef.data_ptr(), pmap.nrecs,
                commands.data_ptr(), 0 if shared else pmap.ncmd, pmap.ncmd, ptr(index), ptr(sign), n,
                _stream_handle(torch, stream))
        capi.check(rc, "mpcasm_params_map")
        return prm

    def given_map(self, rules):
        """The device table of a given map for this assembler's plan (``mpcasm_given_map_compile``; rules as
        :func:`given_map_records`): what :meth:`next_given` reads.  A map belongs to one plan -- the buckets
        of a fleet each build their own."""
        torch = self._torch
        rows, values = given_map_records(self.plan, rules)
        lib, words = capi.load(), ctypes.c_int64()
        args = (self._handle, rows.ctypes.data, values.ctypes.data, self.ng)
        capi.check(lib.mpcasm_given_map_compile(*args, None, 0, ctypes.byref(words)), "mpcasm_given_map_compile")
        host = np.zeros(max(words.value, 1), dtype=np.int32)
        capi.check(lib.mpcasm_given_map_compile(*args, host.ctypes.data, host.size, ctypes.byref(words)),
                   "mpcasm_given_map_compile")
        return GivenMap(torch.as_tensor(host, device=self.device), int(words.value), rows, values, self.plan)

    def next_given(self, given, optim, gmap, index=None, status=None, apply_mask=APPLY_SOLVED, count=None,
                   stream=None):
        """The next tick's ``given`` from a solution, IN PLACE (``mpcasm_next_given``; biped_mpc_loop.py:62-95):
        instance ``b`` reads row ``index[b]`` of ``given`` (``(rows, ng)``, e.g. a whole fleet's) and row ``b``
        of ``optim`` (``(>= count, no)``), evaluates the preview rows ``gmap`` (:meth:`given_map`) names and
        writes them, and its constants, into row ``index[b]``; the columns the map keeps stay as they are.
        ``index``: contiguous int32 device tensor, ``count`` DISTINCT entries in ``[0, rows)`` (None: instance
        ``b`` is row ``b``) -- the caller that builds it vouches for that, nothing is read back to check it; an
        index from the host (array or list) is checked (:func:`checked_index`) and copied to the device.
        ``status`` (``(>= count,)`` int32, :func:`solve_qp`'s): an instance whose status has no bit in
        ``apply_mask`` (``capi.qp_bit``; :data:`APPLY_SOLVED`, :data:`APPLY_ALL`) leaves its row untouched.
        Returns ``given``."""
        torch = self._torch
        n = self.batch if count is None else int(count)
        if not 0 <= n <= self.batch:         # (per-instance sources are sized for the batch)
            raise ValueError("count must lie in 0 .. %d, got %d" % (self.batch, n))
        if not isinstance(gmap, GivenMap) or gmap.plan is not self.plan:
            raise ValueError("gmap: a map this assembler's given_map built")
        _tensor(torch, given, torch.float64, (None, self.ng), self.device,
                "given: a contiguous float64 (rows, %d) tensor on %s (updated in place)" % (self.ng, self.device))
        _tensor(torch, optim, torch.float64, (n, self.no), self.device,
                "optim: a contiguous float64 (>= %d, %d) tensor on %s" % (n, self.no, self.device), at_least=True)
        if index is not None and not torch.is_tensor(index):
            index = np.asarray(index)
            if index.ndim != 1 or index.size < n:
                raise ValueError("index: %d entries" % n)
            index = torch.as_tensor(checked_index(index[:n], given.shape[0]), device=self.device)
        for t, name in ((index, "index"), (status, "status")):
            if t is not None:
                _tensor(torch, t, torch.int32, (n,), self.device,
                        "%s: a contiguous int32 tensor of >= %d entries on %s" % (name, n, self.device), at_least=True)
        if index is None and given.shape[0] < n:
            raise ValueError("given must have %d rows, got %d" % (n, given.shape[0]))
        ptr = lambda t: t.data_ptr() if t is not None else None
        self._call("mpcasm_next_given", given.data_ptr(), given.shape[0], optim.data_ptr(), ptr(index), ptr(status),
                   int(apply_mask) & 0xFFFFFFFF, gmap.table.data_ptr(), gmap.words, self._workspace().data_ptr(), n,
                   stream=stream)
        return given

    # ---- a plan compiled as ltv: rows and the next given by the forward recursion ------------------------
    def _rollout_table(self):
        """The device copy of this plan's row table (:func:`rollout_table`), made once."""
        if not self._ltv:
            raise ValueError("no dynamics of this assembler was compiled as ltv: its rows come from preview_rows, "
                             "its next given from next_given")
        if getattr(self, "_roll", None) is None:
            self._roll = self._torch.as_tensor(rollout_table(self.plan), device=self.device)
        return self._roll

    def rollout_info(self, rows=True, count=None):
        """``(group, lds_bytes, workgroups)`` of the launch :meth:`rollout` (``rows``) or :meth:`advance` (not
        ``rows``) makes for ``count`` instances (default: the batch) -- :func:`rollout_info` on this plan's row
        table; nothing is launched."""
        return rollout_info(self.plan, rows, self.batch if count is None else count, self._rollout_table().numel())

    def _rollout_args(self, given, optim, index, n, writes):
        torch = self._torch
        if not 0 <= n <= self.batch:         # (per-instance sources are sized for the batch)
            raise ValueError("count must lie in 0 .. %d, got %d" % (self.batch, n))
        _tensor(torch, given, torch.float64, (None, self.ng), self.device,
                "given: a contiguous float64 (rows, %d) tensor on %s%s"
                % (self.ng, self.device, " (updated in place)" if writes else ""))
        _tensor(torch, optim, torch.float64, (n, self.no), self.device,
                "optim: a contiguous float64 (>= %d, %d) tensor on %s" % (n, self.no, self.device), at_least=True)
        if index is not None and not torch.is_tensor(index):
            index = np.asarray(index)
            if index.ndim != 1 or index.size < n:
                raise ValueError("index: %d entries" % n)
            index = index[:n]
            if writes:
                index = checked_index(index, given.shape[0])
            elif index.size and (index.min() < 0 or index.max() >= given.shape[0]):
                raise ValueError("an index of rows must hold entries in [0, %d)" % given.shape[0])
            index = torch.as_tensor(index.astype(np.int32), device=self.device)
        if index is not None:
            _tensor(torch, index, torch.int32, (n,), self.device,
                    "index: a contiguous int32 tensor of >= %d entries on %s" % (n, self.device), at_least=True)
        if index is None and given.shape[0] < n:
            raise ValueError("given must have %d rows, got %d" % (n, given.shape[0]))
        return index

    def rollout(self, given, optim, index=None, out=None, count=None, stream=None):
        """:meth:`preview_rows` for a plan compiled with ``ltv=`` (``mpcasm_ltv_rollout``; body.py:209-219):
        ``(B, preview_rows)``, rows of definition ``v`` at ``plan.pm_rows[v]``, from the forward recursion
        ``x_{k+1} = A_k x_k + B_k u_k`` on the ``(A_k, B_k)`` bound now (:meth:`bind_ltv`,
        :meth:`bind_ltv_window`) -- no horizon matrix, no workspace; the rows that are a given value or an unknown
        itself are copies, bit for bit.  ``given``: ``(rows, ng)``, ``optim``: ``(>= count, no)``, contiguous
        float64 tensors on this device; ``index`` (int32 device tensor, or a host array: checked and copied):
        instance ``b`` reads row ``index[b]`` of ``given``.  The rows are what :meth:`goal_distance` takes: the
        goals' distances of such a plan are ``asm.goal_distance(form, asm.rollout(given, optim))``.
        ``ValueError`` on an assembler without ``ltv=``: :meth:`preview_rows` is for it."""
        torch = self._torch
        table = self._rollout_table()
        n = self.batch if count is None else int(count)
        index = self._rollout_args(given, optim, index, n, False)
        if out is None:
            out = torch.empty((self.batch, self.plan.pmrows), dtype=torch.float64, device=self.device)
        else:
            _checked_out(torch, out, (n, self.plan.pmrows), self.device, "rollout")
        self._call("mpcasm_ltv_rollout", given.data_ptr(), given.shape[0], optim.data_ptr(),
                   index.data_ptr() if index is not None else None, table.data_ptr(), table.numel(), out.data_ptr(),
                   n, stream=stream)
        return out

    def advance(self, given, optim, index=None, status=None, apply_mask=APPLY_SOLVED, count=None, stream=None):
        """:meth:`next_given` for a plan compiled with ``ltv=`` (``mpcasm_ltv_advance``; biped_mpc_loop.py:62-95):
        row ``index[b]`` of ``given`` becomes ``x_1 = A_0 x_0 + B_0 u_0`` of every axis, IN PLACE, from row ``b``
        of ``optim`` -- every given value of such a plan is an initial state, so no map is needed.  ``index``,
        ``status`` and ``apply_mask`` as for :meth:`next_given`: distinct rows in range (a host index is checked,
        :func:`checked_index`), and an instance whose status has no bit in ``apply_mask`` leaves its row exactly
        as it was.  Returns ``given``.  ``ValueError`` on an assembler without ``ltv=``: :meth:`next_given` is
        for it."""
        torch = self._torch
        table = self._rollout_table()
        n = self.batch if count is None else int(count)
        index = self._rollout_args(given, optim, index, n, True)
        if status is not None:
            _tensor(torch, status, torch.int32, (n,), self.device,
                    "status: a contiguous int32 tensor of >= %d entries on %s" % (n, self.device), at_least=True)
        ptr = lambda t: t.data_ptr() if t is not None else None
        self._call("mpcasm_ltv_advance", given.data_ptr(), given.shape[0], optim.data_ptr(), ptr(index), ptr(status),
                   int(apply_mask) & 0xFFFFFFFF, table.data_ptr(), table.numel(), n, stream=stream)
        return given

    def true_inputs(self, K_seq, t, given, optim, index=None, out=None, count=None, stream=None):
        """The true inputs of a plan whose bound window is a closed loop's (``mpcasm_ltv_true_inputs``): with
        ``A_cl = A + B K`` bound in ``A``'s place (:meth:`bind_ltv_window`) the unknowns are ``v``, and along
        ``x_{k+1} = A_cl_k x_k + B_k v_k`` from the axis' initial state in ``given`` this returns ``u_k = K_k x_k +
        v_k`` for every instance, axis and step: ``(B, axes, N, m)``.  ``K_seq`` ``(T, m, n)`` / ``(B, T, m, n)``, a
        contiguous float64 tensor on this device: the window ``[t, t + N)`` of it is taken by pointer, as
        :meth:`bind_ltv_window` takes the matrices'.  ``given``, ``optim``, ``index``, ``count`` as for
        :meth:`rollout`."""
        torch = self._torch
        self._rollout_table()        # (ValueError on an assembler without ltv=)
        g = self.plan.ltv[0]
        n, m, N = g["n"], g["m"], g["N"]
        axes = self.plan.sweep["axes"].shape[0]
        t = int(t)
        T = K_seq.shape[-3] if torch.is_tensor(K_seq) and K_seq.dim() >= 3 else -1
        if not 0 <= t <= T - N:
            raise ValueError("the window [%d, %d) does not lie in the %d steps of the gains" % (t, t + N, T))
        tail = (T, m, n)
        if _tensor(torch, K_seq, torch.float64, None, self.device, None) is None \
                or tuple(K_seq.shape) not in (tail, (self.batch,) + tail):
            raise ValueError("K_seq: a contiguous float64 tensor of shape %s or %s on %s"
                             % (tail, (self.batch,) + tail, self.device))
        cnt = self.batch if count is None else int(count)
        index = self._rollout_args(given, optim, index, cnt, False)
        if out is None:
            out = torch.empty((self.batch, axes, N, m), dtype=torch.float64, device=self.device)
        else:
            _checked_out(torch, out, (cnt, axes, N, m), self.device, "true_inputs")
        self._call("mpcasm_ltv_true_inputs", K_seq.data_ptr() + 8 * t * m * n, T * m * n if K_seq.dim() == 4 else 0,
                   given.data_ptr(), given.shape[0], optim.data_ptr(), index.data_ptr() if index is not None else None,
                   out.data_ptr(), cnt, stream=stream)
        return out

    def goal_terms(self, form):
        """Device table of ``mpcasm_goal_distance`` for ``form.goals`` (the plan's costs): one
        record ``(goal, first preview row, rows, aim's parameter slot)`` per goal and axis;
        returns ``(table, goal names)``."""
        if getattr(self, "_goal_terms", None) is None:
            names, recs = list(form.goals.keys()), []
            for gi, name in enumerate(names):
                goal = form.goals[name]
                aim0 = self.plan.param_slots[("cost", name, "aim")][0]
                for i, axis in enumerate(goal.axes):
                    r0, rows = self.plan.pm_rows[goal.variable + axis]
                    recs.append([gi, r0, rows, aim0 + i])
            table = self._torch.as_tensor(np.asarray(recs, dtype=np.int32).reshape(-1, 4),
                                          device=self.device)
            self._goal_terms = (table, names)
        return self._goal_terms

    def goal_distance(self, form, rows, out=None, stream=None, count=None):
        """Squared distance of every goal's variable to its aim (body.py:221-228), per instance:
        ``(B, n_goals)`` from the rows of :meth:`preview_rows`; the row sum over the goals is
        ``full_goal_distance`` (:230-234).  Aims are read from :attr:`params`."""
        torch = self._torch
        table, names = self.goal_terms(form)
        n = self.batch if count is None else int(count)
        if not 0 <= n <= self.batch or rows.shape[0] < n:
            raise ValueError("count must lie in 0 .. %d and within the %d rows given, got %d"
                             % (self.batch, rows.shape[0], n))
        if out is None:
            out = torch.empty((self.batch, len(names)), dtype=torch.float64, device=self.device)
        else:
            _checked_out(torch, out, (n, len(names)), self.device, "goal_distance")
        with torch.cuda.device(self.device):
            rc = capi.load().mpcasm_goal_distance(
                rows.data_ptr(), rows.shape[1], self.params.data_ptr(), self.params.shape[1],
                table.data_ptr(), table.shape[0], len(names), out.data_ptr(), n,
                _stream_handle(torch, stream))
        capi.check(rc, "mpcasm_goal_distance")
        return out

    def full_goal_distances(self, form, given, optim, out=None, stream=None, count=None):
        """``goal_distance`` of every goal (body.py:221-234) straight from the sources, the rows
        of the definitions never leaving the chip (``mpcasm_preview_goal_distance``): ``(B, n_goals)``;
        the row sum is ``full_goal_distance``.  Falls back to :meth:`preview_rows` +
        :meth:`goal_distance` where the plan does not run on the kernel that fuses the two."""
        torch = self._torch
        table, names = self.goal_terms(form)
        n = self.batch if count is None else int(count)
        if not 0 <= n <= self.batch:
            raise ValueError("count must lie in 0 .. %d, got %d" % (self.batch, n))
        g = _as_device(torch, given, self.device).reshape(-1, self.ng) if self.ng else None
        x = _as_device(torch, optim, self.device).reshape(-1, self.no) if self.no else None
        for t, name in ((g, "given"), (x, "optim")):
            if t is not None and t.shape[0] < n:
                raise ValueError("%s must have %d rows, got %d" % (name, n, t.shape[0]))
        if out is None:
            out = torch.empty((self.batch, len(names)), dtype=torch.float64, device=self.device)
        else:
            _checked_out(torch, out, (n, len(names)), self.device, "full_goal_distances")
        rc = self._call_rc("mpcasm_preview_goal_distance", g.data_ptr() if g is not None else None,
                           x.data_ptr() if x is not None else None, self.params.data_ptr(), table.data_ptr(),
                           table.shape[0], len(names), out.data_ptr(), self._workspace().data_ptr(), n, stream=stream)
        if rc == capi.ERR_LIMIT:
            rows = self.preview_rows(given, optim, stream=stream, count=count)
            return self.goal_distance(form, rows, out=out, stream=stream, count=count)
        capi.check(rc, "mpcasm_preview_goal_distance")
        return out

    def preview(self, PM, given, optim, stream=None):
        """``Mg @ given + Mo @ optim`` for every definition row (body.py:209-219):
        ``(B, preview_rows)``."""
        torch = self._torch
        g = _as_device(torch, given, self.device).reshape(self.batch, self.ng) if self.ng else None
        x = _as_device(torch, optim, self.device).reshape(self.batch, self.no) if self.no else None
        out = torch.empty((self.batch, self.plan.pmrows), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = capi.load().mpcasm_preview(
                PM.data_ptr(), g.data_ptr() if g is not None else None,
                x.data_ptr() if x is not None else None, out.data_ptr(), self.batch,
                self.plan.pmrows, self.ng, self.no, _stream_handle(torch, stream))
        capi.check(rc, "mpcasm_preview")
        return out
