"""Differentiable QP solves: ``torch.autograd`` through :func:`mpcasm.engine.solve_qp`.

The forward pass is the solve with polishing, on the device; the backward pass is ONE call of
:func:`mpcasm.engine.qp_sensitivity` (``mpcasm_qp_sens``): at a strictly complementary solution with active rows ``A``
the KKT conditions are ``P x + q + G_A'y_A = 0``, ``G_A x = h_A``, and with ``[u; w_A] = K^-1 [dL/dx; dL/dy_A]`` for the
symmetric ``K = [[P, G_A'], [G_A, 0]]``

    dL/dq = -u      dL/dh = w      dL/dP = -1/2 (u x' + x u')      row i of dL/dG = -(y_i u' + w_i x'), active rows only

("The derivative of a solve").  ``dL/dP`` is the gradient with respect to a symmetric ``P``, which the
solvers require: a caller that builds ``P`` from parameters gets their gradient by the chain rule through that
construction.

Nobody holds ``P, q, G, h`` as leaves: they come out of the assembly.  ``P`` and ``G`` do not depend on ``given``, ``q``
and ``h`` are affine in it, and :meth:`mpcasm.engine.Assembler.given_vjp` / :meth:`~mpcasm.engine.Assembler.given_jvp`
apply that Jacobian and its transpose matrix-free on the device ("The derivative of the assembly").
:func:`mpc_solve_diff` chains the two -- ``given.grad`` of a loss on the solution of the MPC's QP -- and
:func:`tangent` is the tangential predictor ``x*(given + d) ~ x* + dx``.

The parameters (weights, aims, arrows, centres, extremes) enter ``P, q, G, h`` as factors of outer products of
workspace rows, and ``dL/dP``, ``dL/dG`` are of rank two, so ``params.grad`` is a short sum of products of three row
vectors: :meth:`mpcasm.engine.Assembler.params_vjp` (``mpcasm_assemble_params_vjp``) gathers it on the device without
the dense gradients, and ``mpc_solve_diff(asm, given, params=p)`` chains it behind the same sensitivity solve.  Still
open: plans compiled with ``ltv=`` (the sweep's backward recursion), the fleet's wiring (the ``params_map`` chain to
``commands.grad``) and a JVP in params.
"""
from . import engine
from .engine import require_device

_FUNCTION = None


class QpDiffSolution:
    """What :func:`solve_qp_diff` returns: ``x (B, no)`` and ``y (B, nc)``, differentiable with respect to the
    ``P, q, G, h`` that require grad; ``sol``, the :class:`mpcasm.engine.PolishedQpSolution` of the forward pass
    (plain tensors; ``sol.x`` and ``sol.y`` share ``x``'s and ``y``'s memory); and, None until ``backward`` has run,
    ``verdict`` ``(B,)`` int32 (``engine.SENS_*``) and ``lres`` ``(B,)`` of its sensitivity solve.  An instance whose
    verdict is not ``SENS_DONE`` (not solved, more active rows than unknowns, a KKT matrix that does not factor) got
    zero gradients."""
    __slots__ = ("x", "y", "_outcome", "__weakref__")

    def __init__(self, x, y, outcome):
        self.x, self.y, self._outcome = x, y, outcome

    sol = property(lambda self: self._outcome.sol)
    verdict = property(lambda self: self._outcome.verdict)
    lres = property(lambda self: self._outcome.lres)
    # (mpc_solve_diff with params=: the bool (B, nc) active set its params_vjp ran with; None otherwise)
    active = property(lambda self: getattr(self._outcome, "active", None))


class _Outcome:
    """What the two passes leave for the caller beside ``x`` and ``y``.  The autograd node holds THIS, never the
    :class:`QpDiffSolution`: that one holds the node's own outputs, and a node that held it would close a cycle
    through the autograd graph which Python's collector cannot see -- every call would keep its device tensors for
    good.  Nothing here refers to ``x`` or ``y`` (``sol.x`` is the plain tensor they are views of)."""
    __slots__ = ("sol", "verdict", "lres")

    def __init__(self):
        self.sol = self.verdict = self.lres = None


def _function(torch):
    global _FUNCTION
    if _FUNCTION is not None:
        return _FUNCTION

    class SolveQpDiff(torch.autograd.Function):
        @staticmethod
        def forward(ctx, P, q, G, h, outcome, wide, solve_kw):
            P, q, G, h = (t.detach().contiguous() for t in (P, q, G, h))
            solve = engine.solve_qp_wide if wide else engine.solve_qp
            sol = solve(P, q, G, h, polish=True, **solve_kw)
            outcome.sol = sol
            ctx.outcome, ctx.wide, ctx.stream = outcome, wide, solve_kw.get("stream")
            ctx.save_for_backward(P, G, h, sol.x, sol.y, sol.z, sol.status)
            return sol.x.view_as(sol.x), sol.y.view_as(sol.y)

        @staticmethod
        def backward(ctx, gx, gy):
            P, G, h, x, y, z, status = ctx.saved_tensors
            need_P, need_q, need_G, need_h = ctx.needs_input_grad[:4]
            sens = engine.qp_sensitivity_wide if ctx.wide else engine.qp_sensitivity
            s = sens(P, G, h, (x, y, z), gx.contiguous(), gy.contiguous(), status=status, want_P=need_P, want_G=need_G,
                     stream=ctx.stream)
            ctx.outcome.verdict, ctx.outcome.lres = s.verdict, s.lres
            return (s.gP if need_P else None, -s.u if need_q else None, s.gG if need_G else None,
                    s.w if need_h else None, None, None, None)

    _FUNCTION = SolveQpDiff
    return _FUNCTION


def solve_qp_diff(P, q, G, h, wide=False, **solve_kw):
    """``solve_qp(P, q, G, h, polish=True, **solve_kw)`` (``wide``: ``solve_qp_wide``) as a differentiable function
    of ``P, q, G, h``: a :class:`QpDiffSolution`.  ``backward`` through its ``x`` and ``y`` makes one
    :func:`mpcasm.engine.qp_sensitivity` (``wide``: ``qp_sensitivity_wide``) call on the solved instances and asks for
    the dense ``P.grad`` / ``G.grad`` only where ``P`` / ``G`` require grad; the gradients are the active-set model's
    at the polished point, zero for an instance that is not ``SENS_DONE``.  ``soft=`` is refused (``ValueError``):
    the active-set model is the hard problem's, as for ``solve_qp(polish=, soft=)``."""
    if solve_kw.get("soft") is not None:
        raise ValueError("solve_qp_diff with soft=: the active-set model of the derivative is the hard problem's")
    if "polish" in solve_kw:
        raise ValueError("solve_qp_diff always polishes: the derivative is taken at the polished point")
    solve_kw.pop("soft", None)
    torch = require_device()
    outcome = _Outcome()
    x, y = _function(torch).apply(P, q, G, h, outcome, bool(wide), solve_kw)
    return QpDiffSolution(x, y, outcome)


class _MpcOutcome(_Outcome):
    """:class:`_Outcome` of :func:`mpc_solve_diff`, with the assembled ``P, G, h`` the solve ran on (plain tensors of
    the call's own: :func:`tangent` reads them)."""
    __slots__ = ("P", "G", "h", "active")

    def __init__(self):
        super().__init__()
        self.P = self.G = self.h = self.active = None


_MPC_FUNCTION = None


def _mpc_function(torch):
    global _MPC_FUNCTION
    if _MPC_FUNCTION is not None:
        return _MPC_FUNCTION

    class MpcSolveDiff(torch.autograd.Function):
        @staticmethod
        def forward(ctx, given, asm, outcome, wide, solve_kw):
            g = given.detach().contiguous()
            f = dict(dtype=torch.float64, device=asm.device)
            B, no, nc = asm.batch, asm.no, asm.nc
            # (buffers of this call's own: the assembler's are overwritten by its next launch)
            out = (torch.empty((B, no, no), **f), torch.empty((B, no), **f), torch.empty((B, nc, no), **f),
                   torch.empty((B, nc), **f))
            asm.assemble(g, out=out, stream=solve_kw.get("stream"))
            P, q, G, h = out
            solve = engine.solve_qp_wide if wide else engine.solve_qp
            sol = solve(P, q, G, h, polish=True, **solve_kw)
            outcome.sol, outcome.P, outcome.G, outcome.h = sol, P, G, h
            ctx.asm, ctx.outcome, ctx.wide, ctx.stream = asm, outcome, wide, solve_kw.get("stream")
            ctx.save_for_backward(P, G, h, sol.x, sol.y, sol.z, sol.status)
            return sol.x.view_as(sol.x), sol.y.view_as(sol.y)

        @staticmethod
        def backward(ctx, gx, gy):
            P, G, h, x, y, z, status = ctx.saved_tensors
            sens = engine.qp_sensitivity_wide if ctx.wide else engine.qp_sensitivity
            s = sens(P, G, h, (x, y, z), gx.contiguous(), gy.contiguous(), status=status, want_P=False, want_G=False,
                     stream=ctx.stream)
            ctx.outcome.verdict, ctx.outcome.lres = s.verdict, s.lres
            # dL/dq = -u, dL/dh = w; an instance that is not SENS_DONE has u = w = 0: a zero row
            return ctx.asm.given_vjp(-s.u, s.w, stream=ctx.stream), None, None, None, None

    _MPC_FUNCTION = MpcSolveDiff
    return _MPC_FUNCTION


_MPC_PARAMS_FUNCTION = None


def _mpc_params_function(torch):
    global _MPC_PARAMS_FUNCTION
    if _MPC_PARAMS_FUNCTION is not None:
        return _MPC_PARAMS_FUNCTION

    class MpcSolveDiffParams(torch.autograd.Function):
        @staticmethod
        def forward(ctx, given, params, asm, outcome, wide, solve_kw):
            g, p = given.detach().contiguous(), params.detach().contiguous()
            f = dict(dtype=torch.float64, device=asm.device)
            B, no, nc = asm.batch, asm.no, asm.nc
            out = (torch.empty((B, no, no), **f), torch.empty((B, no), **f), torch.empty((B, nc, no), **f),
                   torch.empty((B, nc), **f))
            asm.assemble(g, out=out, stream=solve_kw.get("stream"), params=p)
            P, q, G, h = out
            solve = engine.solve_qp_wide if wide else engine.solve_qp
            sol = solve(P, q, G, h, polish=True, **solve_kw)
            outcome.sol, outcome.P, outcome.G, outcome.h = sol, P, G, h
            ctx.asm, ctx.outcome, ctx.wide, ctx.stream = asm, outcome, wide, solve_kw.get("stream")
            ctx.save_for_backward(P, G, h, sol.x, sol.y, sol.z, sol.status, g, p)
            return sol.x.view_as(sol.x), sol.y.view_as(sol.y)

        @staticmethod
        def backward(ctx, gx, gy):
            P, G, h, x, y, z, status, g, p = ctx.saved_tensors
            sens = engine.qp_sensitivity_wide if ctx.wide else engine.qp_sensitivity
            s = sens(P, G, h, (x, y, z), gx.contiguous(), gy.contiguous(), status=status, want_P=False, want_G=False,
                     stream=ctx.stream)
            ctx.outcome.verdict, ctx.outcome.lres = s.verdict, s.lres
            need_given, need_params = ctx.needs_input_grad[:2]
            ggiven = gparams = None
            if need_given:
                ggiven = ctx.asm.given_vjp(-s.u, s.w, stream=ctx.stream, params=p)
            if need_params:
                # the polish's own test of a row: one subtraction and one compare, so the same set bit for bit
                ctx.outcome.active = (h - z) < y
                gparams = ctx.asm.params_vjp(g, x, s.u, y, s.w, verdict=s.verdict, active=ctx.outcome.active,
                                             params=p, stream=ctx.stream)
            return ggiven, gparams, None, None, None, None

    _MPC_PARAMS_FUNCTION = MpcSolveDiffParams
    return _MPC_PARAMS_FUNCTION


def mpc_solve_diff(asm, given, params=None, wide=False, **solve_kw):
    """The MPC's QP as a differentiable function of ``given (B, ng)``, ``B = asm.batch``: ``asm.assemble(given)``, then
    ``solve_qp(P, q, G, h, polish=True, **solve_kw)`` (``wide``: ``solve_qp_wide``).  A :class:`QpDiffSolution`, as
    :func:`solve_qp_diff` returns it; ``backward`` through its ``x`` and ``y`` makes one
    :func:`mpcasm.engine.qp_sensitivity` call (no dense ``dL/dP``, ``dL/dG``: ``P`` and ``G`` do not depend on
    ``given``) and one :meth:`mpcasm.engine.Assembler.given_vjp` ``(-u, w)``.  An instance that is not ``SENS_DONE``
    gets an exactly zero row of ``given.grad``.  The assembler's :attr:`~mpcasm.engine.Assembler.params` and sources
    are read by both passes and not differentiated.  ``soft=`` and ``polish=`` are refused as in
    :func:`solve_qp_diff`.

    ``params``: a ``(B, n_params)`` float64 tensor to assemble with instead of ``asm.params`` (as
    ``asm.assemble(params=)``); ``given`` and ``params`` get gradients where they require them.  ``backward`` is then
    the same sensitivity solve followed by ``given_vjp`` and / or one :meth:`mpcasm.engine.Assembler.params_vjp`
    ``(given, x, u, y, w)`` with ``verdict`` the solve's and ``active = (h - z) < y`` (kept as ``.active`` of the
    result): no dense ``dL/dP``, ``dL/dG`` there either.  :meth:`mpcasm.engine.Assembler.param_grad` reads a field
    out of ``params.grad``."""
    if solve_kw.get("soft") is not None:
        raise ValueError("mpc_solve_diff with soft=: the active-set model of the derivative is the hard problem's")
    if "polish" in solve_kw:
        raise ValueError("mpc_solve_diff always polishes: the derivative is taken at the polished point")
    solve_kw.pop("soft", None)
    torch = require_device()
    if not (torch.is_tensor(given) and given.dtype == torch.float64 and given.device == asm.device
            and tuple(given.shape) == (asm.batch, asm.ng)):
        raise ValueError("given: a float64 tensor of shape (%d, %d) on %s" % (asm.batch, asm.ng, asm.device))
    outcome = _MpcOutcome()
    if params is None:
        x, y = _mpc_function(torch).apply(given, asm, outcome, bool(wide), solve_kw)
        return QpDiffSolution(x, y, outcome)
    if not (torch.is_tensor(params) and params.dtype == torch.float64 and params.device == asm.device
            and tuple(params.shape) == tuple(asm.params.shape)):
        raise ValueError("params: a float64 tensor of shape %s on %s" % (tuple(asm.params.shape), asm.device))
    x, y = _mpc_params_function(torch).apply(given, params, asm, outcome, bool(wide), solve_kw)
    return QpDiffSolution(x, y, outcome)


def tangent(asm, sol, d, wide=False, P=None, G=None, h=None):
    """The tangential predictor: ``(dx, dy)`` with ``x*(given + d) ~ x* + dx``, ``y* + dy`` while the active set
    stays -- :meth:`mpcasm.engine.Assembler.given_jvp` ``(d)`` fed to :func:`mpcasm.engine.qp_jvp` (``wide``: its wide
    form).  ``sol``: what :func:`mpc_solve_diff` returned (its ``P, G, h`` are used), or a polished
    :class:`mpcasm.engine.PolishedQpSolution` / :class:`~mpcasm.engine.QpSolution` together with the ``P, G, h`` it
    solved.  An instance that is not ``QP_SOLVED`` has ``dx = dy = 0``."""
    if isinstance(sol, QpDiffSolution):
        o = sol._outcome
        P = getattr(o, "P", None) if P is None else P
        G = getattr(o, "G", None) if G is None else G
        h = getattr(o, "h", None) if h is None else h
        sol = o.sol
    if P is None or G is None or h is None:
        raise ValueError("tangent: P, G, h of the solve (or the result of mpc_solve_diff)")
    dq, dh = asm.given_jvp(d)
    j = engine.qp_jvp(P, G, h, sol, dq, dh, status=getattr(sol, "status", None), wide=wide)
    return j.dx, j.dy
