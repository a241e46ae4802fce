"""numpy restatement of the sensitivity solve of a solved QP  --  TEST INFRASTRUCTURE ONLY (the checker of
``mpcasm_qp_sens`` and ``mpcasm_qp_sens_wide``).

For ``min 1/2 x'Px + q'x  s.t.  Gx <= h`` at a strictly complementary solution with active rows ``A`` the KKT
conditions are ``P x + q + G_A'y_A = 0``, ``G_A x = h_A``: with ``s = [x; y_A]`` and ``K = [[P, G_A'], [G_A, 0]]``,
``K s = [-q; h_A]``, so every derivative of the solution is a solve with the symmetric ``K``.  With
``[u; w_A] = K^-1 [rx; ry_A]`` and ``w = 0`` off the active set:

- adjoint, ``rx = dL/dx``, ``ry = dL/dy``: ``dL/dq = -u``, ``dL/dh = w``, ``dL/dP = -1/2 (u x' + x u')`` (with respect to
  a symmetric ``P``), row ``i`` of ``dL/dG`` ``= -(y_i u' + w_i x')`` on active rows and 0 elsewhere;
- forward, ``rx = -(dq + dP x + dG_A'y_A)``, ``ry = dh - dG x``: ``dx = u``, ``dy = w``.

The steps of include/mpcasm.h, per instance:

1. skipped: ``status`` given and not SOLVED, or the guessed active set has more rows than unknowns.
2. active set: row i iff ``h_i - z_i < y_i`` (the polish's test; always the fp64 comparison of the inputs).
3. solve: ``r = [rx; ry_A]``, ``dK = diag(delta I, -delta I)``; ``t = (K + dK)^-1 r``, then ``refine_iters`` times
   ``t += (K + dK)^-1 (r - K t)``, factored and refined the way tests/polish_restatement.py does (block elimination,
   two Cholesky factorisations, plain loops in the chosen number format); a pivot that is not positive: singular.
4. results: ``u = t[:no]``, ``w = t[no:]`` scattered, ``lres = |r - K t|_inf`` after the last refinement.
"""
import collections

import numpy as np

from helpers import LD
from osqp_restatement import SOLVED, _rel
from polish_restatement import DELTA, REFINE, _backward, _forward, _inf, cholesky

DONE, SKIPPED, SINGULAR = 1, 0, -1

Sens = collections.namedtuple("Sens", "u w verdict lres active margin")


def active_set(h, y, z):
    """``(active, margin)``: the polish's test in fp64 and the relative distance of its nearest row from a tie."""
    h, y, z = (np.asarray(v, dtype=np.float64).ravel() for v in (h, y, z))
    with np.errstate(invalid="ignore"):
        slack = h - z
        active = slack < y
    ties = [_rel(a, b) for a, b in zip(slack, y) if np.isfinite(a) and np.isfinite(b)]
    return active, min(ties, default=np.inf)


def sens(P, G, h, x, y, z, rx, ry, status=None, delta=DELTA, refine_iters=REFINE, dtype=np.float64):
    """One instance, the steps above, the solve in ``dtype``.  A :class:`Sens`: ``u, w`` (None unless DONE),
    ``verdict``, ``lres``, ``active`` (None when skipped by status) and the active-set ``margin``."""
    if status is not None and int(status) != SOLVED:
        return Sens(None, None, SKIPPED, None, None, np.inf)
    hq = np.asarray(h, dtype=np.float64).ravel()
    no, nc = np.asarray(x).size, hq.size
    active, margin = active_set(hq, y, z)
    na = int(active.sum())
    if na > no:
        return Sens(None, None, SKIPPED, None, active, margin)
    c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
    Pd, Gd = c(P), c(G).reshape(nc, no)
    r1, r2 = c(rx).ravel(), c(ry).ravel()[active]
    GA = Gd[active]
    dl = dtype(delta)
    L = cholesky(Pd + dl * np.eye(no, dtype=dtype), dtype)
    if L is None:
        return Sens(None, None, SINGULAR, None, active, margin)
    V = _backward(L, _forward(L, GA.T)) if na else np.zeros((no, 0), dtype=dtype)     # (P + delta I)^-1 G_A'
    Ls = cholesky(GA @ V + dl * np.eye(na, dtype=dtype), dtype)
    if Ls is None:
        return Sens(None, None, SINGULAR, None, active, margin)

    def solve(a1, a2):
        a = _backward(L, _forward(L, a1))
        ya = _backward(Ls, _forward(Ls, GA @ a - a2))
        return a - V @ ya, ya

    residual = lambda tx, ty: (r1 - Pd @ tx - GA.T @ ty, r2 - GA @ tx)
    tx, ty = solve(r1, r2)
    for _ in range(refine_iters):
        dx, dy = solve(*residual(tx, ty))
        tx, ty = tx + dx, ty + dy
    e1, e2 = residual(tx, ty)
    w = np.zeros(nc, dtype=dtype)
    w[active] = ty
    return Sens(tx, w, DONE, max(_inf(e1), _inf(e2)), active, margin)


def exact(P, G, h, x, y, z, rx, ry, status=None, delta=DELTA):
    """:func:`sens` in long double, refined until the residual against ``K`` stops falling: ``K^-1 r`` to long-double
    rounding (at most 50 steps; each divides the error by about ``1 / (delta |K^-1|)``)."""
    best = sens(P, G, h, x, y, z, rx, ry, status, delta, 0, LD)
    if best.verdict != DONE:
        return best
    for iters in range(1, 51):
        out = sens(P, G, h, x, y, z, rx, ry, status, delta, iters, LD)
        if not out.lres < best.lres:
            break
        best = out
    return best


def kkt_residual(P, G, active, u, w, rx, ry):
    """``|r - K t|_inf`` in long double of ``t = [u; w_A]``, and the magnitude its rounding scales with,
    ``max_i (|K||t| + |r|)_i``; ``K`` from the given active set."""
    c = lambda a: np.asarray(a, dtype=np.float64).astype(LD)
    P, u, w, rx, ry = c(P), c(u).ravel(), c(w).ravel(), c(rx).ravel(), c(ry).ravel()
    G = c(G).reshape(len(active), P.shape[0])
    GA, wa = G[active], w[active]
    e1, e2 = rx - P @ u - GA.T @ wa, ry[active] - GA @ u
    m1 = np.abs(P) @ np.abs(u) + np.abs(GA).T @ np.abs(wa) + np.abs(rx)
    m2 = np.abs(GA) @ np.abs(u) + np.abs(ry[active])
    top = lambda *vs: max(float(v.max(initial=LD(0))) for v in vs)
    return top(np.abs(e1), np.abs(e2)), top(m1, m2)


def gradients(u, w, x, y, active):
    """``(gq, gh, gP, gG)`` of the adjoint in the arrays' own format (long double in, long double out)."""
    u, w, x, y = (np.asarray(v).ravel() for v in (u, w, x, y))
    gP = -(np.outer(u, x) + np.outer(x, u)) / 2
    gG = -(np.outer(y, u) + np.outer(w, x))
    gG[~np.asarray(active, dtype=bool)] = 0
    return -u, w, gP, gG


def jvp_rhs(x, y, active, dq, dh, dP=None, dG=None):
    """``(rx, ry)`` of the forward derivative along ``(dq, dh, dP, dG)``, in the arrays' own format."""
    ya = np.where(active, y, 0)
    rx, ry = -np.asarray(dq), np.array(dh)
    if dP is not None:
        rx = rx - dP @ x
    if dG is not None:
        rx, ry = rx - dG.T @ ya, ry - dG @ x
    return rx, ry
