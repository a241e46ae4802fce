"""numpy restatement of OSQP's solve to tolerance  --  TEST INFRASTRUCTURE ONLY (the checker of
``mpcasm_qp_solve``).

What this pins: the rules of the published algorithm (B. Stellato, G. Banjac, P. Goulart, A. Bemporad,
S. Boyd, "OSQP: an operator splitting solver for quadratic programs", Math. Prog. Comp. 12 (2020):
Algorithm 1, the termination criteria of section 3.4, the infeasibility certificates of section 3.4 and
the adaptive step of section 5.2) with problem scaling off and solution polishing off, for the problem the
walking loop poses, ``min 1/2 x'Px + q'x  s.t.  Gx <= h`` (l = -inf, u = h).  It does NOT pin parity with
osqp itself, which is not available to the tests: osqp picks its adaptive-rho interval from timing, scales
the problem and polishes; here the interval is a fixed argument and the other two are absent.

The iteration is oracle/admm_oracle.py's, called as it is.  After iteration k, when k % check_every == 0 or
k == max_iter, with infinity norms, dx = x_k - x_{k-1} and dy = max(y_k - y_{k-1}, 0) (the projection of the
step of y onto the normal cone of (-inf, h]):

* solved (1):             |Gx - z| <= eps_abs + eps_rel max(|Gx|, |z|)  and
                          |Px + q + G'y| <= eps_abs + eps_rel max(|Px|, |G'y|, |q|)
* primal infeasible (-3): |dy| > 1e-30, h'dy < -eps_prim_inf |dy|, |G'dy| < eps_prim_inf |dy|
* dual infeasible (-4):   |dx| > 1e-30, q'dx < -eps_dual_inf |dx|, |P dx| < eps_dual_inf |dx|,
                          max_i (G dx)_i < eps_dual_inf |dx|

tested in that order; the first that holds ends the solve at k.  None by max_iter: -2 with k = max_iter.
With ``adaptive_rho_interval`` > 0, a check at k % adaptive_rho_interval == 0 that decides nothing and is not
the last iteration computes rho' = rho sqrt((r_p / (scale_p + 1e-30)) / (r_d / (scale_d + 1e-30))), clipped
to [1e-6, 1e6], and takes it when it is more than 5 times off; x, y, z carry over.  A rho <= 0, or a
P + sigma I + rho G'G that is not positive definite (at the start or after a change): -7, NaN iterates.

Every comparison a verdict rests on is recorded with its relative distance from equality (``margin``):
a device whose sums are rounded in another order can only disagree where that distance is of the order of
the rounding, and the tests pick instances far from such ties.
"""
import collections

import numpy as np

from oracle import admm_oracle as ao

SOLVED, MAX_ITER, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE, NON_CVX = 1, -2, -3, -4, -7
RHO_MIN, RHO_MAX = 1e-6, 1e6

Solution = collections.namedtuple("Solution", "x y z status iters res rho margin rho_changes")


def _inf(v):
    return float(np.abs(v).max(initial=0.0))


def _rel(a, b):
    a, b = float(a), float(b)
    if a == b:
        return 0.0
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def _conj(terms):
    """``terms``: (holds, lhs, rhs) in order.  Their conjunction and how far it is from flipping: when it
    holds, the nearest of its terms; when it fails, the farthest of the failing ones (any failing term
    keeps it false)."""
    holds = all(t[0] for t in terms)
    if holds:
        return True, min((_rel(t[1], t[2]) for t in terms), default=np.inf)
    return False, max(_rel(t[1], t[2]) for t in terms if not t[0])


def _factor_ok(P, G, rho, sigma):
    try:
        np.linalg.cholesky(P + sigma * np.eye(P.shape[0]) + rho * (G.T @ G))
        return True
    except np.linalg.LinAlgError:
        return False


def check(P, q, G, h, x, y, z, x_prev, y_prev, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf):
    """The three tests at one iterate: ``(status or 0, (r_p, scale_p, r_d, scale_d), margin)``."""
    Gx, Px, Gty = G @ x, P @ x, G.T @ y
    rp, sp = _inf(Gx - z), max(_inf(Gx), _inf(z))
    rd, sd = _inf(Px + q + Gty), max(_inf(Px), _inf(Gty), _inf(q))
    norms = (rp, sp, rd, sd)
    margins = []
    tp, td = eps_abs + eps_rel * sp, eps_abs + eps_rel * sd
    solved, m = _conj([(rp <= tp, rp, tp), (rd <= td, rd, td)])
    margins.append(m)
    if solved:
        return SOLVED, norms, min(margins)
    dy = np.maximum(y - y_prev, 0.0)
    ndy, hdy, ngdy = _inf(dy), float(h @ dy), _inf(G.T @ dy)
    pinf, m = _conj([(ndy > 1e-30, ndy, 1e-30), (hdy < -eps_prim_inf * ndy, hdy, -eps_prim_inf * ndy),
                     (ngdy < eps_prim_inf * ndy, ngdy, eps_prim_inf * ndy)])
    margins.append(m)
    if pinf:
        return PRIMAL_INFEASIBLE, norms, min(margins)
    dx = x - x_prev
    ndx, qdx, npdx = _inf(dx), float(q @ dx), _inf(P @ dx)
    mgdx = float((G @ dx).max(initial=-np.inf))
    dinf, m = _conj([(ndx > 1e-30, ndx, 1e-30), (qdx < -eps_dual_inf * ndx, qdx, -eps_dual_inf * ndx),
                     (npdx < eps_dual_inf * ndx, npdx, eps_dual_inf * ndx),
                     (mgdx < eps_dual_inf * ndx, mgdx, eps_dual_inf * ndx)])
    margins.append(m)
    return (DUAL_INFEASIBLE if dinf else 0), norms, min(margins)


def new_rho(rho, norms):
    """OSQP's step for the residuals ``norms`` = (r_p, scale_p, r_d, scale_d), clipped; NaN stays NaN."""
    rp, sp, rd, sd = norms
    with np.errstate(divide="ignore", invalid="ignore"):
        rn = float(rho * np.sqrt(np.float64(rp / (sp + 1e-30)) / np.float64(rd / (sd + 1e-30))))
    return RHO_MIN if rn < RHO_MIN else RHO_MAX if rn > RHO_MAX else rn


def solve(P, q, G, h, x=None, y=None, z=None, rho=ao.RHO, sigma=ao.SIGMA, alpha=ao.ALPHA, eps_abs=1e-3,
          eps_rel=1e-3, eps_prim_inf=1e-4, eps_dual_inf=1e-4, max_iter=4000, check_every=25,
          adaptive_rho_interval=100):
    """One QP, the rules above.  Start: ``x, y, z`` (all three) or cold (x = 0, y = 0, z = min(0, h)).
    Returns a :class:`Solution`: the iterate, ``status``, ``iters``, ``res`` = (|Gx - z|, |Px + q + G'y|)
    of the iterate, the final ``rho``, the smallest ``margin`` of any decision taken on the way and the
    number of changes of rho."""
    P, G = np.asarray(P, dtype=np.float64), np.asarray(G, dtype=np.float64)
    q, h = np.asarray(q, dtype=np.float64).ravel(), np.asarray(h, dtype=np.float64).ravel()
    no, nc = P.shape[0], G.shape[0]
    assert check_every >= 1 and max_iter >= 0 and adaptive_rho_interval >= 0
    assert adaptive_rho_interval % check_every == 0
    if x is None:
        x, y, z = np.zeros(no), np.zeros(nc), np.minimum(0.0, h)
    else:
        x, y, z = (np.array(v, dtype=np.float64).ravel() for v in (x, y, z))
    rho = float(rho)
    nan = lambda n: np.full(n, np.nan)
    if not (rho > 0.0) or not _factor_ok(P, G, rho, sigma):
        return Solution(nan(no), nan(nc), nan(nc), NON_CVX, 0, (np.nan, np.nan), rho, np.inf, 0)
    margin, changes, k, status = np.inf, 0, 0, MAX_ITER
    while k < max_iter:
        nxt = min((k // check_every + 1) * check_every, max_iter)
        if nxt - k > 1:
            x, y, z, _ = ao.admm(P, q, G, h, x, y, z, iters=nxt - k - 1, rho=rho, sigma=sigma, alpha=alpha)
        x_prev, y_prev = x, y
        x, y, z, _ = ao.admm(P, q, G, h, x, y, z, iters=1, rho=rho, sigma=sigma, alpha=alpha)
        k = nxt
        verdict, norms, m = check(P, q, G, h, x, y, z, x_prev, y_prev, eps_abs, eps_rel, eps_prim_inf,
                                  eps_dual_inf)
        margin = min(margin, m)
        if verdict:
            status = verdict
            break
        if adaptive_rho_interval > 0 and k % adaptive_rho_interval == 0 and k < max_iter:
            rn = new_rho(rho, norms)
            up, down = rn > 5.0 * rho, rn < rho / 5.0
            if up or down:
                margin = min(margin, max(_rel(rn, 5.0 * rho) if up else 0.0, _rel(rn, rho / 5.0) if down else 0.0))
            elif rn == rn:
                margin = min(margin, _rel(rn, 5.0 * rho), _rel(rn, rho / 5.0))
            if up or down:
                rho, changes = rn, changes + 1
                if not _factor_ok(P, G, rho, sigma):
                    return Solution(nan(no), nan(nc), nan(nc), NON_CVX, k, (np.nan, np.nan), rho, margin, changes)
    return Solution(x, y, z, status, k, ao.residuals(P, q, G, x, y, z), rho, margin, changes)


# ---- instances the tests pose ------------------------------------------------------------------------------
def random_qp(rng, no, nc):
    """Strictly convex, x = 0 strictly feasible: solvable."""
    R = rng.standard_normal((no + 3, no))
    return (R.T @ R + 0.1 * np.eye(no), rng.standard_normal(no), rng.standard_normal((nc, no)),
            rng.uniform(0.1, 1.0, nc))


def primal_infeasible_qp(rng, no, nc):
    """Rows 0 and 1 contradict each other: x_0 <= -1 and -x_0 <= -1 (nc >= 2)."""
    P, q, G, h = random_qp(rng, no, nc)
    G[0], G[1] = 0.0, 0.0
    G[0, 0], G[1, 0], h[0], h[1] = 1.0, -1.0, -1.0, -1.0
    return P, q, G, h


def dual_infeasible_qp(rng, no, nc):
    """Unbounded below: P singular along d, q'd < 0, every row falling along d (G d < 0: no row limits d, and
    rho G'G keeps P + sigma I + rho G'G well conditioned along d; without rows it is sigma there)."""
    P, q, G, h = random_qp(rng, no, nc)
    d = rng.standard_normal(no)
    d /= np.linalg.norm(d)
    Pr = np.eye(no) - np.outer(d, d)
    P = Pr @ P @ Pr
    G = G @ Pr - np.outer(rng.uniform(0.5, 1.0, nc), d)
    q = q - (q @ d + 1.0) * d            # q'd = -1
    return P, q, G, h
