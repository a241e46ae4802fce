"""numpy restatement of OSQP's solution polishing  --  TEST INFRASTRUCTURE ONLY (the checker of
``mpcasm_qp_polish``).

What this pins: the polishing step of the published algorithm (B. Stellato, G. Banjac, P. Goulart,
A. Bemporad, S. Boyd, "OSQP: an operator splitting solver for quadratic programs", Math. Prog. Comp. 12 (2020),
section 4) for the problem the walking loop poses, ``min 1/2 x'Px + q'x  s.t.  Gx <= h`` (l = -inf, u = h),
with ONE stated departure: a polished point with a negative multiplier is rejected.  It does NOT pin parity
with osqp itself, which is not available to the tests.  The five steps of include/mpcasm.h, per instance:

1. skipped: ``status`` given and not SOLVED, or the guessed active set has more rows than unknowns; nothing
   is written.
2. active set: row i iff ``h_i - z_i < y_i``.
3. solve: ``K = [[P, G_A'], [G_A, 0]]``, ``g = [-q; h_A]``, ``dK = diag(delta I, -delta I)``;
   ``t = (K + dK)^-1 g``, then ``refine_iters`` times ``t += (K + dK)^-1 (g - K t)``, the residual from ``K`` as
   it is.  By block elimination with two Cholesky factorisations (``P + delta I`` and the Schur complement
   ``G_A (P + delta I)^-1 G_A' + delta I``), plain loops in the chosen number format; a pivot that is not
   positive: rejected.
4. the point: ``x^ = t[:no]``, ``y^ = t[no:]`` on the active rows and 0 elsewhere, ``z^ = min(G x^, h)``.
5. accept: OSQP's rule on the residuals of the iterate and of the polished point,
   ``(r^_p < r_p and r^_d < r_d) or (r^_p < r_p and r_d < 1e-10) or (r^_d < r_d and r_p < 1e-10)``, AND every
   ``y^_i >= 0``.  Rejected: the iterate comes back as it went in.  A NaN fails every comparison.

``dtype`` is the format of steps 3 to 5: float64 (the "plain fp64 restatement", a correct implementation in the
kernel's own format in another order of summation) or ``helpers.LD``.  The active-set test is always the fp64
comparison of the inputs: it involves no sum, and a device evaluates it to the same bits.

Every comparison the verdict rests on is recorded with its relative distance from a tie, as osqp_restatement
does (``margin``: the smallest over the decisions taken): the active-set tests, the comparisons of the
acceptance rule, and the sign test (the multiplier nearest to zero, relative to the largest).
"""
import collections

import numpy as np

from osqp_restatement import SOLVED, _conj, _rel

DONE, SKIPPED, REJECTED = 1, 0, -1
DELTA, REFINE = 1e-6, 3          # OSQP's defaults
SMALL = 1e-10                    # OSQP's "this residual was already as good as zero"

Polished = collections.namedtuple(
    "Polished", "x y z polish res res_in active margin margins")


def cholesky(K, dtype):
    """Unblocked Cholesky of the lower triangle in ``dtype``; None when a pivot is not positive."""
    n = K.shape[0]
    L = np.tril(np.asarray(K).astype(dtype))
    for k in range(n):
        if not L[k, k] > 0:
            return None
        L[k, k] = np.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        col = L[k + 1:, k]
        for j in range(k + 1, n):
            L[j:, j] -= col[j - k - 1:] * col[j - k - 1]
    return L


def _forward(L, b):
    """``L^-1 b`` (``b``: a vector or a matrix of right-hand sides)."""
    out = np.array(b, dtype=L.dtype)
    for i in range(L.shape[0]):
        out[i] = (out[i] - L[i, :i] @ out[:i]) / L[i, i]
    return out


def _backward(L, b):
    """``L^-T b``."""
    out = np.array(b, dtype=L.dtype)
    for i in range(L.shape[0] - 1, -1, -1):
        out[i] = (out[i] - L[i + 1:, i] @ out[i + 1:]) / L[i, i]
    return out


def _inf(v):
    return v.dtype.type(np.abs(v).max(initial=0))


def residual_norms(P, q, G, x, y, z):
    """``(|Gx - z|_inf, |Px + q + G'y|_inf)`` in the arrays' own format (NaN propagates)."""
    return _inf(G @ x - z), _inf(P @ x + q + G.T @ y)


def _sign_margin(ya):
    """``(every y^ >= 0, distance from flipping)``: holding, the multiplier nearest to zero relative to the
    largest; failing, the most negative one relative to the largest."""
    if ya.size == 0:
        return True, np.inf
    if not np.isfinite(ya.astype(np.float64)).all():
        return False, np.inf
    top = float(np.abs(ya).max())
    if top == 0.0:
        return True, 0.0
    neg = ya < 0
    if neg.any():
        return False, float(np.abs(ya[neg]).max()) / top
    return True, float(np.abs(ya).min()) / top


def _rule(rp, rd, rph, rdh):
    """OSQP's acceptance rule and its distance from flipping: a disjunction holds as firmly as its firmest
    holding term, and fails as narrowly as its nearest failing one."""
    vals = [float(v) for v in (rp, rd, rph, rdh)]
    if not np.isfinite(vals).all():
        return False, np.inf                    # (a NaN or inf fails the comparisons however it is rounded)
    rp, rd, rph, rdh = vals
    terms = [_conj([(rph < rp, rph, rp), (rdh < rd, rdh, rd)]),
             _conj([(rph < rp, rph, rp), (rd < SMALL, rd, SMALL)]),
             _conj([(rdh < rd, rdh, rd), (rp < SMALL, rp, SMALL)])]
    if any(t[0] for t in terms):
        return True, max(t[1] for t in terms if t[0])
    return False, min(t[1] for t in terms)


def polish(P, q, G, h, x, y, z, status=None, delta=DELTA, refine_iters=REFINE, dtype=np.float64):
    """One instance, the steps above.  Returns a :class:`Polished`: ``x, y, z`` (the inputs themselves unless
    DONE), ``polish``, ``res`` = (r^_p, r^_d) when DONE else None, ``res_in`` = (r_p, r_d), ``active`` (bool per
    row, None when skipped by status), ``margin`` and its parts ``margins`` = {"active", "rule", "sign"}."""
    x0, y0, z0 = (np.asarray(v, dtype=np.float64).ravel() for v in (x, y, z))
    hq = np.asarray(h, dtype=np.float64).ravel()
    no, nc = x0.size, hq.size
    margins = {"active": np.inf, "rule": np.inf, "sign": np.inf}
    back = lambda verdict, active, res_in=None: Polished(x0, y0, z0, verdict, None, res_in, active,
                                                         min(margins.values()), dict(margins))
    if status is not None and int(status) != SOLVED:
        return back(SKIPPED, None)
    with np.errstate(invalid="ignore"):
        slack = hq - z0
        active = slack < y0
    ties = [_rel(a, b) for a, b in zip(slack, y0) if np.isfinite(a) and np.isfinite(b)]
    margins["active"] = min(ties, default=np.inf)
    na = int(active.sum())
    if na > no:
        return back(SKIPPED, active)
    c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
    Pd, qd, Gd, hd = c(P), c(q).ravel(), c(G).reshape(nc, no), c(hq)
    xd, yd, zd = c(x0), c(y0), c(z0)
    rp, rd = residual_norms(Pd, qd, Gd, xd, yd, zd)
    GA, hA = Gd[active], hd[active]
    dl = dtype(delta)
    L = cholesky(Pd + dl * np.eye(no, dtype=dtype), dtype)
    if L is None:
        return back(REJECTED, active, (rp, rd))
    V = _backward(L, _forward(L, GA.T)) if na else np.zeros((no, 0), dtype=dtype)     # (P + delta I)^-1 G_A'
    Ls = cholesky(GA @ V + dl * np.eye(na, dtype=dtype), dtype)
    if Ls is None:
        return back(REJECTED, active, (rp, rd))

    def solve(r1, r2):
        a = _backward(L, _forward(L, r1))
        ya = _backward(Ls, _forward(Ls, GA @ a - r2))
        return a - V @ ya, ya

    tx, ty = solve(-qd, hA)
    for _ in range(refine_iters):
        dx, dy = solve(-qd - Pd @ tx - GA.T @ ty, hA - GA @ tx)
        tx, ty = tx + dx, ty + dy
    yh = np.zeros(nc, dtype=dtype)
    yh[active] = ty
    gx = Gd @ tx
    zh = np.minimum(gx, hd)
    rph, rdh = residual_norms(Pd, qd, Gd, tx, yh, zh)
    better, margins["rule"] = _rule(rp, rd, rph, rdh)
    signs, margins["sign"] = _sign_margin(ty)
    if better and signs:
        return Polished(tx, yh, zh, DONE, (rph, rdh), (rp, rd), active, min(margins.values()), dict(margins))
    # rejected: only the tests that failed keep it so -- the verdict is as far from flipping as the farthest
    # of them (and as the active set is from another one)
    failing = max(m for ok, m in ((better, margins["rule"]), (signs, margins["sign"])) if not ok)
    return Polished(x0, y0, z0, REJECTED, None, (rp, rd), active, min(margins["active"], failing), dict(margins))


# ---- instances the tests pose ------------------------------------------------------------------------------
SHAPES = [(5, 3, 0), (5, 3, 2), (7, 12, 7), (36, 76, 20), (65, 70, 33), (33, 100, 33)]     # (no, nc, na)


def complementary_qp(rng, no, nc, na):
    """A strictly convex QP with a chosen, strictly complementary solution: ``P = R'R / no + 0.1 I``, ``x*``
    standard normal, the first ``na`` rows of a random permutation active with multipliers in [0.5, 2], the
    others with slacks in [0.5, 2].  Returns ``P, q, G, h, x*, y*, active``."""
    R = rng.standard_normal((no, no))
    P = R.T @ R / no + 0.1 * np.eye(no)
    P = (P + P.T) / 2.0
    G = rng.standard_normal((nc, no))
    xs = rng.standard_normal(no)
    active = np.zeros(nc, dtype=bool)
    active[rng.permutation(nc)[:na]] = True
    ys = np.where(active, rng.uniform(0.5, 2.0, nc), 0.0)
    slack = np.where(active, 0.0, rng.uniform(0.5, 2.0, nc))
    q = -(P @ xs) - G.T @ ys
    h = G @ xs + slack
    return P, q, G, h, xs, ys, active


def wrong_active_set(h, y, z, active):
    """``y`` with 2 slack added on the first inactive row: the test of step 2 calls it active."""
    i = int(np.flatnonzero(~active)[0])
    out = np.array(y, dtype=np.float64)
    out[i] += 2.0 * (h[i] - z[i])
    return out, i
