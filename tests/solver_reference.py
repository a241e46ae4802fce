"""The QP solvers' iteration restated in long double  --  TEST INFRASTRUCTURE ONLY (no tests here).

mpcasm_admm, mpcasm_qp_solve and mpcasm_qp_solve_wide apply an explicit ``K^-1 = (P + sigma I + rho G'G)^-1``
from an unblocked Cholesky factorisation (factor, invert the factor, multiply).  This module states the same
three steps and the iteration of include/mpcasm.h with plain numpy loops in a chosen number format:

  * in long double (``helpers.LD``), with one Newton step on the inverse, it is the reference ``X*`` and the
    reference iterate: 2^11 times finer than the fp64 the kernels compute in;
  * in float64 it is the "plain fp64 restatement": a correct implementation in the kernels' own format, in
    another order of summation.  It is the yardstick where no sharp a-priori bound is to be had, and the check
    that the a-priori bounds are ones a correct implementation meets (tests/test_solver_reference_cpu.py).

The bounds of tests/test_gpu_solver_precision.py live here too (``inverse_bound``, ``step_bounds``,
``res_bounds``), so that the CPU check and the GPU tests cannot drift apart; so do the inputs (``case``).
"""
import functools

import numpy as np

from helpers import LD, U64

EPS_LD = float(np.finfo(LD).eps)
SIGMA, ALPHA = 1e-6, 1.6          # OSQP's defaults (oracle/admm_oracle.py)
TARGETS = (1e1, 1e5, 1e9)
RHOS = (1e-6, 0.1, 1e6)
INSTANCES = 3
LDS_LIMIT = 156 * 1024            # include/mpcasm.h: what one instance may take on chip


def form_k(P, G, rho, sigma, dtype=LD):
    """``K = P + sigma I + rho G'G`` in ``dtype`` from the fp64 inputs."""
    P, G = np.asarray(P, dtype=np.float64).astype(dtype), np.asarray(G, dtype=np.float64).astype(dtype)
    no = P.shape[0]
    K = P + dtype(sigma) * np.eye(no, dtype=dtype)
    if G.shape[0]:
        K = K + dtype(rho) * (G.T @ G)
    return K


def cholesky_inverse(K, dtype):
    """Unblocked Cholesky of the lower triangle, the factor's inverse by forward substitution, ``T'T``: the
    kernels' three steps in ``dtype``.  ``np.linalg.LinAlgError`` when a pivot is not positive."""
    n = K.shape[0]
    L = np.tril(np.asarray(K).astype(dtype))
    for k in range(n):
        if not L[k, k] > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % k)
        L[k, k] = np.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        col = L[k + 1:, k]
        for j in range(k + 1, n):                         # column j of the trailing block, from the diagonal down
            L[j:, j] -= col[j - k - 1:] * col[j - k - 1]
    T = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        row = -(L[i, :i] @ T[:i, :i + 1]) if i else np.zeros(1, dtype=dtype)
        row[i] += dtype(1)
        T[i, :i + 1] = row / L[i, i]
    return T.T @ T


def inverse(K):
    """``X*``: the three steps in long double, then one Newton step ``X (2I - K X)`` in long double."""
    K = np.asarray(K).astype(LD)
    K = np.tril(K) + np.tril(K, -1).T
    X = cholesky_inverse(K, LD)
    X = X @ (LD(2) * np.eye(K.shape[0], dtype=LD) - K @ X)
    return (X + X.T) / LD(2)


def norm2(A):
    A = np.asarray(A).astype(np.float64)
    return float(np.linalg.norm(A, 2)) if A.size else 0.0


def kappa2(K, X=None):
    """``|K|_2 |X*|_2`` of the fp64-rounded arrays (``X``: ``inverse(K)`` when the caller has it)."""
    return norm2(K) * norm2(inverse(K) if X is None else X)


def step(P, q, G, h, x, y, z, X, rho, sigma=SIGMA, alpha=ALPHA, dtype=LD, full=False):
    """One iteration as include/mpcasm.h states it, applying the given ``X`` for ``K^-1``, in ``dtype``:
    ``x+, y+, z+, r`` with ``r = sigma x - q + G'(rho z - y)`` (``full``: also ``zr = alpha G xt + (1 - alpha) z``).
    ``P`` is not read: ``X`` stands for it."""
    c = lambda a: np.asarray(a).astype(dtype)
    q, G, h, x, y, z, X = c(q).ravel(), c(G), c(h).ravel(), c(x).ravel(), c(y).ravel(), c(z).ravel(), c(X)
    rho, sigma, alpha = dtype(rho), dtype(sigma), dtype(alpha)
    r = sigma * x - q + G.T @ (rho * z - y)
    xt = X @ r
    zt = G @ xt
    xn = alpha * xt + (dtype(1) - alpha) * x
    zr = alpha * zt + (dtype(1) - alpha) * z
    zn = np.minimum(zr + y / rho, h)
    yn = y + rho * (zr - zn)
    return (xn, yn, zn, r, zr) if full else (xn, yn, zn, r)


def cold_start(h, no, dtype=LD):
    h = np.asarray(h).astype(dtype).ravel()
    return np.zeros(no, dtype=dtype), np.zeros(h.size, dtype=dtype), np.minimum(dtype(0), h)


def iterate(P, q, G, h, X, rho, sigma=SIGMA, alpha=ALPHA, iters=40, dtype=LD, x=None, y=None, z=None):
    """``step`` repeated ``iters`` times from ``x, y, z`` (all three) or from the kernels' cold start
    ``x = 0, y = 0, z = min(0, h)``: ``x, y, z``."""
    if x is None:
        x, y, z = cold_start(h, np.asarray(q).size, dtype)
    for _ in range(iters):
        x, y, z, _r = step(P, q, G, h, x, y, z, X, rho, sigma, alpha, dtype)
    return x, y, z


def residuals(P, q, G, x, y, z):
    """``|Gx - z|_inf`` and ``|Px + q + G'y|_inf`` in long double, and the magnitudes their rounding scales with:
    ``Mp = max_i (|G||x| + |z|)_i``, ``Md = max_j (|P||x| + |q| + |G'||y|)_j``."""
    c = lambda a: np.asarray(a, dtype=np.float64).astype(LD)
    P, q, G, x, y, z = c(P), c(q).ravel(), c(G), c(x).ravel(), c(y).ravel(), c(z).ravel()
    top = lambda v: v.max(initial=LD(0))
    rp, rd = top(np.abs(G @ x - z)), top(np.abs(P @ x + q + G.T @ y))
    Mp = top(np.abs(G) @ np.abs(x) + np.abs(z))
    Md = top(np.abs(P) @ np.abs(x) + np.abs(q) + np.abs(G).T @ np.abs(y))
    return rp, rd, Mp, Md


def conditioned_qp(rng, no, nc, target_kappa, rho, sigma=SIGMA, details=False):
    """``P, q, G, h`` whose ``K = P + sigma I + rho G'G`` has 2-norm condition ``target_kappa`` within a factor
    10 (asserted: a premise, like helpers._premise).  ``P = Q diag(logspace) Q'`` with its smallest eigenvalue
    100 sigma at least, so that sigma does not set the condition; ``G`` random, scaled so that ``rho |G|_2^2`` is
    ``P``'s smallest eigenvalue: ``rho G'G`` weighs in where ``K^-1`` is largest and leaves the extremes of the
    spectrum within a factor 2.  ``details``: also ``K``, ``X*`` and the realised condition."""
    lmin = max(1.0 / target_kappa, 100.0 * sigma)
    lam = lmin * np.logspace(np.log10(target_kappa), 0.0, no) if no > 1 else np.array([lmin])
    Q = np.linalg.qr(rng.standard_normal((no, no)))[0]
    P = (Q * lam) @ Q.T
    P = (P + P.T) / 2.0
    G = rng.standard_normal((nc, no))
    gscale = np.sqrt(lmin / rho) / norm2(G) if nc else 1.0
    G = G * gscale
    q = lmin * rng.standard_normal(no)
    h = rng.uniform(0.02, 0.5, nc) * gscale
    K = form_k(P, G, rho, sigma)
    X = inverse(K)
    got, want = kappa2(K, X), target_kappa if no > 1 else 1.0
    assert want / 10.0 <= got <= want * 10.0, "cond(K) %.3g, asked for %.3g" % (got, want)
    return (P, q, G, h, K, X, got) if details else (P, q, G, h)


def deficient_qp(rng, no, nc, rho, sigma=SIGMA, bounded=True):
    """Past the method's reach: ``P`` of rank ``no - 3`` (eigenvalues 1 down to 1e-2, then three zeros), ``G``
    standard normal, not scaled, its rows orthogonal to one of the directions ``P`` lacks -- along it ``K`` is
    ``sigma`` alone, elsewhere up to ``rho |G|_2^2``: 1e14 apart at ``rho = 1e6``.  ``bounded``: ``q`` in the range
    of ``P``, a QP with a solution (else the cost falls without end along what ``P`` lacks).  Returns
    ``P, q, G, h, K, X*, kappa2``."""
    lam = np.concatenate([np.logspace(0.0, -2.0, no - 3), np.zeros(3)])
    Q = np.linalg.qr(rng.standard_normal((no, no)))[0]
    P = (Q * lam) @ Q.T
    P = (P + P.T) / 2.0
    G = rng.standard_normal((nc, no))
    G = G - np.outer(G @ Q[:, -1], Q[:, -1])
    q = rng.standard_normal(no)
    if bounded:
        q = Q[:, :no - 3] @ (Q[:, :no - 3].T @ q)
    h = rng.uniform(0.1, 1.0, nc)
    K = form_k(P, G, rho, sigma)
    X = inverse(K)
    return P, q, G, h, K, X, kappa2(K, X)


def warm_start(rng, G, h, rho):
    """A start for one step: random ``x``; about half the rows active (``z = h``, ``y > 0``, sized so that
    ``y / rho`` is ``h``-sized), the others not (``z < h``, ``y = 0``)."""
    nc, no = G.shape
    x = rng.standard_normal(no)
    active = rng.random(nc) < 0.5
    if nc >= 2:
        active[0], active[1] = True, False
    z = np.where(active, h, h - rng.uniform(0.1, 1.0, nc) * np.abs(h))
    y = np.where(active, rng.uniform(0.1, 1.0, nc) * rho * np.abs(h), 0.0)
    return x, y, z


# --------------------------------------------------------------------------------------------------------
# the bounds
# --------------------------------------------------------------------------------------------------------
def depth(n):
    """The count of roundings in the bounds below: ``n``, the length of the sums, but 5 at least -- forming an
    entry of ``K`` (a product-sum and the sigma), the square root, the reciprocal and the final product are
    roundings whatever the size, each up to ``u``.  It matters for one unknown only, where ``kappa2 = 1`` and
    a bound of ``1 u`` would refuse every fp64 implementation (the restatement sits at 0.8 u there)."""
    return max(n, 5)


def inverse_bound(no, kappa, Xstar):
    """``max |X - X*| <= no u kappa2(K) |X*|_2``: the forward bound of an inverse from a Cholesky factor."""
    return depth(no) * U64 * kappa * norm2(Xstar)


def assert_inverse(X, P, G, rho, sigma=SIGMA, what="K^-1"):
    """A kernel's ``K^-1`` (fp64) within ``inverse_bound`` of ``X*`` for this ``P, G, rho, sigma``."""
    K = form_k(P, G, rho, sigma)
    Xstar = inverse(K)
    err, bound = err_inf(X, Xstar), inverse_bound(K.shape[0], kappa2(K, Xstar), Xstar)
    assert err <= bound, "%s: max |X - X*| %.3e > %.3e" % (what, err, bound)
    return err / bound


def step_bounds(G, h, y, rho, kappa, Xstar, rstar, zrstar):
    """Bounds on ``|dx|_inf, |dy|_inf, |dz|_inf`` of one step against the long-double step with ``X*``:
    ``e = (no + nc) u kappa2 |X*|_2 |r*|_2``, ``Mz = max_i (|zr*_i| + |y_i| / rho + |h_i|)``."""
    nc, no = np.asarray(G).shape
    e = depth(no + nc) * U64 * kappa * norm2(Xstar) * float(np.linalg.norm(np.asarray(rstar).astype(np.float64)))
    mz = np.abs(np.asarray(zrstar).astype(np.float64)) + np.abs(y) / rho + np.abs(h)
    Mz = float(mz.max(initial=0.0))
    bz = 2.0 * norm2(G) * e + 8.0 * U64 * Mz
    return 2.0 * e, rho * bz, bz


def res_bounds(no, nc, Mp, Md):
    return (no + 2) * U64 * float(Mp), (no + nc + 2) * U64 * float(Md)


def ratio(err, bound):
    """``err / bound``; a bound of 0 (no rows) admits an error of 0 only."""
    return err / bound if bound > 0 else (0.0 if err == 0 else np.inf)


def fp64_residuals(P, q, G, x, y, z):
    """The restatement's ``res``: the two norms in plain fp64."""
    return (float(np.abs(G @ x - z).max(initial=0.0)), float(np.abs(P @ x + q + G.T @ y).max(initial=0.0)))


CONVERGE_ITERS, CONVERGE_ROUNDS = 1000, 10   # (d): warm runs from the 65-step iterate of a well-conditioned
                                             # case until res < 1e-10: that many iterations a run, runs at most
CONVERGED = 1e-10
SLOW = [(33, 200)]                # (200 rows on 33 unknowns: the plain iteration needs more than 1e4 steps)


def err_inf(a, ref):
    """``max |a - ref|`` with ``a`` fp64 values and ``ref`` long double (0 for empty arrays)."""
    d = np.abs(np.asarray(a, dtype=np.float64).astype(LD) - np.asarray(ref).astype(LD))
    return float(d.max(initial=LD(0)))


# --------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests, built once per process and never changed
# --------------------------------------------------------------------------------------------------------
LDS_SHAPES = [(63, 5), (64, 65), (65, 3), (96, 1), (7, 0), (33, 200)]
WIDE_SHAPES = [(1, 1), (64, 3), (65, 17), (128, 9), (129, 4), (256, 17), (257, 3), (512, 8)]
SHAPES = LDS_SHAPES + WIDE_SHAPES


def cases():
    """``(no, nc, target, rho)`` of every case: each shape at the three targets, one rho per target, the
    assignment rotated from shape to shape so that every rho meets every target and every path."""
    out = []
    for s, (no, nc) in enumerate(SHAPES):
        for t, target in enumerate(TARGETS):
            out.append((no, nc, target, RHOS[(s + t) % 3]))
    return out


def case_id(c):
    return "%dx%d-k%.0e-rho%g" % c


def lds_doubles(no, nc):
    """Doubles one instance of mpcasm_admm / mpcasm_qp_solve takes on chip (include/mpcasm.h)."""
    m = max(nc, no)
    total = (no + m) * (no | 1) + 8 * no + 4 * nc + 4 * m
    return total + (total & 1)


def wide_doubles(no, nc, onchip):
    total = 3 * nc + 23 * no + 64 + (no * (no | 1) if onchip else 0)
    return total + (total & 1)


def entries(no, nc):
    """The entries that take the shape: the LDS pair where an instance fits on chip, the wide kernel with K^-1
    on chip where that fits, and with K^-1 in d_kinv always."""
    out = []
    if 8 * lds_doubles(no, nc) <= LDS_LIMIT:
        out += ["admm", "solve"]
    if 8 * wide_doubles(no, nc, True) <= LDS_LIMIT:
        out.append("wide-lds")
    return out + ["wide-global"]


class Case:
    """One case: ``INSTANCES`` QPs, their ``K``, ``X*``, condition, the fp64 restatement's inverse, a warm start
    and the reference step from it.  Iterates are computed on demand and kept."""

    def __init__(self, no, nc, target, rho):
        self.no, self.nc, self.target, self.rho, self.sigma, self.alpha = no, nc, target, rho, SIGMA, ALPHA
        rng = np.random.default_rng([no, nc, int(round(np.log10(target))), int(round(np.log10(rho))) + 6])
        qps = [conditioned_qp(rng, no, nc, target, rho, SIGMA, details=True) for _ in range(INSTANCES)]
        self.P, self.q, self.G, self.h = (np.stack(a) for a in list(zip(*qps))[:4])
        self.K, self.X, self.kappa = ([qp[i] for qp in qps] for i in (4, 5, 6))
        self.X64 = [cholesky_inverse(form_k(self.P[b], self.G[b], rho, SIGMA, np.float64), np.float64)
                    for b in range(INSTANCES)]
        starts = [warm_start(rng, self.G[b], self.h[b], rho) for b in range(INSTANCES)]
        self.x0, self.y0, self.z0 = (np.stack(a) for a in zip(*starts))
        self._kept = {}

    def qp(self, b):
        return self.P[b], self.q[b], self.G[b], self.h[b]

    def start(self, b):
        return self.x0[b], self.y0[b], self.z0[b]

    def ref_step(self, b):
        """``x+*, y+*, z+*, r*, zr*`` of the warm start, in long double with ``X*``."""
        key = ("step", b)
        if key not in self._kept:
            self._kept[key] = step(*self.qp(b), *self.start(b), self.X[b], self.rho, full=True)
        return self._kept[key]

    def fp64_step(self, b):
        key = ("step64", b)
        if key not in self._kept:
            self._kept[key] = step(*self.qp(b), *self.start(b), self.X64[b], self.rho, dtype=np.float64)
        return self._kept[key]

    def iterates(self, b, dtype):
        """``[(x, y, z) after 40 steps from the cold start, after 25 more]`` in ``dtype`` (LD: with ``X*``;
        float64: the restatement with its own inverse)."""
        key = ("iter", b, np.dtype(dtype).name)
        if key not in self._kept:
            X = self.X[b] if dtype is LD else self.X64[b]
            first = iterate(*self.qp(b), X, self.rho, iters=40, dtype=dtype)
            self._kept[key] = [first, iterate(*self.qp(b), X, self.rho, iters=25, dtype=dtype, x=first[0],
                                              y=first[1], z=first[2])]
        return self._kept[key]


@functools.lru_cache(maxsize=None)
def case(no, nc, target, rho):
    return Case(no, nc, target, rho)


DEFICIENT = [(64, 2), (129, 4)]     # (e): shapes whose K is built past the explicit inverse's reach, rho = 1e6


@functools.lru_cache(maxsize=None)
def deficient_case(no, nc):
    """``INSTANCES`` QPs of ``deficient_qp`` at ``rho = 1e6`` (two with a solution, one without):
    ``P, q, G, h`` stacked and the list of their ``kappa2``."""
    rng = np.random.default_rng([no, nc, 13])
    qps = [deficient_qp(rng, no, nc, 1e6, bounded=b < 2) for b in range(INSTANCES)]
    return tuple(np.stack(a) for a in list(zip(*qps))[:4]) + ([qp[6] for qp in qps],)
