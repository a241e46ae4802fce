"""Instances the soft-limit tests pose  --  TEST INFRASTRUCTURE ONLY (test_gpu_qp_soft.py,
test_gpu_qp_soft_wide.py)."""
import collections

import numpy as np

import osqp_restatement as rs
import soft_restatement as ss
from oracle import admm_oracle as ao

MARGIN = 1e-6
TOL = 1e-10


def penalties(rng, nc, hard=()):
    """A row of per-instance penalties mixing hard and soft rows: about a third hard (and those of ``hard``), the
    others with ``lin`` in [0.05, 5] and ``quad`` 0 on every other soft row, else in [0, 2]."""
    lin = rng.uniform(0.05, 5.0, nc)
    quad = rng.uniform(0.0, 2.0, nc)
    quad[::2] = 0.0
    lin[rng.random(nc) < 1.0 / 3.0] = np.inf
    lin[list(hard)] = np.inf
    return lin, quad


def mixed_batch(no, nc, seed):
    """Five solvable instances, a contradicting pair kept hard among soft rows, the same pair soft (where there are
    two rows), a dual-infeasible instance and one with an indefinite ``P``, in one batch of one shape, each with
    penalties of its own: ``P, q, G, h, lin, quad`` stacked."""
    rng = np.random.default_rng(seed)
    qps = [rs.random_qp(rng, no, nc) + penalties(rng, nc) for _ in range(5)]
    if nc >= 2:
        pair = rs.primal_infeasible_qp(rng, no, nc)
        qps.append(pair + penalties(rng, nc, hard=(0, 1)))
        lin, quad = penalties(rng, nc)
        lin[:2] = (3.0, 0.5)
        qps.append(pair + (lin, quad))
    qps.append(rs.dual_infeasible_qp(rng, no, nc) + penalties(rng, nc))
    P, q, G, h = rs.random_qp(rng, no, nc)
    qps.append((-50.0 * np.eye(no), q, G, h) + penalties(rng, nc))
    return [np.stack(a) for a in zip(*qps)]


# offsets from no * 1000 + nc at which every instance of the mixed batch is :func:`well_posed`.  What this selection
# EXCLUDES: a dual-infeasible instance that changes rho (unless it lands on a clip) -- it runs off along a direction
# no row limits, its primal residual is rounding, and most seeds have it change rho on that residual.  The mixed
# batches therefore never cover the adaptive step of a dual-infeasible instance away from the clips.
SEED_OFFSETS = {(36, 76): 2, (65, 70): 2, (96, 196): 1, (129, 40): 3, (12, 257): 10}


def seed(no, nc):
    return no * 1000 + nc + SEED_OFFSETS.get((no, nc), 0)


Ref = collections.namedtuple("Ref", rs.Solution._fields + ("rho_amp", "rho_path"))
RHO_AMP_TOL = 1e-3


def _unclipped_rho(rho, norms):
    rp, sp, rd, sd = norms
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(rho * np.sqrt(np.float64(rp / (sp + 1e-30)) / np.float64(rd / (sd + 1e-30))))


def solve(P, q, G, h, lin, quad, **kw):
    """soft_restatement.solve with ``rho_path``, every rho the solve iterated with, and ``rho_amp``, how much a
    relative error of the iterate is amplified in the final rho.  A new rho is rho sqrt((r_p / s_p) / (r_d / s_d)),
    and a residual is a difference that has cancelled down to r / s of its scale, so an iterate off by ``tol`` of its
    scale moves the new rho by about tol (s_p / r_p + s_d / r_d) / 2 of itself; the changes of one solve multiply,
    their relative errors add.  One kind of change adds nothing: a residual within the rounding of its own sum,
    r <= (no + nc) u s, that sends rho to a clip (1e-6, 1e6) even at that bound -- whatever rounding makes of it,
    both arithmetics take the clip itself.
    What this is for: at a residual that is rounding (r / s ~ 1e-14: the dual residual of a cold start's first
    check, the primal residual after a hundred iterations at rho = 1e6) the new rho is rounding's to pick, and two
    arithmetics part ways from there.  Measured in numpy alone, (5, 9) at lin = 1e4: rho goes 0.1 -> 1e6 (clipped,
    from r_d = 9e-16) -> 0.57 from r_p = 1.9e-14 of 0.49; np.linalg.solve against an explicit inverse moves that r_p
    by 0.3 %, the device by more, and x follows the last rho at 3e-3 of itself per unit of d rho / rho -- the
    3.8e-5 of |x| once seen between device and numpy there.  With the rho path held fixed the two numpy arithmetics
    stay within 4e-13 of each other through the clip, and a 2e-16 nudge of z at rho = 1e6 moves the final x by
    3e-12."""
    rec = []
    sol = ss.solve(P, q, G, h, lin, quad, rho_record=rec, **kw)
    path, amp = [float(kw.get("rho", ao.RHO))], 0.0
    nu = (np.shape(P)[0] + np.shape(G)[0]) * 2.0 ** -53
    for norms in rec:
        rp, sp, rd, sd = norms
        up = rd <= nu * sd and _unclipped_rho(path[-1], (rp, sp, nu * sd, sd)) >= rs.RHO_MAX
        down = rp <= nu * sp and _unclipped_rho(path[-1], (nu * sp, sp, rd, sd)) <= rs.RHO_MIN
        path.append(rs.new_rho(path[-1], norms))
        if not (up or down):
            with np.errstate(divide="ignore"):
                amp += float(0.5 * (np.float64(sp) / rp + np.float64(sd) / rd))
    return Ref(*sol, amp, tuple(path))


def well_posed(ref):
    """Whether device and restatement can be held to each other on this instance: every decision far from a tie, and
    every change of rho resting on residuals that stand clear of rounding -- TOL rho_amp within RHO_AMP_TOL, TOL being
    how far two arithmetics' iterates are apart at best.  (The soft fleet from rest: 1e-7 .. 3e-4 on the walker-ticks
    that pass, 2e-3 .. 2e2 on those that do not.)"""
    return ref.margin > MARGIN and TOL * ref.rho_amp <= RHO_AMP_TOL


def expected(P, q, G, h, lin, quad, **kw):
    """Every instance's :class:`Ref`, each asserted :func:`well_posed` (else: pick another seed)."""
    out = [solve(P[b], q[b], G[b], h[b], lin[b], quad[b], **kw) for b in range(P.shape[0])]
    for b, s in enumerate(out):
        assert s.margin > MARGIN, "instance %d decides within %.1e of a tie: pick another" % (b, s.margin)
        assert well_posed(s), "instance %d picks a rho from residuals at rounding level: pick another" % b
    return out


def tolerance(P, G, ref):
    """test_gpu_qp_solve.py's: the kernel applies an explicit K^-1, the restatement solves with K -- they differ by
    rounding times K's condition."""
    if ref.status == rs.NON_CVX:
        return TOL
    K = P + ao.SIGMA * np.eye(P.shape[0]) + ref.rho * G.T @ G
    return max(TOL, 1e-14 * np.linalg.cond(K))


def assert_matches(sol, ref, b, what="", tol=TOL, P=None, G=None):
    """test_gpu_qp_solve.py's ``assert_matches``, check for check and bound for bound, but for rho where it has
    moved (below) and for the absolute slack of the two residuals.  Every instance passed in must be
    :func:`well_posed` (asserted): none is compared on less than status, iterations, rho, x, y, z and residuals.
    The residuals are differences of sums of |P| |x|-, |G| |x|- and |z|-sized terms, which the kernel adds in another
    order than numpy: each carries up to (no + nc) u times that size (the bound of an inner product of
    that length).  Where the iterate is of order one that is below the 1e-12 the hard test allows; a dual-infeasible
    instance whose soft rows let rho fall to 1e-6 runs off to |x| ~ 1e5 before it is called, and its primal
    residual is that rounding alone: 6.98e-10 on the device against 5.82e-10 in numpy at (36, 76)."""
    from helpers import assert_close

    assert not hasattr(ref, "rho_amp") or well_posed(ref), (what, b, "not well posed: pick another instance")
    assert int(sol.status[b]) == ref.status, (what, b, int(sol.status[b]), ref.status)
    assert int(sol.iters[b]) == ref.iters, (what, b, int(sol.iters[b]), ref.iters)
    # (rho: 1e-9 as there, or what the iterate's own bound allows it, see :func:`solve`)
    rtol = max(1e-9, tol * getattr(ref, "rho_amp", 0.0))
    assert np.isclose(float(sol.rho[b]), ref.rho, rtol=rtol, atol=0), (what, b, float(sol.rho[b]), ref.rho, rtol)
    if ref.status == rs.NON_CVX:
        for t in (sol.x, sol.y, sol.z, sol.res):
            assert bool(t[b].isnan().all())
        return
    assert_close(sol.x[b].cpu().numpy(), ref.x, tol, "%s x[%d]" % (what, b))
    ydev = sol.y[b].cpu().numpy()
    yscale = max(np.abs(ref.y).max(initial=0.0), ref.rho * np.abs(ref.z).max(initial=0.0))
    assert np.abs(ydev - ref.y).max(initial=0.0) <= tol * yscale, "%s y[%d]" % (what, b)
    assert_close(sol.z[b].cpu().numpy(), ref.z, tol, "%s z[%d]" % (what, b))
    size = np.abs(ref.z).max(initial=0.0)
    for M in (P, G):
        if M is not None and M.size:
            size = max(size, np.abs(M).sum(axis=1).max() * np.abs(ref.x).max())
    if G is not None and G.size:
        size = max(size, np.abs(G).sum(axis=0).max() * np.abs(ref.y).max(initial=0.0))
    n = (0 if P is None else P.shape[0]) + (0 if G is None else G.shape[0])
    # (and x, z themselves are only known to tol of their size)
    slack = max(1e-12, n * 2.0 ** -53 * size, tol * size)
    assert np.allclose(sol.res[b].cpu().numpy(), ref.res, rtol=1e-6, atol=slack), (what, b, sol.res[b], ref.res, slack)
