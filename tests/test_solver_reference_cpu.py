"""tests/solver_reference.py pinned on the CPU: its long-double inverse against 50-digit arithmetic, its fp64
iteration against oracle/admm_oracle.py, and -- for every input tests/test_gpu_solver_precision.py gives the
kernels -- the plain fp64 restatement against the bounds the kernels are held to: a correct implementation in
another order of summation must sit at half of each at the most, or the input or the derivation is wrong."""
import numpy as np
import pytest

import solver_reference as sr
from helpers import LD, assert_close
from oracle import admm_oracle as ao
from test_gpu_admm import random_qps


def _mpf(mp, v):
    """A long double as an mpf, exactly (two doubles)."""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))


@pytest.mark.parametrize("target", sr.TARGETS, ids=["k1e1", "k1e5", "k1e9"])
def test_the_inverse_against_fifty_digits(target):
    """no = 12: max |X* - X_mp| <= no eps_LD kappa2 |X_mp|_2."""
    import mpmath

    no, nc, rho = 12, 5, 0.1
    P, q, G, h, K, X, kappa = sr.conditioned_qp(np.random.default_rng(12), no, nc, target, rho, details=True)
    with mpmath.workdps(50):
        Kmp = mpmath.matrix(no, no)
        for i in range(no):
            for j in range(no):
                Kmp[i, j] = _mpf(mpmath, K[max(i, j), min(i, j)])       # (the lower triangle, as inverse reads it)
        Xmp = mpmath.inverse(Kmp)
        err = max(abs(_mpf(mpmath, X[i, j]) - Xmp[i, j]) for i in range(no) for j in range(no))
        X64 = np.array([[float(Xmp[i, j]) for j in range(no)] for i in range(no)])
        bound = no * sr.EPS_LD * kappa * sr.norm2(X64)
        print("inverse vs mpmath: kappa2 %.3g, error %.3g, bound %.3g" % (kappa, float(err), bound))
        assert float(err) <= bound


@pytest.mark.parametrize("no,nc", [(36, 76), (5, 3), (70, 10), (64, 65), (33, 200), (7, 0)],
                         ids=["biped", "tiny", "wide", "edge", "tall", "free"])
def test_the_fp64_iteration_against_the_oracle(no, nc):
    """tests/test_gpu_admm.py's six shapes, 40 iterations: the two differ by the solve only (an explicit
    inverse against LAPACK's LU on well-conditioned K): 1e-12 block-relative."""
    P, q, G, h = random_qps(np.random.default_rng(no * 1000 + nc), 3, no, nc)
    for b in range(3):
        X = sr.cholesky_inverse(sr.form_k(P[b], G[b], 1.0, ao.SIGMA, np.float64), np.float64)
        x, y, z = sr.iterate(P[b], q[b], G[b], h[b], X, 1.0, iters=40, dtype=np.float64)
        xo, yo, zo, _ = ao.admm(P[b], q[b], G[b], h[b], iters=40, rho=1.0)
        assert_close(x, xo, 1e-12, "x"), assert_close(y, yo, 1e-12, "y"), assert_close(z, zo, 1e-12, "z")


def _res_ratios(qp, x, y, z):
    no, nc = qp[0].shape[0], qp[2].shape[0]
    rp, rd, Mp, Md = sr.residuals(*qp[:3], x, y, z)
    bp, bd = sr.res_bounds(no, nc, Mp, Md)
    gp, gd = sr.fp64_residuals(*qp[:3], x, y, z)
    return sr.ratio(abs(gp - float(rp)), bp), sr.ratio(abs(gd - float(rd)), bd), float(max(rp, rd))


@pytest.mark.parametrize("c", sr.cases(), ids=sr.case_id)
def test_the_fp64_restatement_sits_at_half_of_every_bound(c):
    """The inverse (a), one step (b) and the residuals (d: after 40 steps, after 65 and, well conditioned, at
    the converged iterate) of the plain fp64 restatement on the GPU tests' own inputs."""
    cs = sr.case(*c)
    worst = {}
    for b in range(sr.INSTANCES):
        qp = cs.qp(b)
        got = {"inverse": sr.ratio(sr.err_inf(cs.X64[b], cs.X[b]), sr.inverse_bound(cs.no, cs.kappa[b], cs.X[b]))}
        xs, ys, zs, rs, zrs = cs.ref_step(b)
        bx, by, bz = sr.step_bounds(qp[2], qp[3], cs.y0[b], cs.rho, cs.kappa[b], cs.X[b], rs, zrs)
        x1, y1, z1, _ = cs.fp64_step(b)
        got["dx"], got["dy"], got["dz"] = (sr.ratio(sr.err_inf(x1, xs), bx), sr.ratio(sr.err_inf(y1, ys), by),
                                           sr.ratio(sr.err_inf(z1, zs), bz))
        for name, it in zip(("40", "65"), cs.iterates(b, np.float64)):
            got["res_p " + name], got["res_d " + name], _ = _res_ratios(qp, *it)
        if cs.target == sr.TARGETS[0] and (cs.no, cs.nc) not in sr.SLOW:
            x, y, z = cs.iterates(b, np.float64)[1]
            for _ in range(sr.CONVERGE_ROUNDS):
                x, y, z = sr.iterate(*qp, cs.X64[b], cs.rho, iters=sr.CONVERGE_ITERS, dtype=np.float64, x=x, y=y, z=z)
                got["res_p conv"], got["res_d conv"], res = _res_ratios(qp, x, y, z)
                if res < sr.CONVERGED:
                    break
            assert res < sr.CONVERGED, "instance %d not converged: res %.3g" % (b, res)
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("fp64 restatement / bound, %s (kappa2 %.3g): %s"
          % (sr.case_id(c), max(cs.kappa), ", ".join("%s %.2g" % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= 0.5, "%s: the restatement's %s sits at %.3g of its bound" % (sr.case_id(c), k, v)


@pytest.mark.parametrize("no,nc", sr.DEFICIENT)
def test_the_deficient_inputs_lie_past_the_reach(no, nc):
    """(e)'s premise: kappa2 >= 1e13 for every instance."""
    kappas = sr.deficient_case(no, nc)[4]
    print("deficient %dx%d: kappa2 %s" % (no, nc, ", ".join("%.3g" % k for k in kappas)))
    assert min(kappas) >= 1e13
