"""tests/osqp_restatement.py (the numpy restatement of OSQP's solve to tolerance, the checker of
mpcasm_qp_solve) against what a solve must deliver: the KKT conditions of the QP to the tolerance it
claims, scipy's SLSQP on the same QPs, and the infeasibility and iteration-limit verdicts.  osqp itself is
not available: parity with it is not pinned."""
import numpy as np
import pytest
from scipy.optimize import minimize

import osqp_restatement as rs
from mpcasm import problems
from oracle import qp_oracle as orc


def slsqp(P, q, G, h):
    r = minimize(lambda x: 0.5 * x @ P @ x + q @ x, np.zeros(P.shape[0]), jac=lambda x: P @ x + q,
                 constraints=[{"type": "ineq", "fun": lambda x: h - G @ x, "jac": lambda x: -G}],
                 method="SLSQP", options={"maxiter": 500, "ftol": 1e-15})
    assert r.status == 0, r.message
    return r.x


def biped_qps(cpu_api, n, seed=3):
    form = problems.biped(cpu_api, problems.BipedConfig(step_samples=8))
    form.update(step_times=np.array([6, 14]), step_count=0)
    rng = np.random.default_rng(seed)
    for _ in range(n):
        G, h, P, q = orc.assemble(form, rng.normal(0, 0.001, [form.given_len, 1]))
        yield P, q.ravel(), G, h.ravel()


def assert_kkt(P, q, G, h, s, eps_abs, eps_rel):
    """What status 1 claims, restated from the iterate: both residuals within their tolerances; with z
    <= h and y >= 0 (the projection and the multiplier update keep them there), x is eps-feasible and
    eps-stationary, and complementary slackness holds to the same order."""
    x, y, z = s.x, s.y, s.z
    Gx, Px, Gty = G @ x, P @ x, G.T @ y
    inf = lambda v: float(np.abs(v).max(initial=0.0))
    assert inf(Gx - z) <= eps_abs + eps_rel * max(inf(Gx), inf(z))
    assert inf(Px + q + Gty) <= eps_abs + eps_rel * max(inf(Px), inf(Gty), inf(q))
    assert (z <= h).all() and (y >= -1e-12).all()
    assert (Gx - h).max(initial=0.0) <= eps_abs + eps_rel * max(inf(Gx), inf(z))
    # (y_i > 0 only where z_i = h_i: the slack of Gx is within the primal residual there)
    assert np.abs(y * (z - h)).max(initial=0.0) <= 1e-9 * max(1.0, inf(y))


@pytest.mark.parametrize("eps", [1e-3, 1e-5])
def test_the_bipeds_qps_are_solved_and_agree_with_slsqp(cpu_api, eps):
    for P, q, G, h in biped_qps(cpu_api, 3):
        s = rs.solve(P, q, G, h, eps_abs=eps, eps_rel=eps)
        assert s.status == rs.SOLVED and 0 < s.iters < 4000 and s.iters % 25 == 0
        assert_kkt(P, q, G, h, s, eps, eps)
        ref = slsqp(P, q, G, h)
        # (the distance to the solution of a strongly convex QP is bounded by the residuals over the
        # smallest eigenvalue of P; the biped's is of order 1e-2)
        lam = np.linalg.eigvalsh(P).min()
        assert np.abs(s.x - ref).max() <= 10 * max(s.res) / lam + 1e-9
        assert 0.5 * s.x @ P @ s.x + q @ s.x <= 0.5 * ref @ P @ ref + q @ ref + 10 * eps * max(1.0, np.abs(ref).max())


def test_random_qps_are_solved_and_agree_with_slsqp():
    rng = np.random.default_rng(19)
    for no, nc in ((5, 3), (12, 30), (20, 8), (7, 0)):
        P, q, G, h = rs.random_qp(rng, no, nc)
        s = rs.solve(P, q, G, h, eps_abs=1e-6, eps_rel=1e-6)
        assert s.status == rs.SOLVED, s
        assert_kkt(P, q, G, h, s, 1e-6, 1e-6)
        ref = slsqp(P, q, G, h) if nc else np.linalg.solve(P, -q)
        assert np.abs(s.x - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


def test_contradictory_rows_are_primal_infeasible():
    s = rs.solve(np.eye(1), np.zeros(1), np.array([[1.0], [-1.0]]), np.array([-1.0, -1.0]))
    assert s.status == rs.PRIMAL_INFEASIBLE and s.iters > 0
    s = rs.solve(*rs.primal_infeasible_qp(np.random.default_rng(1), 12, 30))
    assert s.status == rs.PRIMAL_INFEASIBLE


def test_a_cost_unbounded_below_is_dual_infeasible():
    # P singular along d = e_0, q'd < 0, no row limits d
    P = np.diag([0.0, 1.0])
    s = rs.solve(P, np.array([-1.0, 0.0]), np.array([[0.0, 1.0]]), np.array([1.0]))
    assert s.status == rs.DUAL_INFEASIBLE and s.iters > 0
    s = rs.solve(*rs.dual_infeasible_qp(np.random.default_rng(1), 12, 30))
    assert s.status == rs.DUAL_INFEASIBLE


def test_too_few_iterations_and_what_does_not_factor(cpu_api):
    P, q, G, h = next(biped_qps(cpu_api, 1))
    s = rs.solve(P, q, G, h, max_iter=40)
    assert s.status == rs.MAX_ITER and s.iters == 40
    s = rs.solve(P, q, G, h, max_iter=0)
    assert s.status == rs.MAX_ITER and s.iters == 0 and not s.x.any()
    # all four eps 0: nothing short of an exact fixed point stops the solve
    s = rs.solve(P, q, G, h, eps_abs=0, eps_rel=0, eps_prim_inf=0, eps_dual_inf=0, max_iter=300)
    assert s.status == rs.MAX_ITER and s.iters == 300
    s = rs.solve(-50.0 * np.eye(36), q, G, h)
    assert s.status == rs.NON_CVX and s.iters == 0 and np.isnan(s.x).all()
    assert rs.solve(P, q, G, h, rho=0.0).status == rs.NON_CVX


def test_adaptive_rho_moves_and_keeps_the_fixed_point(cpu_api):
    """From rho = 1e-4 the biped's solve changes rho; without adaptation it needs far more iterations to
    reach the same tolerance; both land on the same solution."""
    P, q, G, h = next(biped_qps(cpu_api, 1))
    a = rs.solve(P, q, G, h, rho=1e-4, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000)
    b = rs.solve(P, q, G, h, rho=1e-4, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, adaptive_rho_interval=0)
    assert a.status == rs.SOLVED and a.rho_changes >= 1 and a.rho != 1e-4
    assert b.rho == 1e-4 and (b.status == rs.MAX_ITER or b.iters > 2 * a.iters)
    if b.status == rs.SOLVED:
        assert np.abs(a.x - b.x).max() < 1e-3
    # check_every = 1 decides at the first iteration that satisfies the tests
    c = rs.solve(P, q, G, h, check_every=1, adaptive_rho_interval=0)
    d = rs.solve(P, q, G, h, check_every=25, adaptive_rho_interval=0)
    assert c.status == d.status == rs.SOLVED and c.iters <= d.iters and d.iters - c.iters < 25
