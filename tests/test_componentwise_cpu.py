"""CPU: the componentwise check against extended precision (tests/helpers.py: precise_reference,
assert_componentwise) -- the oracle's new dtype / magnitude keywords leave its default results bit for
bit as they were; the fp64 oracle passes the check on every plant the GPU tests use; on C5 the check
rejects damage that the block measure lets through; the kernels' CPU emulators pass it."""
import numpy as np
import pytest

import plan_emulator
from helpers import (LD, RTOL_TIGHT, assert_close, assert_componentwise, cancellation_free_plants, kappa,
                     lti_tracking_problem, precise_reference)
from mpcasm import problems
from mpcasm.plan import _H, compile_plan
from oracle import qp_oracle as orc


def _fp64_oracle(form, name, A, B, given, ltv=False):
    dyn = form.dynamics[name]
    N = dyn.matrices[-1].shape[0]
    saved = list(dyn.matrices)
    try:
        S, U = (orc.extend_matrices_ltv if ltv else orc.extend_matrices)(N, A, B)
        dyn.matrices = list(U) + [S]
        dyn.update_definitions()
        G, h, P, q = orc.assemble(form, np.asarray(given, dtype=float).reshape(-1, 1))
    finally:
        dyn.matrices = saved
        dyn.update_definitions()
    return {"S": S, "U": np.stack(U), "G": G, "h": h.ravel(), "P": P, "q": q.ravel()}


def _check_all(mine, ref, kap, what):
    return {key: assert_componentwise(mine[key], *ref[key], kap, "%s %s" % (what, key))
            for key in mine if key in ref}


def _c5(api):
    """BASELINE config C5 as the issue's table measures it: lipm_ltv(N=100), ltv_lipm_steps(theta=0.3)."""
    N = 100
    form = problems.lipm_ltv(api, N=N)
    A, B = problems.ltv_lipm_steps(api, N=N, theta=0.3)
    given = np.random.default_rng(5).normal(0, 0.05, form.given_len)
    return form, A, B, given, N


def test_default_arguments_are_the_oracle_as_it_was(cpu_api):
    """dtype=float is the default, bit for bit; the magnitude bounds the long-double result everywhere."""
    rng = np.random.default_rng(1)
    form, A, B = lti_tracking_problem(cpu_api, rng, 4, 3, 12, scaled=True, two_axis_limit=True, extra_unknown=True)
    given = rng.normal(0, 0.3, [form.given_len, 1])
    for a, b in zip(orc.assemble(form, given), orc.assemble(form, given, dtype=float, magnitude=False)):
        assert a.dtype == b.dtype == np.float64 and np.array_equal(a, b)
    S0, U0 = orc.extend_matrices(12, A, B)
    S1, U1 = orc.extend_matrices(12, A, B, dtype=float)
    assert np.array_equal(S0, S1) and all(np.array_equal(x, y) for x, y in zip(U0, U1))
    PM0, PM1 = orc.preview_matrices(form), orc.preview_matrices(form, dtype=float)
    optim = rng.normal(0, 0.3, [form.optim_len, 1])
    for var in PM0:
        assert np.array_equal(PM0[var][0], PM1[var][0]) and np.array_equal(PM0[var][1], PM1[var][1])
        assert np.array_equal(orc.preview(PM0, given, optim, var), orc.preview(PM1, given, optim, var, dtype=float))
    form5, A5, B5, g5, N = _c5(cpu_api)
    S0, U0 = orc.extend_matrices_ltv(N, A5, B5)
    S1, U1 = orc.extend_matrices_ltv(N, A5, B5, dtype=float)
    assert np.array_equal(S0, S1) and np.array_equal(U0[0], U1[0])
    # M >= |x*| on every element, and the long double result is long double
    for f, name, (a, b), g, ltv in ((form, "plant", (A, B), given, False), (form5, "LIP", (A5, B5), g5, True)):
        ref = precise_reference(f, name, a, b, g, ltv=ltv)
        for key, (x, mag) in ref.items():
            assert x.dtype == mag.dtype == LD, key
            assert (mag >= np.abs(x)).all(), key


@pytest.mark.parametrize("nx,nu,N,rho,kw", [
    (5, 3, 48, 1.3, {}), (12, 6, 64, 1.25, {}), (4, 2, 100, 1.3, {}), (4, 2, 100, 1e-4, {}),
    (5, 3, 48, 1.3, dict(scaled=True)), (5, 3, 48, 1.3, dict(extra_unknown=True)),
    (5, 3, 48, 1.3, dict(given_input=True)), (5, 3, 48, 1.3, dict(two_axis_limit=True)),
    (4, 1, 9, 1.3, {}), (6, 3, 7, 1.3, {}),
], ids=["5-3-48", "c4-shape", "4-2-100", "4-2-100-underflow", "scaled", "extra-unknown", "given-input",
        "two-axis-limit", "4-1-9", "6-3-7"])
def test_fp64_oracle_passes_on_the_gpu_tests_plants(cpu_api, nx, nu, N, rho, kw):
    rng = np.random.default_rng(nx * 1000 + N)
    A, B = cancellation_free_plants(rng, 1, nx, nu, rho, N)
    form, _, _ = lti_tracking_problem(cpu_api, rng, nx, nu, N, plant=(A[0], B[0]), **kw)
    given = rng.normal(0, 0.3, form.given_len)
    ref = precise_reference(form, "plant", A[0], B[0], given)
    _check_all(_fp64_oracle(form, "plant", A[0], B[0], given), ref, kappa(N, nx), "fp64 oracle")


def test_fp64_oracle_passes_on_per_step_plants_and_c5(cpu_api):
    rng = np.random.default_rng(4100)
    A, B = cancellation_free_plants(rng, 1, 4, 2, 1.3, 100, per_step=True)
    form, _, _ = lti_tracking_problem(cpu_api, rng, 4, 2, 100, plant=(A[0, 0], B[0, 0]), two_axis_limit=True,
                                      scaled=True)
    given = rng.normal(0, 0.3, form.given_len)
    ref = precise_reference(form, "plant", A[0], B[0], given, ltv=True)
    _check_all(_fp64_oracle(form, "plant", A[0], B[0], given, ltv=True), ref, kappa(100, 4), "fp64 oracle")
    form, A, B, given, N = _c5(cpu_api)
    ref = precise_reference(form, "LIP", A, B, given, ltv=True)
    _check_all(_fp64_oracle(form, "LIP", A, B, given, ltv=True), ref, kappa(N, 3), "fp64 oracle, C5")
    # ... and the biped with its pendulum replaced by a growing plant
    conf = problems.BipedConfig(step_samples=8)
    biped = problems.biped(cpu_api, conf)
    biped.update(step_times=np.array([6, 14]), step_count=0)
    A, B = cancellation_free_plants(rng, 1, 3, 1, 1.3, conf.horizon_lenght)
    given = rng.normal(0, 0.1, biped.given_len)
    ref = precise_reference(biped, "LIP", A[0], B[0], given)
    _check_all(_fp64_oracle(biped, "LIP", A[0], B[0], given), ref, kappa(conf.horizon_lenght, 3), "biped")


def test_c5_damage_the_block_measure_lets_through_is_rejected(cpu_api):
    """The issue's table: each damaged fp64 result passes assert_close(..., RTOL_TIGHT) and fails the
    componentwise check."""
    form, A, B, given, N = _c5(cpu_api)
    ref = precise_reference(form, "LIP", A, B, given, ltv=True)
    kap = kappa(N, 3)
    good = _fp64_oracle(form, "LIP", A, B, given, ltv=True)
    _check_all(good, ref, kap, "undamaged")

    def rejected(key, x):
        assert_close(x, ref[key][0].astype(float), RTOL_TIGHT, "block measure, " + key)
        with pytest.raises(AssertionError):
            assert_componentwise(x, *ref[key], kap, key)

    # step N-1 uses B_{N-2}: an off-by-one at the end of the horizon
    Bo = B.copy()
    Bo[N - 1] = B[N - 2]
    off = _fp64_oracle(form, "LIP", A, Bo, given, ltv=True)
    rejected("G", off["G"])
    rejected("P", off["P"])
    # rows 0-19 of G and h rounded to fp32
    G, h = good["G"].copy(), good["h"].copy()
    G[:20], h[:20] = G[:20].astype(np.float32), h[:20].astype(np.float32)
    rejected("G", G)
    rejected("h", h)
    # the elements of P below 1e-6 max|P| rounded to fp32
    P = good["P"].copy()
    small = np.abs(P) < 1e-6 * np.abs(P).max()
    P[small] = P[small].astype(np.float32)
    rejected("P", P)
    # the rows of G of steps 0-4 scaled by (1 + 1e-9): the CoP box holds N rows per facet
    G = good["G"].copy()
    for facet in range(4):
        G[facet * N:facet * N + 5] *= 1 + 1e-9
    rejected("G", G)


@pytest.mark.parametrize("nx,nu,N,rho", [(5, 3, 48, 1.3), (12, 6, 64, 1.25), (4, 2, 100, 1.3)])
def test_tiled_and_scan_emulators_pass(cpu_api, nx, nu, N, rho):
    rng = np.random.default_rng(7 * nx + N)
    A, B = cancellation_free_plants(rng, 1, nx, nu, rho, N)
    form = problems.random_lti(cpu_api, rng, nx=nx, nu=nu, N=N)
    plan = compile_plan(form, lti=["plant"])
    given = rng.normal(0, 0.3, form.given_len)
    ref = precise_reference(form, "plant", A[0], B[0], given)
    kap = kappa(N, nx)
    _check_all(plan_emulator.run_tiled(plan, given, ab=[(A[0], B[0])]), ref, kap, "run_tiled")
    if plan.itab[_H["T_SCAN"]] > 0 and N <= 64:
        _check_all(plan_emulator.run_scan(plan, given, ab=[(A[0], B[0])]), ref, kap, "run_scan")


@pytest.mark.parametrize("nx,nu,N", [(4, 1, 9), (6, 3, 7)])
def test_resident_emulator_passes(cpu_api, nx, nu, N):
    rng = np.random.default_rng(11 * nx + N)
    A, B = cancellation_free_plants(rng, 1, nx, nu, 1.3, N)
    form = problems.random_lti(cpu_api, rng, nx=nx, nu=nu, N=N)
    plan = compile_plan(form, lti=["plant"])
    assert plan.itab[_H["RS_OK"]] == 1
    g = plan.lti[0]
    srcs = [s.array for s in plan.sources]
    srcs[g["ids"][0]], srcs[g["ids"][1]] = A[0], B[0]
    given = rng.normal(0, 0.3, form.given_len)
    ref = precise_reference(form, "plant", A[0], B[0], given)
    _check_all(plan_emulator.run_resident(plan, given, sources=srcs), ref, kappa(N, nx), "run_resident")


def test_sweep_emulator_passes(cpu_api):
    rng = np.random.default_rng(31)
    N = 100
    A, B = cancellation_free_plants(rng, 1, 4, 2, 1.3, N, per_step=True)
    form, _, _ = lti_tracking_problem(cpu_api, rng, 4, 2, N, plant=(A[0, 0], B[0, 0]), scaled=True,
                                      two_axis_limit=True)
    plan = compile_plan(form, ltv=["plant"])
    assert plan.itab[_H["SW_OK"]] == 1
    given = rng.normal(0, 0.3, form.given_len)
    ref = precise_reference(form, "plant", A[0], B[0], given, ltv=True)
    _check_all(plan_emulator.run_sweep(plan, given, A[0], B[0]), ref, kappa(N, 4), "run_sweep")
    form, A, B, given, N = _c5(cpu_api)
    plan = compile_plan(form, ltv=["LIP"])
    ref = precise_reference(form, "LIP", A, B, given, ltv=True)
    _check_all(plan_emulator.run_sweep(plan, given, A, B), ref, kappa(N, 3), "run_sweep, C5")
