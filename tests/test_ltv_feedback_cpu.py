"""CPU: the premises of pre-stabilised prediction (csrc/feedback.hip, ``LtvLoop(feedback=)``), which the GPU test
(test_gpu_ltv_feedback.py) builds on -- the fp64 restatement of the Riccati sweep stays close to the long-double
one on every shape the kernel is run at; the pendulum's closed-loop matrices are stable; and the restated loop at
N = 100 solves with the feedback and is NON_CVX everywhere without it.  And those of
test_gpu_ltv_feedback_variants.py (feedback_cases.py): one step of the restated sweep keeps the residual bounds at
all sixteen (n, m), a later pivot's failure is reported, and the lane and block arithmetic of every case."""
import numpy as np
import pytest

import feedback_cases as fc
import feedback_restatement as fr
import rollout_cases as rc
from helpers import LD, assert_componentwise
from mpcasm import capi, problems
from mpcasm.plan import compile_plan


@pytest.mark.parametrize("shape", fr.RICCATI_SHAPES, ids=["-".join(map(str, s)) for s in fr.RICCATI_SHAPES])
def test_the_fp64_restatement_stays_close_to_long_double(cpu_api, shape):
    """The GPU test's bound is 8 times THIS distance (or a floor of one step's depth), so it has to be small: the
    sweep is a contraction once the loop is closed, but a step's S^-1 and the unstable A_k amplify what P carries.
    Held to 2^13 u -- 40 of fp64's 53 bits are the gains' own -- and recorded: measured 1.0, 4.1, 342, 592 and 44 u on these
    shapes, relative to each step's largest |K*|."""
    n, m, T, batch = shape
    A, B, Q, R = fr.riccati_case(cpu_api, shape)
    assert A.shape == (batch, T, n, n) and B.shape == (batch, T, n, m)
    if shape != (3, 1, 18, 4):
        radius = np.abs(np.linalg.eigvals(A)).max(axis=-1)
        assert radius.min() > 1.3 - 1e-9 and radius.max() < 1.4 + 1e-9
    worst = 0.0
    for b in range(batch):
        K, Acl, info = fr.lqr(A[b], B[b], Q, R)
        K_ref, Acl_ref, info_ref = fr.lqr(A[b], B[b], Q, R, dtype=LD)
        assert info == info_ref == -1 and K_ref.dtype == LD
        assert np.isfinite(K).all() and np.isfinite(Acl).all()
        worst = max(worst, fr.gain_errors(K, K_ref).max())
    print("ltv-feedback-precision: restatement fp64 vs long double, shape %s: worst %.3g u" % (shape, worst))
    assert worst <= 2.0 ** 13, worst


@pytest.mark.parametrize("n,m", fc.NM, ids=["%d-%d" % nm for nm in fc.NM])
def test_one_step_of_the_restatement_stays_within_the_step_bounds(n, m):
    """The premise of test_gpu_ltv_feedback_variants.py's sharp check: on feedback_cases.step_case (T = 2, 70
    instances, a terminal weight that is not Q) the gains of ``fr.lqr`` in fp64 keep the two residual bounds of
    feedback_cases.step_residuals -- (2 n + 3 m + 2) u M at step 1, that plus (2 n + m + 2) u M_P at step 0 -- and
    its ``A_cl`` (m + 2) u (|A| + |B| |K|).  Reached on these inputs, over the sixteen shapes: 0.053 .. 0.23 of the
    bound at step 1 and 0.014 .. 0.13 at step 0, the largest at n = m = 1 -- recorded, the
    constants are the derivation's and are not tightened to them.  A gain with one element off by a part in 10^9
    misses the bound by orders of magnitude."""
    A, B, Q, R, terminal = fc.step_case(n, m)
    assert A.shape == (fc.STEP_BATCH, fc.STEP_T, n, n) and B.shape == (fc.STEP_BATCH, fc.STEP_T, n, m)
    assert fc.true_lanes(fc.STEP_BATCH, 1) == (2, 6)        # (one lane per instance: the second workgroup holds six)
    assert fc.step_constants(n, m) == (2 * n + 3 * m + 2, 2 * n + m + 2)
    assert np.array_equal(terminal, terminal.T) and np.linalg.eigvalsh(terminal).min() > 0
    swept = [fr.lqr(A[b], B[b], Q, R, terminal=terminal) for b in range(fc.STEP_BATCH)]
    assert all(s[2] == -1 for s in swept)
    K, Acl = np.stack([s[0] for s in swept]), np.stack([s[1] for s in swept])
    r1, r0 = fc.step_ratios(A, B, Q, R, terminal, K)
    print("ltv-feedback-variants: restatement, (%d, %d): residual / bound %.3g at step 1, %.3g at step 0" % (n, m, r1, r0))
    assert r1 <= 1.0 and r0 <= 1.0, (r1, r0)
    assert_componentwise(Acl, fr.close(A, B, K, dtype=LD), fr.close(A, B, K, dtype=LD, magnitude=True), m + 2,
                         "the restatement's A_cl, (%d, %d)" % (n, m))
    # the terminal weight is used: the default's gains are others
    assert not np.array_equal(fr.lqr(A[0], B[0], Q, R)[0][1], K[0, 1])
    # what the bound is worth: one element of one gain off by 1e-9 of the step's largest
    for k in range(fc.STEP_T):
        off = K.copy()
        off[3, k, m - 1, n - 1] += 1e-9 * np.abs(K[3, k]).max()
        assert max(fc.step_ratios(A, B, Q, R, terminal, off)) > 1e3, k
    off = K.copy()
    off[3, 0, 0, 0] = np.nan
    assert np.isnan(fc.step_ratios(A, B, Q, R, terminal, off)).all()


@pytest.mark.parametrize("shape", fc.CHAIN_SHAPES, ids=["-".join(map(str, s)) for s in fc.CHAIN_SHAPES])
def test_the_fp64_restatement_stays_close_on_the_other_eleven_chains(shape):
    """test_the_fp64_restatement_stays_close_to_long_double's premise at the (n, m) its five shapes leave out: T =
    7, three instances each."""
    n, m, T, batch = shape
    assert len(fc.CHAIN_SHAPES) == 11 and (n, m) not in {s[:2] for s in fr.RICCATI_SHAPES}
    A, B, Q, R = fr.riccati_case(None, shape)
    worst = 0.0
    for b in range(batch):
        K, _, info = fr.lqr(A[b], B[b], Q, R)
        K_ref, _, info_ref = fr.lqr(A[b], B[b], Q, R, dtype=LD)
        assert info == info_ref == -1
        worst = max(worst, fr.gain_errors(K, K_ref).max())
    print("ltv-feedback-variants: restatement fp64 vs long double, shape %s: worst %.3g u" % (shape, worst))
    assert worst <= 2.0 ** 13, worst


def test_the_lane_arithmetic_of_the_true_input_cases():
    """``lanes = count * axes``, 64 to a workgroup: the workgroups and the last one's lanes every case of
    feedback_cases.TRUE_GEOMETRY claims, the one instance that lies in two workgroups, and where the missing rows'
    instances sit."""
    seen = set()
    for name, axes, counts in fc.TRUE_GEOMETRY:
        assert fc.shape_of(name).axes == axes
        for count, claim in counts.items():
            groups, last = fc.true_lanes(count, axes)
            assert (groups, last) == claim and 1 <= last <= 64 and (groups - 1) * 64 + last == count * axes
            assert fc.straddlers(count, axes) == fc.STRADDLERS.get((name, count), ())
            seen.add((groups > 1, last == 64))
    assert seen == {(False, False), (False, True), (True, False)}       # partial, exactly full, and a second workgroup
    assert sorted(fc.TRUE_GEOMETRY[0][2]) == [31, 32, 33, 70] and sorted(fc.TRUE_GEOMETRY[1][2]) == [64, 65]
    assert sorted(fc.TRUE_GEOMETRY[2][2]) == [16, 17] and sorted(fc.TRUE_GEOMETRY[3][2]) == [21, 22]
    one = fc.shape_of("one-1-1-1")
    assert (one.n, one.m, one.N, one.axes) == (1, 1, 1, 1)
    three = fc.shape_of("three-2-2")
    assert (three.n, three.m, three.N, three.axes) == (2, 2, 5, 3)
    assert [21 * 3 + a for a in range(3)] == [63, 64, 65]               # (instance 21: lane 63, then lanes 0 and 1)
    assert fc.true_lanes(fc.TRUE_BATCH, 2) == (1, 22)
    # the missing rows: -1, rows and 2^31 - 1; instance 31's second axis is the last lane of the first workgroup
    name, batch, count, rows, wild = fc.MISSING
    axes = fc.shape_of(name).axes
    assert sorted(wild.values()) == [-1, rows, 2 ** 31 - 1] and max(wild) < count <= batch
    assert any((b * axes + axes - 1) % 64 == 63 for b in wild) and fc.true_lanes(count, axes)[0] == 2
    assert np.int32(2 ** 31 - 1) == 2 ** 31 - 1


def test_the_block_arithmetic_of_close_and_augment():
    """256 elements to a workgroup: at n = m = 2, T = 4 and 8 instances ``At`` ends exactly on its second workgroup
    and ``Bt``, ``Kt`` on their first; at T = 3 and 7 instances no region ends on one, at any of the six shapes;
    ``ltv_close``'s total is a multiple of 256 at 256 steps for every n and at 21 steps for none."""
    assert fc.AUGMENT_NM == [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (3, 1)]
    T, batch = fc.AUGMENT_SIZES["exact"]
    assert fc.augment_blocks(2, 2, T, batch) == ((512, 256, 256), (2, 1, 1))
    T, batch = fc.AUGMENT_SIZES["ragged"]
    assert fc.augment_blocks(2, 2, T, batch) == ((336, 168, 168), (2, 1, 1))
    for n, m in fc.AUGMENT_NM:
        assert all(t % 256 for t in fc.augment_blocks(n, m, T, batch)[0]), (n, m)
    assert len(fc.CLOSE_NM) == 10 and (1, 2) in fc.CLOSE_NM and (3, 2) not in fc.CLOSE_NM
    for n in range(1, 5):
        total, blocks = fc.close_blocks(n, *fc.CLOSE_SIZES["exact"])
        assert total == 256 * n * n and blocks == n * n
        total, blocks = fc.close_blocks(n, *fc.CLOSE_SIZES["ragged"])
        assert total == 21 * n * n and total % 256 and blocks == total // 256 + 1


@pytest.mark.parametrize("n,m", fc.FAIL_SHAPES)
def test_the_restatement_reports_a_later_pivot(n, m):
    """feedback_cases.failure_case: R = diag(1, .., 1, 0) and the last column of B zero at the failing step -- every
    pivot but the last is positive there (a sweep that tested the first alone would go on), ``info`` names that
    step, it and the earlier ones are NaN, the later ones stand; the other 67 instances go through."""
    A, B, Q, R = fc.failure_case(n, m)
    assert sorted(fc.FAILS) == [5, 64, 69] and sorted(fc.FAILS.values()) == [0, 2, fc.FAIL_T - 1]
    for b in range(fc.FAIL_BATCH):
        K, Acl, info = fr.lqr(A[b], B[b], Q, R)
        assert info == fc.FAILS.get(b, -1), b
        if b not in fc.FAILS:
            assert np.isfinite(K).all() and np.isfinite(Acl).all()
            continue
        assert np.isnan(K[:info + 1]).all() and np.isnan(Acl[:info + 1]).all()
        assert np.isfinite(K[info + 1:]).all() and np.isfinite(Acl[info + 1:]).all()
        # the failing step's S: P as the sweep has it on arrival there
        P = Q
        for k in range(fc.FAIL_T - 1, info, -1):
            P = Q + A[b, k].T @ (P @ Acl[k])
            P = (P + P.T) / 2
        S = R + B[b, info].T @ (P @ B[b, info])
        L, bad = fr.cholesky(S)
        assert bad == m - 1 and (np.diag(L)[:m - 1] > 0).all() and not S[m - 1].any()


def test_the_two_input_loops_first_tick_is_well_posed(cpu_api):
    """feedback_cases.loop_inputs: a plan without limits (nc = 0) on two axes of two inputs each; closed by the
    gains of Q = I, R = I the first window's P is positive definite (its smallest eigenvalue 3e-4 .. 2e-2, the
    largest below 10) and the restated solver calls every instance SOLVED, no verdict near a tie."""
    import osqp_restatement as osqp
    from oracle import qp_oracle as orc

    form, A, B, given = fc.loop_inputs(cpu_api)
    shape = fc.shape_of(fc.LOOP_SHAPE)
    plan = compile_plan(form, ltv=["plant"])
    assert (plan.nc, plan.no, plan.ng) == (0, 2 * shape.m * shape.N, 2 * shape.n)
    assert A.shape == (fc.LOOP_BATCH, shape.N + fc.LOOP_TICKS - 1, shape.n, shape.n)
    dyn, saved = form.dynamics["plant"], list(form.dynamics["plant"].matrices)
    try:
        for b in range(fc.LOOP_BATCH):
            K, Acl, info = fr.lqr(A[b], B[b], np.eye(shape.n), np.eye(shape.m))
            assert info == -1
            S, U = orc.extend_matrices_ltv(shape.N, Acl[:shape.N], B[b, :shape.N])
            dyn.matrices = list(U) + [S]
            dyn.update_definitions()
            P, q = orc.qp_all_costs(form, orc.preview_matrices(form), given[b].reshape(-1, 1), float, False)
            P, q = np.asarray(P, dtype=float), np.asarray(q, dtype=float).ravel()
            eig = np.linalg.eigvalsh((P + P.T) / 2)
            assert 1e-4 < eig.min() and eig.max() < 10.0, (b, eig.min(), eig.max())
            sol = osqp.solve(P, q, np.zeros((0, plan.no)), np.zeros(0))
            assert sol.status == capi.QP_SOLVED and sol.margin >= 0.05, (b, sol.status, sol.margin)
    finally:
        dyn.matrices = saved
        dyn.update_definitions()


def test_the_restatement_reports_the_failing_step():
    """R = 0 and B_2 = 0: S_2 = 0, no positive pivot -- info = 2, steps 0 .. 2 NaN, steps 3 and 4 stand."""
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((5, 3, 3)), rng.standard_normal((5, 3, 2))
    B[2] = 0.0
    for dtype in (float, LD):
        K, Acl, info = fr.lqr(A, B, np.eye(3), np.zeros((2, 2)), dtype=dtype)
        assert info == 2 and np.isnan(K[:3]).all() and np.isnan(Acl[:3]).all()
        assert np.isfinite(K[3:]).all() and np.isfinite(Acl[3:]).all()


def test_the_pendulums_closed_loop_is_stable(cpu_api):
    """Every A_k of the sequence has an eigenvalue near 1.4; with the gains of lipm_feedback_weights every A_cl_k
    at least 5 steps before the sequence's end has a spectral radius below 1 (the last steps' gains still carry
    the terminal P = Q)."""
    form, A, B, given = fr.c5_loop_inputs(cpu_api)
    Q, R = problems.lipm_feedback_weights()
    assert np.abs(np.linalg.eigvals(A)).max(axis=-1).min() > 1.3
    for b in range(fr.C5_BATCH):
        K, Acl, info = fr.lqr(A[b], B[b], Q, R)
        assert info == -1
        np.testing.assert_array_equal(Acl, fr.close(A[b], B[b], K))
        radius = np.abs(np.linalg.eigvals(Acl)).max(axis=-1)
        assert radius[:fr.C5_T - 5].max() < 1.0, radius


def test_the_restated_loop_at_n100_solves_closed_and_cannot_factor_open(cpu_api):
    """The GPU loop test's inputs on the CPU: with the feedback, instance 1 primal infeasible and the others solved
    at every tick, no verdict near a tie; on the open-loop plant every instance NON_CVX at every tick."""
    form, A, B, given = fr.c5_loop_inputs(cpu_api)
    plan = compile_plan(form, ltv=["LIP"])
    Q, R = problems.lipm_feedback_weights()
    Acl = np.stack([fr.lqr(A[b], B[b], Q, R)[1] for b in range(fr.C5_BATCH)])
    status, trail, margin = rc.restated_loop(cpu_api, plan, form, Acl, B, given, ticks=fr.C5_TICKS)
    print("closed: statuses %s, smallest margin %.3g" % (status.tolist(), margin))
    assert status.tolist() == fr.C5_STATUS and margin >= 0.05
    assert np.isfinite(trail).all()
    status, trail, margin = rc.restated_loop(cpu_api, plan, form, A, B, given, ticks=fr.C5_TICKS)
    assert status.tolist() == fr.C5_OPEN_STATUS and capi.QP_NON_CVX == -7
    assert np.array_equal(trail[-1], trail[0])


def test_the_true_inputs_close_the_loop(cpu_api):
    """What `true_inputs` is for: the closed-loop recursion on v and the open-loop recursion on u = K x + v reach
    the same states (the restatement against itself, N = 12)."""
    form, A, B, given = rc.loop_inputs(cpu_api)
    plan = compile_plan(form, ltv=["LIP"])
    sw = plan.sweep
    Q, R = problems.lipm_feedback_weights()
    v = np.random.default_rng(9).normal(0.0, 0.1, plan.no)
    K, Acl, _ = fr.lqr(A[2, :rc.LOOP_N], B[2, :rc.LOOP_N], Q, R)
    u, M = fr.true_inputs(plan, Acl, B[2], K, given[2], v)
    assert u.shape == M.shape == (sw["axes"].shape[0], rc.LOOP_N, 1) and (M >= np.abs(u)).all()
    for a in range(sw["axes"].shape[0]):
        c0 = int(sw["axes"][a, 0])
        x_open, x_closed = given[2, c0:c0 + 3].copy(), given[2, c0:c0 + 3].copy()
        for k in range(rc.LOOP_N):
            x_open = A[2, k] @ x_open + B[2, k] @ u[a, k]
            x_closed = Acl[k] @ x_closed + B[2, k, :, 0] * v[int(sw["axes"][a, 1]) + k]
        np.testing.assert_allclose(x_open, x_closed, rtol=0, atol=1e-9 * np.abs(x_closed).max())


def test_the_entries_refuse_before_any_launch():
    """Sizes and pointers are decided on the host: n or m of 5 is MPCASM_ERR_LIMIT, a null or misaligned pointer or
    a negative size MPCASM_ERR_ARG, an empty batch MPCASM_OK -- none of these reaches the device (the pointers
    below are never read)."""
    lib = capi.load()
    p = 1 << 20
    lqr = lambda n, m, T, batch, A=p, K=p, info=p, sa=0: lib.mpcasm_ltv_lqr(n, m, T, batch, A, sa, p, 0, p, p, None,
                                                                             K, None, info, None)
    assert lqr(5, 1, 2, 1) == lqr(1, 5, 2, 1) == capi.ERR_LIMIT
    assert lqr(0, 1, 2, 1) == lqr(2, 0, 2, 1) == lqr(2, 1, -1, 1) == lqr(2, 1, 2, -1) == capi.ERR_ARG
    assert lqr(2, 1, 2, 1, sa=-1) == lqr(2, 1, 2, 1, A=None) == lqr(2, 1, 2, 1, K=p + 4) == capi.ERR_ARG
    assert lqr(2, 1, 2, 1, info=None) == lqr(2, 1, 2, 1, info=p + 2) == capi.ERR_ARG
    assert lqr(2, 1, 2, 0) == capi.OK
    close = lambda n, m, T, batch, K=p, sk=0, st=0: lib.mpcasm_ltv_close(n, m, T, batch, p, 0, p, 0, K, sk, st, p, None)
    assert close(5, 1, 2, 1) == close(1, 5, 2, 1) == capi.ERR_LIMIT
    assert close(2, 1, 2, 1, K=None) == close(2, 1, 2, 1, K=p + 2) == capi.ERR_ARG
    assert close(2, 1, 2, 1, sk=-1) == close(2, 1, 2, 1, st=-1) == close(2, 1, -2, 1) == capi.ERR_ARG
    assert close(2, 1, 0, 1) == close(2, 1, 2, 0) == capi.OK
    assert lib.mpcasm_ltv_true_inputs(None, None, None, p, 0, p, 2, p, None, p, 2, None) == capi.ERR_ARG
