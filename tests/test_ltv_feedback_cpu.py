"""CPU: the premises of pre-stabilised prediction (csrc/feedback.hip, ``LtvLoop(feedback=)``), which the GPU test
(test_gpu_ltv_feedback.py) builds on -- the fp64 restatement of the Riccati sweep stays close to the long-double
one on every shape the kernel is run at; the pendulum's closed-loop matrices are stable; and the restated loop at
N = 100 solves with the feedback and is NON_CVX everywhere without it."""
import numpy as np
import pytest

import feedback_restatement as fr
import rollout_cases as rc
from helpers import LD
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
