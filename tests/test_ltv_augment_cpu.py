"""CPU: the premises of limits and costs on the true input of a pre-stabilised plan (``mpcasm_ltv_augment``,
``problems.lipm_ltv_true_input``, ``LtvLoop(feedback=, true_input=True)``), which the GPU test
(test_gpu_ltv_augment.py) builds on -- the QP of the formulation on the augmented plant is the QP a dense
construction from the plant gives; the plan compiles onto the sweep back end, which a limit on the input VARIABLE
of ``lipm_ltv`` does not; the restated loop at N = 100 solves with the limit active and honoured; and the entries
refuse on the host."""
import numpy as np
import pytest

import augment_cases as ac
import feedback_restatement as fr
import rollout_cases as rc
from mpcasm import capi, problems
from mpcasm.plan import compile_plan


def _block_error(x, ref):
    return float(np.abs(np.asarray(x) - ref).max() / np.abs(ref).max())


def test_augment_matrices_blocks():
    """problems.augment_matrices against the block-by-block restatement, over leading axes and a broadcast gain."""
    A, B, K = ac.case((2, 2, 5, 67), "per-instance")
    At, Bt = problems.augment_matrices(A, B, K[:, None])
    want_A, want_B, _ = ac.augmented(A, B, K[:, None])
    want_A[..., :2, :2] = A + B @ K[:, None]
    assert At.shape == (67, 5, 4, 4) and Bt.shape == (67, 5, 4, 2)
    assert np.array_equal(At, want_A) and np.array_equal(Bt, want_B)
    assert not np.signbit(At[..., 2:]).any() and not np.signbit(Bt[..., 2:, :]).any()


@pytest.mark.parametrize("N", [12, 100])
def test_the_qp_on_the_augmented_plant_is_the_qp_on_the_true_input(cpu_api, N):
    """The premise: the oracle's assembly of lipm_ltv_true_input on augment_matrices of every instance's window
    against the dense construction from the plant (augment_cases.dense_true_input_qp: no augmentation, the effort
    term w U^T U with U = K X + I) -- the limit's rows of G and h, and P and q, to 1e-12 of each block's largest
    element.  The input slots of `given` hold anything finite: they have no influence."""
    form, A, B, given = ac.loop_inputs(cpu_api, N=N, T=N + 4)
    K = ac.loop_gains(A, B)
    given[:, 3], given[:, 7] = 0.37, -12.5
    worst = {}
    for b in range(ac.LOOP_BATCH):
        for t in (0, 4):
            At, Bt = problems.augment_matrices(A[b, t:t + N], B[b, t:t + N], K[b, t:t + N])
            P, q, G, h = rc.window_qp(form, "LIP", At, Bt, given[b])
            assert P.shape == (2 * N, 2 * N) and G.shape == (8 * N + 4, 2 * N)
            ref = ac.dense_true_input_qp(A[b, t:t + N], B[b, t:t + N], K[b, t:t + N], given[b],
                                         input_limit=ac.LOOP_LIMIT)
            for key, got, want in zip("PqGh", (P, q, G[:4 * N], h[:4 * N]), ref):
                worst[key] = max(worst.get(key, 0.0), _block_error(got, want))
    print("N = %d: worst block errors %s" % (N, {k: "%.2e" % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1e-12, worst


def test_the_plan_compiles_onto_the_sweep_tables_and_the_input_variable_still_does_not(cpu_api):
    form = problems.lipm_ltv_true_input(cpu_api, N=ac.LOOP_N, input_limit=ac.LOOP_LIMIT)
    assert form.optim_variables == ["v_x", "v_y"] and form.given_len == 8
    plan = compile_plan(form, ltv=["LIP"])
    sw = plan.sweep
    assert (sw["n"], sw["m"], sw["N"], sw["axes"].shape[0]) == (4, 1, ac.LOOP_N, 2)
    assert (plan.no, plan.nc, plan.ng) == (200, 804, 8)
    assert compile_plan(problems.lipm_ltv_true_input(cpu_api, N=ac.LOOP_N), ltv=["LIP"]).nc == 404
    # the nominal matrices have the structure LtvLoop(true_input=True) asks for
    mats = form.dynamics["LIP"].matrices
    assert np.all(mats[-1][0].T[:, 3:] == 0) and np.array_equal(mats[0][0, 0, :], [*mats[0][0, 0, :3], 1.0])
    with pytest.raises(ValueError):
        problems.lipm_ltv_true_input(cpu_api, N=12, gain=np.zeros((3, 1)))
    # the gap, recorded: a limit on the input VARIABLE of lipm_ltv is no fixed combination of one step's states
    plain = problems.lipm_ltv(cpu_api, N=12)
    plain.incorporate_constraint("input limit", [cpu_api.Constraint("cCoP_dot_x", ac.LOOP_LIMIT)])
    plain.make_preview_matrices()
    with pytest.raises(ValueError, match="no fixed combination of one step's states"):
        compile_plan(plain, ltv=["LIP"])


def test_the_restated_loop_at_n100_honours_the_limit(cpu_api):
    """The GPU loop test's inputs on the CPU (rollout_cases.restated_loop on the augmented form and sequences):
    instances 0, 2, 3 SOLVED at every tick, no verdict near a tie, every true input of the trail within the limit
    (1 + 2 eps); the unlimited plan exceeds 0.12 on each of them at tick 0.  Instance 1 runs out of iterations with
    a margin below 0.05: its first tick is reported, not asserted."""
    import osqp_restatement as osqp

    form, A, B, given = ac.loop_inputs(cpu_api)
    plan = compile_plan(form, ltv=["LIP"])
    K = ac.loop_gains(A, B)
    At, Bt = problems.augment_matrices(A, B, K)
    idx, N = list(ac.LOOP_ASSERTED), ac.LOOP_N
    status, trail, margin = rc.restated_loop(cpu_api, plan, form, At[idx], Bt[idx], given[idx], ticks=ac.LOOP_TICKS)
    print("limited: statuses %s, smallest margin %.3g" % (status.tolist(), margin))
    assert status.tolist() == ac.LOOP_STATUS and margin >= 0.05
    bound = ac.LOOP_LIMIT * (1 + ac.LOOP_TOL)
    applied = np.abs(trail[1:][:, :, [3, 7]])          # (the input slots: u_0 of every tick's plan)
    assert applied.max() <= bound, applied.max()
    # every input of the first plan, limited and not
    free = problems.lipm_ltv_true_input(cpu_api, N=N)
    for b in ac.LOOP_ASSERTED:
        peak = []
        for f in (form, free):
            sol = osqp.solve(*rc.window_qp(f, "LIP", At[b, :N], Bt[b, :N], given[b]))
            assert sol.status == capi.QP_SOLVED
            u, _ = ac.plan_inputs(plan, At[b, :N], Bt[b, :N], K[b, :N], given[b], sol.x)
            peak.append(np.abs(u).max())
        print("instance %d: max |u| of the first plan %.4f with the limit, %.4f without" % (b, *peak))
        assert peak[0] <= bound and peak[1] > ac.LOOP_UNLIMITED_EXCEEDS
    sol = osqp.solve(*rc.window_qp(form, "LIP", At[1, :N], Bt[1, :N], given[1]))
    print("instance 1 (reported): status %d, margin %.3g" % (sol.status, sol.margin))
    if sol.margin >= 0.05:            # (measured 0.027: should the margin ever be a safe one, the verdict holds)
        assert sol.status == capi.QP_MAX_ITER


def test_the_entry_refuses_before_any_launch():
    """Decided on the host, the pointers below never read: n + m > 4 or n, m not in 1 .. 4 is MPCASM_ERR_LIMIT; a
    null (Kt excepted) or misaligned pointer, a negative size or stride MPCASM_ERR_ARG; T == 0 or batch == 0 OK."""
    lib = capi.load()
    p = 1 << 20

    def augment(n, m, T, batch, A=p, B=p, K=p, At=p, Bt=p, Kt=p, sa=0, sb=0, sk=0, st=0):
        return lib.mpcasm_ltv_augment(n, m, T, batch, A, sa, B, sb, K, sk, st, At, Bt, Kt, None)

    assert augment(5, 1, 2, 1) == augment(1, 5, 2, 1) == augment(0, 1, 2, 1) == augment(1, 0, 2, 1) == capi.ERR_LIMIT
    assert augment(4, 1, 2, 1) == augment(3, 2, 2, 1) == augment(2, 3, 2, 1) == augment(1, 4, 2, 1) == capi.ERR_LIMIT
    assert augment(-1, 1, 2, 1) == augment(3, 1, -2, 1) == augment(3, 1, 2, -1) == capi.ERR_ARG
    assert augment(3, 1, 2, 1, sa=-1) == augment(3, 1, 2, 1, sb=-1) == capi.ERR_ARG
    assert augment(3, 1, 2, 1, sk=-1) == augment(3, 1, 2, 1, st=-3) == capi.ERR_ARG
    for name in ("A", "B", "K", "At", "Bt"):
        assert augment(3, 1, 2, 1, **{name: None}) == augment(3, 1, 2, 1, **{name: p + 4}) == capi.ERR_ARG
    assert augment(3, 1, 2, 1, Kt=p + 2) == capi.ERR_ARG
    assert augment(3, 1, 0, 1) == augment(3, 1, 2, 0) == augment(2, 2, 0, 0, Kt=None) == capi.OK


def test_the_loop_refuses_on_the_host(cpu_api):
    """LtvLoop(true_input=True): without feedback; on a formulation whose states are not the plant's and its
    inputs; on one whose nominal matrices are not an augmented plant's -- before anything is compiled."""
    from mpcasm.ltv_loop import LtvLoop

    A, B = np.zeros((16, 3, 3)), np.zeros((16, 3, 1))
    K = np.zeros((1, 3))
    good = problems.lipm_ltv_true_input(cpu_api, N=12)
    with pytest.raises(ValueError, match="feedback"):
        LtvLoop(good, "LIP", 2, A, B, true_input=True)
    with pytest.raises(ValueError, match="3 states"):
        LtvLoop(problems.lipm_ltv(cpu_api, N=12), "LIP", 2, A, B, feedback=K, true_input=True)
    with pytest.raises(ValueError, match="4 states"):
        LtvLoop(good, "LIP", 2, np.zeros((16, 2, 2)), np.zeros((16, 2, 1)), feedback=K, true_input=True)
    # four states and one input, but not [x ; u_prev]
    axes = ["_x", "_y"]
    rng = np.random.default_rng(2)
    system = cpu_api.ControlSystem(["v"], ["a", "b", "c", "d"], rng.standard_normal((4, 4)),
                                   rng.standard_normal((4, 1)), axes)
    form = cpu_api.Formulation()
    form.incorporate_dynamics("LIP", cpu_api.ExtendedSystem.from_cotrol_system(system, "x", 12))
    form.incorporate_goal("effort", cpu_api.Cost("d", 1.0, aim=[0, 0], axes=axes))
    form.identify_qp_domain(["v_x", "v_y"])
    form.make_preview_matrices()
    with pytest.raises(ValueError, match="'LIP'"):
        LtvLoop(form, "LIP", 2, A, B, feedback=K, true_input=True)
    # zero columns alone are not enough: the last row of B must be the identity's
    At, Bt = problems.augment_matrices(rng.standard_normal((3, 3)), rng.standard_normal((3, 1)), K)
    Bt[3, 0] = 2.0
    system = cpu_api.ControlSystem(["v"], ["a", "b", "c", "d"], At, Bt, axes)
    form = cpu_api.Formulation()
    form.incorporate_dynamics("LIP", cpu_api.ExtendedSystem.from_cotrol_system(system, "x", 12))
    form.incorporate_goal("effort", cpu_api.Cost("d", 1.0, aim=[0, 0], axes=axes))
    form.identify_qp_domain(["v_x", "v_y"])
    form.make_preview_matrices()
    with pytest.raises(ValueError, match="identity"):
        LtvLoop(form, "LIP", 2, A, B, feedback=K, true_input=True)
