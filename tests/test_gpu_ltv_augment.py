"""GPU: limits and costs on the true input of a pre-stabilised plan -- ``mpcasm_ltv_augment`` (csrc/feedback.hip)
against long double and, bit for bit, against ``mpcasm_ltv_close`` and the blocks it copies; the assembly of
``problems.lipm_ltv_true_input`` on the matrices the device built, element by element against extended precision;
and ``LtvLoop(feedback=, true_input=True)`` at N = 100 with the limit active (test_ltv_augment_cpu.py holds the
premises).

The tests print report lines ``ltv-augment-precision: ...`` (pytest -s); profiles/ltv_augment_precision.txt keeps those
of one full run."""
import numpy as np
import pytest

import augment_cases as ac
import feedback_restatement as fr
import rollout_cases as rc
from helpers import LD, assert_componentwise, kappa, precise_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _dev(torch, v):
    return torch.as_tensor(np.array(v, order="C"), device="cuda")


def _bits(v):
    return np.ascontiguousarray(v).view(np.int64)


@pytest.mark.parametrize("layout", ac.GAINS + ["shared"])
@pytest.mark.parametrize("shape", ac.SHAPES, ids=["-".join(map(str, s)) for s in ac.SHAPES])
def test_the_kernel_against_long_double_and_what_it_copies(gpu_api, torch_gpu, shape, layout):
    """The A + B K block within (m + 2) u (|A| + |B| |K|) of long double -- mpcasm_ltv_close's own bound -- and
    engine.ltv_close's result bit for bit; every other element the bits of what it copies, of +0.0 or of 1.0.
    ``shared``: one pair of sequences for the batch (a_stride = b_stride = 0) under per-step gains."""
    torch = torch_gpu
    from mpcasm import engine

    n, m, T, batch = shape
    gains = "per-step" if layout == "shared" else layout
    A, B, K = ac.case(shape, gains, shared=layout == "shared")
    Ad, Bd, Kd = _dev(torch, A), _dev(torch, B), _dev(torch, K)
    At, Bt, Kt = engine.ltv_augment(Ad, Bd, Kd)
    assert At.shape == (batch, T, n + m, n + m) and Bt.shape == (batch, T, n + m, m)
    assert Kt.shape == (batch, T, m, n + m)
    At, Bt, Kt = (v.cpu().numpy() for v in (At, Bt, Kt))
    Kf = ac.full_gain(K, T, batch)
    Af, Bf = np.broadcast_to(A, (batch,) + A.shape[-3:]), np.broadcast_to(B, (batch,) + B.shape[-3:])
    closed = At[..., :n, :n]
    worst = assert_componentwise(closed, fr.close(Af, Bf, Kf, dtype=LD), fr.close(Af, Bf, Kf, dtype=LD, magnitude=True),
                                 m + 2, "A + B K, shape %s, %s" % (shape, layout))
    print("ltv-augment-precision: A + B K, shape %s, %s: worst %.3g u M (bound %d)" % (shape, layout, worst, m + 2))
    assert np.array_equal(_bits(closed), _bits(engine.ltv_close(Ad, Bd, Kd).cpu().numpy()))
    want_At, want_Bt, want_Kt = ac.augmented(Af, Bf, Kf)
    At[..., :n, :n] = 0.0
    for what, got, want in (("At", At, want_At), ("Bt", Bt, want_Bt), ("Kt", Kt, want_Kt)):
        assert np.array_equal(_bits(got), _bits(want)), (what, shape, layout)


def test_one_gain_over_shared_sequences_and_a_kt_that_is_not_wanted(gpu_api, torch_gpu):
    """Everything shared: no leading batch, the same numbers as the replicated call.  ``want_gain=False``: None,
    and the entry with d_Kt = NULL writes At and Bt and not a double behind them (a poisoned buffer)."""
    torch = torch_gpu
    from mpcasm import capi, engine

    shape = n, m, T, batch = 2, 2, 5, 67
    A, B, K = ac.case(shape, "one", shared=True)
    one = engine.ltv_augment(_dev(torch, A), _dev(torch, B), _dev(torch, K))
    assert [tuple(v.shape) for v in one] == [(T, 4, 4), (T, 4, 2), (T, 2, 4)]
    rep = lambda v: _dev(torch, np.broadcast_to(v, (batch,) + v.shape))
    many = engine.ltv_augment(rep(A), rep(B), _dev(torch, K))
    for a, b in zip(one, many):
        assert b.shape[0] == batch and torch.equal(a.expand_as(b), b)
    At, Bt, none = engine.ltv_augment(rep(A), rep(B), _dev(torch, K), want_gain=False)
    assert none is None and torch.equal(At, many[0]) and torch.equal(Bt, many[1])
    size_a, size_b, size_k = batch * T * 16, batch * T * 8, batch * T * 8
    buf = torch.full((size_a + size_b + size_k + 512,), -7.5, dtype=torch.float64, device="cuda")
    Ad, Bd, Kd = rep(A), rep(B), _dev(torch, K)
    rc_ = capi.load().mpcasm_ltv_augment(n, m, T, batch, Ad.data_ptr(), T * n * n, Bd.data_ptr(), T * n * m,
                                         Kd.data_ptr(), 0, 0, buf.data_ptr(), buf.data_ptr() + 8 * size_a, None, None)
    assert rc_ == capi.OK
    torch.cuda.synchronize()
    assert torch.equal(buf[:size_a].view(batch, T, 4, 4), many[0])
    assert torch.equal(buf[size_a:size_a + size_b].view(batch, T, 4, 2), many[1])
    assert (buf[size_a + size_b:] == -7.5).all()
    # the Python layer: n + m > 4, and ltv_close's own rules for the gain
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    for A_, B_, K_ in ((z(3, 3, 3), z(3, 3, 2), z(2, 3)), (z(3, 4, 4), z(3, 4, 1), z(1, 4)),
                       (z(3, 2, 2), z(3, 2, 1), z(2, 1)), (z(4, 3, 2, 2), z(3, 2, 1), z(5, 1, 2)),
                       (z(3, 2, 2), z(3, 2, 1), z(2, 4, 1, 2))):
        with pytest.raises(ValueError):
            engine.ltv_augment(A_, B_, K_)


def _instances(api, torch, N, T, batch):
    """The plant's sequences of ``batch`` pendulums, their Riccati gains and the augmented sequences, built on the
    device; host copies of all of them."""
    from mpcasm import engine, problems

    seqs = [problems.ltv_lipm_steps(api, N=T, theta=0.4 * b) for b in range(batch)]
    A, B = np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs])
    Q, R = problems.lipm_feedback_weights()
    K, _, info = engine.ltv_lqr(_dev(torch, A), _dev(torch, B), Q, R, want_closed=False)
    assert (info == -1).all()
    At, Bt, Kt = engine.ltv_augment(_dev(torch, A), _dev(torch, B), K)
    return A, B, K, At, Bt, Kt


@pytest.mark.parametrize("N,batch", [(12, 5), (100, 3)])
def test_the_assembly_on_device_built_matrices(gpu_api, torch_gpu, N, batch):
    """G, h, P, q of lipm_ltv_true_input(input_limit = 0.1) on the sweep kernel, every element within kappa(N, 4)
    (u M + 2^-1022) of helpers.precise_reference on the very fp64 At, Bt the device built: test_gpu_sweep.py's
    depth at n + m states."""
    torch = torch_gpu
    from mpcasm import engine, problems

    form = problems.lipm_ltv_true_input(gpu_api, N=N, input_limit=ac.LOOP_LIMIT)
    asm = engine.Assembler(form, batch=batch, ltv=["LIP"])
    assert (asm.plan.sweep["n"], asm.plan.sweep["m"], asm.no, asm.nc) == (4, 1, 2 * N, 8 * N + 4)
    A, B, K, At, Bt, Kt = _instances(gpu_api, torch, N, N, batch)
    asm.bind_ltv("LIP", At, Bt)
    given = np.random.default_rng(31).normal(0.0, 0.05, (batch, asm.ng))
    results = [v.cpu().numpy() for v in asm.assemble(_dev(torch, given))]
    assert "sweep" in asm.last_kernel(), asm.last_kernel()
    Ah, Bh = At.cpu().numpy(), Bt.cpu().numpy()
    worst = 0.0
    for b in range(batch):
        ref = precise_reference(form, "LIP", Ah[b], Bh[b], given[b], ltv=True)
        for key, x in zip("PqGh", results):
            worst = max(worst, assert_componentwise(x[b], *ref[key], kappa(N, 4), "instance %d %s" % (b, key)))
    print("ltv-augment-precision: assembly, N = %d: worst %.3g u M (kappa %d)" % (N, worst, kappa(N, 4)))


def _feedback():
    from mpcasm import problems

    Q, R = problems.lipm_feedback_weights()
    return {"Q": Q, "R": R}


def _loop(torch, api, **kw):
    from mpcasm.ltv_loop import LtvLoop

    form, A, B, given = ac.loop_inputs(api)
    loop = LtvLoop(form, "LIP", ac.LOOP_BATCH, _dev(torch, A), _dev(torch, B), on_unsolved="hold",
                   feedback=_feedback(), true_input=True, **kw)
    loop.given.copy_(_dev(torch, given))
    return loop, A, B, given


def test_the_loop_at_n100_honours_the_input_limit(gpu_api, torch_gpu):
    """The inputs of the CPU premise, tick by tick from the device's own solution.  Per tick: the statuses of the
    restatement on instances 0, 2, 3; the true inputs within kappa_rollout(N, 4, 1) of long double and, where
    solved, inside the limit (1 + 2 eps); the rollout's rows of cCoP_dot within the same bound of the same
    reference; an applied row of given: its input slots out["u"][:, :, 0] bit for bit, its states within
    kappa_rollout(1, 4, 1) of the long-double A_t x_0 + B_t u_0 on the OPEN-LOOP plant; a held row bit for bit."""
    torch = torch_gpu
    loop, A, B, given0 = _loop(torch, gpu_api)
    N, T = ac.LOOP_N, ac.LOOP_T
    assert loop.horizon == N and loop.ticks_possible == T - N + 1 and loop.true_input
    assert loop.K_seq.shape == (ac.LOOP_BATCH, T, 1, 3) and loop.At_seq.shape == (ac.LOOP_BATCH, T, 4, 4)
    assert loop.Bt_seq.shape == (ac.LOOP_BATCH, T, 4, 1) and loop.Kt_seq.shape == (ac.LOOP_BATCH, T, 1, 4)
    asm, plan = loop.asm, loop.asm.plan
    At, Bt, Kt = (v.cpu().numpy() for v in (loop.At_seq, loop.Bt_seq, loop.Kt_seq))
    kap, kap1 = rc.kappa_rollout(N, 4, 1), rc.kappa_rollout(1, 4, 1)
    bound = ac.LOOP_LIMIT * (1 + ac.LOOP_TOL)
    seen, applied, worst_u = [], 0, 0.0
    for t in range(ac.LOOP_TICKS):
        pre_dev = loop.given.clone()
        pre = pre_dev.cpu().numpy()
        out = loop.step()
        assert set(out) == {"x", "status", "iters", "u"} and out["u"].shape == (ac.LOOP_BATCH, 2, N, 1)
        rows = asm.rollout(pre_dev, out["x"]).cpu().numpy()       # (the window of tick t is still bound)
        x, status, post, u = (v.cpu().numpy() for v in (out["x"], out["status"], loop.given, out["u"]))
        seen.append([int(status[b]) for b in ac.LOOP_ASSERTED])
        print("tick %d: statuses %s, iterations %s, max |u| %s" % (t, status.tolist(), out["iters"].tolist(),
                                                                   np.abs(u).max(axis=(1, 2, 3)).tolist()))
        for b in range(ac.LOOP_BATCH):
            if np.isfinite(x[b]).all():
                ref = fr.true_inputs(plan, At[b, t:t + N], Bt[b, t:t + N], Kt[b, t:t + N], pre[b], x[b], dtype=LD)
                worst_u = max(worst_u, assert_componentwise(u[b], *ref, kap, "u, tick %d, instance %d" % (t, b)))
                for a, axis in enumerate(("_x", "_y")):
                    r0, count = plan.pm_rows["cCoP_dot" + axis]
                    assert count == N
                    assert_componentwise(rows[b, r0:r0 + N], ref[0][a, :, 0], ref[1][a, :, 0], kap,
                                         "rollout's cCoP_dot%s, tick %d, instance %d" % (axis, t, b))
            if status[b] == 1:
                assert np.abs(u[b]).max() <= bound, (t, b, np.abs(u[b]).max())
            if rc.applies(int(status[b]), "hold"):
                applied += 1
                assert np.array_equal(_bits(post[b, [3, 7]]), _bits(u[b, :, 0, 0])), (t, b)
                for a in range(2):
                    x0, u0 = pre[b, 4 * a:4 * a + 3], u[b, a, 0]
                    f, g = (lambda v: np.asarray(v, dtype=LD)), (lambda v: np.abs(np.asarray(v, dtype=LD)))
                    assert_componentwise(post[b, 4 * a:4 * a + 3], f(A[b, t]) @ f(x0) + f(B[b, t]) @ f(u0),
                                         g(A[b, t]) @ g(x0) + g(B[b, t]) @ g(u0), kap1,
                                         "x_1 on the open-loop plant, tick %d, instance %d, axis %d" % (t, b, a))
            else:
                assert np.array_equal(_bits(post[b]), _bits(pre[b])), (t, b)
    print("ltv-augment-precision: true inputs of the loop: worst %.3g u M (kappa %d)" % (worst_u, kap))
    assert seen == ac.LOOP_STATUS and applied >= len(ac.LOOP_ASSERTED) * ac.LOOP_TICKS


def test_true_input_false_is_the_loop_without_the_keyword(gpu_api, torch_gpu):
    """``true_input=False`` beside ``feedback=``: one tick of rollout_cases.loop_inputs (N = 12), bit for bit what
    the same call without the keyword gives."""
    torch = torch_gpu
    from mpcasm.ltv_loop import LtvLoop

    form, A, B, given = rc.loop_inputs(gpu_api)
    results = []
    for kw in ({}, {"true_input": False}):
        loop = LtvLoop(form, "LIP", rc.LOOP_BATCH, _dev(torch, A), _dev(torch, B), feedback=_feedback(), **kw)
        loop.given.copy_(_dev(torch, given))
        out = loop.step()
        assert set(out) == {"x", "status", "iters", "u"} and not loop.true_input
        results.append([out[k].clone() for k in ("x", "status", "iters", "u")] + [loop.given.clone(), loop.A_cl_seq])
    for a, b in zip(*results):
        assert torch.equal(a, b)
    assert results[0][1].tolist() == [rc.LOOP_STATUS[b] for b in range(rc.LOOP_BATCH)]


def test_the_loop_with_warm_and_polish_and_what_run_records(gpu_api, torch_gpu):
    torch = torch_gpu
    cold, _, _, _ = _loop(torch, gpu_api)
    first = cold.step()["status"].tolist()             # (instance 1 is near a tie: not held to anything)
    loop, A, B, given0 = _loop(torch, gpu_api, warm=True, polish=True)
    res = loop.run(ac.LOOP_TICKS, record=True)
    assert set(res) == {"status", "iters", "polish", "given", "u"}
    assert [res["status"][0, b].item() for b in ac.LOOP_ASSERTED] == [first[b] for b in ac.LOOP_ASSERTED] \
        == ac.LOOP_STATUS[0]
    assert res["given"].shape == (ac.LOOP_TICKS + 1, ac.LOOP_BATCH, 8)
    assert res["u"].shape == (ac.LOOP_TICKS, ac.LOOP_BATCH, 2, 1) and res["u"].dtype == torch.float64
    assert torch.isfinite(res["u"][:, list(ac.LOOP_ASSERTED)]).all()
    # a gain tensor in the dict's place: the same augmented sequences, bit for bit
    again = cold
    from mpcasm.ltv_loop import LtvLoop

    form, A, B, given = ac.loop_inputs(gpu_api)
    tensor = LtvLoop(form, "LIP", ac.LOOP_BATCH, _dev(torch, A), _dev(torch, B), feedback=again.K_seq, true_input=True)
    for a, b in ((tensor.At_seq, again.At_seq), (tensor.Bt_seq, again.Bt_seq), (tensor.Kt_seq, again.Kt_seq)):
        assert torch.equal(a, b)
