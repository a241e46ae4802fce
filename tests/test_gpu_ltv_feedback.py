"""GPU: pre-stabilised prediction (csrc/feedback.hip) -- the Riccati sweep ``mpcasm_ltv_lqr``, ``mpcasm_ltv_close``
and ``mpcasm_ltv_true_inputs`` against the long-double restatement (feedback_restatement.py), and the closed loop
``LtvLoop(feedback=)`` at N = 100, where the open loop cannot factor (test_ltv_feedback_cpu.py holds the premises).

Every test prints report lines ``ltv-feedback-precision: ...`` (pytest -s); profiles/ltv_feedback_precision.txt keeps
those of one full run."""
import numpy as np
import pytest

import feedback_restatement as fr
import rollout_cases as rc
from helpers import LD, assert_componentwise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _dev(torch, v):
    return torch.as_tensor(np.array(v, order="C"), device="cuda")      # (a copy: the shared references are read-only)


_references = {}


def _riccati_reference(api, shape):
    """The case and its restatements, once per shape: ``A, B, Q, R``, the long-double ``K*``, and the fp64
    restatement's own error on every instance (in u, relative to each step's largest ``|K*|``)."""
    if shape not in _references:
        A, B, Q, R = fr.riccati_case(api, shape)
        K_ref = np.stack([fr.lqr(A[b], B[b], Q, R, dtype=LD)[0] for b in range(shape[3])])
        own = np.array([fr.gain_errors(fr.lqr(A[b], B[b], Q, R)[0], K_ref[b]).max() for b in range(shape[3])])
        for v in (A, B, Q, R, K_ref, own):
            v.setflags(write=False)
        _references[shape] = (A, B, Q, R, K_ref, own)
    return _references[shape]


@pytest.mark.parametrize("shape", fr.RICCATI_SHAPES, ids=["-".join(map(str, s)) for s in fr.RICCATI_SHAPES])
def test_the_gains_and_the_closed_loop_matrices(gpu_api, torch_gpu, shape):
    """Every step's K within max(8 x the fp64 restatement's own error on that instance, 16 (n + m) u), elementwise,
    relative to the step's largest |K*|: 8 is the margin a kernel gets over its restatement in test_gpu_qp_polish
    (another association, FMA contraction, another order in the small solve), the floor one step's depth.  A_cl
    from the kernel's own K, and ltv_close on it, within (m + 2) u (|A| + |B| |K|) of the long-double A + B K."""
    torch = torch_gpu
    from mpcasm import engine

    n, m, T, batch = shape
    A, B, Q, R, K_ref, own = _riccati_reference(gpu_api, shape)
    Q, R = np.array(Q), np.array(R)         # (copies: the shared references are read-only)
    K, Acl, info = engine.ltv_lqr(_dev(torch, A), _dev(torch, B), Q, R)
    assert K.shape == (batch, T, m, n) and Acl.shape == (batch, T, n, n) and info.shape == (batch,)
    assert info.dtype == torch.int32 and (info == -1).all()
    Kh, Ah = K.cpu().numpy(), Acl.cpu().numpy()
    err = fr.gain_errors(Kh, K_ref)
    bound = np.maximum(8.0 * own, 16.0 * (n + m))
    ratio = (err / bound[:, None, None, None]).max()
    print("ltv-feedback-precision: K, shape %s: worst error %.3g u, restatement's own %.3g u, worst error / bound "
          "%.3g" % (shape, err.max(), own.max(), ratio))
    assert np.isfinite(Kh).all() and ratio <= 1.0, (shape, ratio)
    # A_cl, from the kernel's own K; ltv_close on the same K
    ref, mag = fr.close(A, B, Kh, dtype=LD), fr.close(A, B, Kh, dtype=LD, magnitude=True)
    closed = engine.ltv_close(_dev(torch, A), _dev(torch, B), K).cpu().numpy()
    for what, got in (("ltv_lqr's A_cl", Ah), ("ltv_close", closed)):
        worst = assert_componentwise(got, ref, mag, m + 2, "%s, shape %s" % (what, shape))
        print("ltv-feedback-precision: %s, shape %s: worst %.3g u M (bound %d)" % (what, shape, worst, m + 2))
    # the terminal P and want_closed: P_T = Q is the default, and the gains do not depend on whether A_cl is written
    K2, none, _ = engine.ltv_lqr(_dev(torch, A), _dev(torch, B), Q, R, terminal=Q, want_closed=False)
    assert none is None and torch.equal(K2, K)
    if T > 1:
        K3, _, _ = engine.ltv_lqr(_dev(torch, A), _dev(torch, B), Q, R, terminal=3.0 * Q)
        assert not torch.equal(K3, K)


def test_stride_zero_is_the_same_data_replicated(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine

    n, m, T, batch = 3, 2, 6, 70
    rng = np.random.default_rng(21)
    A1, B1 = rng.standard_normal((T, n, n)), rng.standard_normal((T, n, m))
    Ab, Bb = rng.standard_normal((batch, T, n, n)), rng.standard_normal((batch, T, n, m))
    Q, R = np.eye(n), 0.1 * np.eye(m)
    rep = lambda v: _dev(torch, np.broadcast_to(v, (batch,) + v.shape))
    # the sweep: A shared, B shared, both shared
    for A, B, Ar, Br in ((A1, Bb, rep(A1), None), (Ab, B1, None, rep(B1)), (A1, B1, rep(A1), rep(B1))):
        got = engine.ltv_lqr(_dev(torch, A), _dev(torch, B), Q, R)
        want = engine.ltv_lqr(_dev(torch, A) if Ar is None else Ar, _dev(torch, B) if Br is None else Br, Q, R)
        for g, w in zip(got, want):
            assert torch.equal(g if g.shape == w.shape else g.expand_as(w), w)
    # ltv_close: A, B shared and every form of K
    K1, Ki, Kf = rng.standard_normal((m, n)), rng.standard_normal((batch, m, n)), rng.standard_normal((batch, T, m, n))
    full = lambda K: np.ascontiguousarray(np.broadcast_to(K if K.ndim == 4 else K[..., None, :, :] if K.ndim == 3
                                                          else K[None, None], (batch, T, m, n)))
    for K in (K1, Ki, Kf):
        want = engine.ltv_close(_dev(torch, Ab), _dev(torch, Bb), _dev(torch, full(K)))
        assert torch.equal(engine.ltv_close(_dev(torch, Ab), _dev(torch, Bb), _dev(torch, K)), want)
        shared = engine.ltv_close(_dev(torch, A1), _dev(torch, B1), _dev(torch, K))
        want = engine.ltv_close(rep(A1), rep(B1), _dev(torch, full(K)))
        assert torch.equal(shared if shared.dim() == 4 else shared.expand_as(want), want)
        assert shared.dim() == (3 if K.ndim == 2 else 4)
    ref = fr.close(Ab, Bb, full(Kf), dtype=LD)
    got = engine.ltv_close(_dev(torch, Ab), _dev(torch, Bb), _dev(torch, Kf)).cpu().numpy()
    assert_componentwise(got, ref, fr.close(Ab, Bb, full(Kf), dtype=LD, magnitude=True), m + 2, "ltv_close")


def test_info_names_the_failing_step_and_the_others_are_unaffected(gpu_api, torch_gpu):
    """R = 0 and, for instance 3 of five, B_2 = 0: its S_2 = 0 has no positive pivot."""
    torch = torch_gpu
    from mpcasm import engine

    n, m, T, batch, bad = 3, 2, 5, 5, 3
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((batch, T, n, n)), rng.standard_normal((batch, T, n, m))
    B[bad, 2] = 0.0
    Q, R = np.eye(n), np.zeros((m, m))
    K, Acl, info = engine.ltv_lqr(_dev(torch, A), _dev(torch, B), Q, R)
    assert info.tolist() == [-1, -1, -1, 2, -1]
    assert torch.isnan(K[bad, :3]).all() and torch.isnan(Acl[bad, :3]).all()
    assert torch.isfinite(K[bad, 3:]).all() and torch.isfinite(Acl[bad, 3:]).all()
    rest = [b for b in range(batch) if b != bad]
    K4, Acl4, info4 = engine.ltv_lqr(_dev(torch, A[rest]), _dev(torch, B[rest]), Q, R)
    assert (info4 == -1).all() and torch.equal(K4, K[rest]) and torch.equal(Acl4, Acl[rest])
    assert torch.isfinite(K4).all() and torch.isfinite(Acl4).all()
    # NaN in S is caught by the same test
    B[1, 4, 0, 0] = np.nan
    assert engine.ltv_lqr(_dev(torch, A), _dev(torch, B), Q, R)[2].tolist() == [-1, 4, -1, 2, -1]


def test_the_entries_refuse(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import capi, engine
    from mpcasm.ltv_loop import LtvLoop

    lib = capi.load()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    info = torch.zeros(8, dtype=torch.int32, device="cuda")
    p, ip = buf.data_ptr(), info.data_ptr()
    lqr = lambda n, m, T, batch, A=p, K=p, inf=ip, sa=0: lib.mpcasm_ltv_lqr(n, m, T, batch, A, sa, p, 0, p, p, None, K,
                                                                            None, inf, None)
    assert lqr(5, 1, 2, 1) == capi.ERR_LIMIT and lqr(1, 5, 2, 1) == capi.ERR_LIMIT
    assert lqr(0, 1, 2, 1) == lqr(2, 1, -1, 1) == lqr(2, 1, 2, -1) == lqr(2, 1, 2, 1, sa=-1) == capi.ERR_ARG
    assert lqr(2, 1, 2, 1, A=None) == lqr(2, 1, 2, 1, K=p + 4) == lqr(2, 1, 2, 1, inf=None) == capi.ERR_ARG
    assert lqr(2, 1, 2, 0) == capi.OK
    close = lambda n, m, T, batch, K=p, sk=0: lib.mpcasm_ltv_close(n, m, T, batch, p, 0, p, 0, K, sk, 0, p + 2048, None)
    assert close(5, 1, 2, 1) == close(1, 5, 2, 1) == capi.ERR_LIMIT
    assert close(2, 1, 2, 1, K=None) == close(2, 1, 2, 1, K=p + 2) == close(2, 1, 2, 1, sk=-1) == capi.ERR_ARG
    assert close(2, 1, -2, 1) == capi.ERR_ARG and close(2, 1, 0, 1) == capi.OK
    # the Python layer: sizes, shapes, dtypes
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    for A, B in ((z(3, 5, 5), z(3, 5, 1)), (z(3, 2, 2), z(3, 2, 5)), (z(3, 2, 2), z(4, 2, 1)), (z(2, 2), z(2, 1)),
                 (z(2, 3, 2, 2), z(3, 3, 2, 1)), (z(3, 2, 2).float(), z(3, 2, 1))):
        with pytest.raises(ValueError):
            engine.ltv_lqr(A, B, np.eye(A.shape[-1]), np.eye(B.shape[-1]))
    with pytest.raises(ValueError):
        engine.ltv_lqr(z(3, 2, 2), z(3, 2, 1), np.eye(3), np.eye(1))
    with pytest.raises(ValueError):
        engine.ltv_close(z(3, 2, 2), z(3, 2, 1), z(2, 1))
    with pytest.raises(ValueError):
        engine.ltv_close(z(4, 3, 2, 2), z(3, 2, 1), z(5, 1, 2))
    # the loop: a feedback of the wrong shape, weights without R, a sweep that fails; true_inputs without ltv=
    form, A, B, given = rc.loop_inputs(gpu_api)
    Ad, Bd = _dev(torch, A), _dev(torch, B)
    for feedback in (z(3, 1), z(rc.LOOP_BATCH + 1, 1, 3), z(rc.LOOP_BATCH, rc.LOOP_T - 1, 1, 3), np.zeros((1, 3)),
                     {"Q": np.eye(3)}, {"Q": np.eye(3), "R": np.eye(1), "S": 0}, {"Q": np.eye(3), "R": np.zeros((1, 1)) - 1}):
        with pytest.raises(ValueError):
            LtvLoop(form, "LIP", rc.LOOP_BATCH, Ad, Bd, feedback=feedback)
    plain = engine.Assembler(form, batch=2)
    with pytest.raises(ValueError):
        plain.true_inputs(z(rc.LOOP_T, 1, 3), 0, z(2, plain.ng), z(2, plain.no))
    asm = engine.Assembler(form, batch=2, ltv=["LIP"])
    with pytest.raises(ValueError):
        asm.true_inputs(z(rc.LOOP_T, 1, 3), rc.LOOP_T - rc.LOOP_N + 1, z(2, asm.ng), z(2, asm.no))
    with pytest.raises(ValueError):
        asm.true_inputs(z(rc.LOOP_T, 3, 1), 0, z(2, asm.ng), z(2, asm.no))
    assert lib.mpcasm_ltv_true_inputs(plain._handle, *plain._src_args(), p, 0, p, 2, p, None, p, 2, None) == capi.ERR_ARG
    assert lib.mpcasm_ltv_true_inputs(None, None, None, p, 0, p, 2, p, None, p, 2, None) == capi.ERR_ARG
    assert lib.mpcasm_ltv_true_inputs(asm._handle, *asm._src_args(), p, 0, p, 1, p, None, p, 2, None) == capi.ERR_ARG
    assert lib.mpcasm_ltv_true_inputs(asm._handle, *asm._src_args(), None, 0, p, 2, p, None, p, 2, None) == capi.ERR_ARG


def _true_input_check(torch, asm, plan, K_seq, Acl, B, t, given, optim, index, count, what):
    N, n, m = plan.sweep["N"], plan.sweep["n"], plan.sweep["m"]
    axes = plan.sweep["axes"].shape[0]
    out = torch.full((count, axes, N, m), -7.5, dtype=torch.float64, device="cuda")
    got = asm.true_inputs(K_seq, t, _dev(torch, given), _dev(torch, optim),
                          index=None if index is None else index, out=out, count=count)
    assert got is out
    got, Kh = got.cpu().numpy(), K_seq.cpu().numpy()
    kap, worst = rc.kappa_rollout(N, n, m), 0.0
    for b in range(count):
        row = b if index is None else int(index[b])
        ref = fr.true_inputs(plan, Acl[b, t:t + N], B[b, t:t + N], Kh[b, t:t + N], given[row], optim[b], dtype=LD)
        worst = max(worst, assert_componentwise(got[b], *ref, kap, "%s, instance %d" % (what, b)))
    print("ltv-feedback-precision: true inputs, %s: worst %.3g u M (kappa %d)" % (what, worst, kap))


def test_the_true_inputs(gpu_api, torch_gpu):
    """Every element within kappa_rollout(N, n, m) (u M + 2^-1022) of the long-double restatement, on the closed
    loop the device itself built: lipm_ltv(N = 12) on rollout_cases.loop_inputs at two ticks, and N = 33 with 20
    instances of which 17 run, by an index into 23 rows of given (workgroups of 64 lanes: 34 lanes, two axes)."""
    torch = torch_gpu
    from mpcasm import engine, problems

    Q, R = problems.lipm_feedback_weights()
    form, A, B, given = rc.loop_inputs(gpu_api)
    asm = engine.Assembler(form, batch=rc.LOOP_BATCH, ltv=["LIP"])
    K_seq, Acl_seq, info = engine.ltv_lqr(_dev(torch, A), _dev(torch, B), Q, R)
    assert (info == -1).all()
    optim = np.random.default_rng(8).normal(0.0, 0.1, (rc.LOOP_BATCH, asm.no))
    for t in (0, rc.LOOP_T - rc.LOOP_N):
        asm.bind_ltv_window("LIP", Acl_seq, _dev(torch, B), t)
        _true_input_check(torch, asm, asm.plan, K_seq, Acl_seq.cpu().numpy(), B, t, given, optim, None,
                          rc.LOOP_BATCH, "N = 12, tick %d" % t)
    # one gain sequence and one B sequence for the whole batch (stride 0), A_cl per instance
    shared = K_seq[1].contiguous()
    closed = engine.ltv_close(_dev(torch, A), _dev(torch, B[1]), shared[0].contiguous())
    asm.bind_ltv_window("LIP", closed, _dev(torch, B[1]), 2)
    a = asm.true_inputs(shared, 2, _dev(torch, given), _dev(torch, optim))
    asm.bind_ltv_window("LIP", closed, _dev(torch, np.broadcast_to(B[1], B.shape)), 2)
    b = asm.true_inputs(shared[None].expand(rc.LOOP_BATCH, -1, -1, -1).contiguous(), 2, _dev(torch, given),
                        _dev(torch, optim))
    assert torch.equal(a, b) and a.shape == (rc.LOOP_BATCH, 2, rc.LOOP_N, 1)
    # N = 33, batch 20, count 17, an index into 23 rows
    batch, count, rows, N = 20, 17, 23, 33
    form = problems.lipm_ltv(gpu_api, N=N)
    asm = engine.Assembler(form, batch=batch, ltv=["LIP"])
    seqs = [problems.ltv_lipm_steps(gpu_api, N=N + 2, theta=0.1 * b) for b in range(batch)]
    A, B = np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs])
    rng = np.random.default_rng(12)
    given, optim = rng.normal(0.0, 0.05, (rows, asm.ng)), rng.normal(0.0, 0.1, (batch, asm.no))
    index = rng.permutation(rows)[:batch].astype(np.int32)
    K_seq, Acl_seq, info = engine.ltv_lqr(_dev(torch, A), _dev(torch, B), Q, R)
    asm.bind_ltv_window("LIP", Acl_seq, _dev(torch, B), 1)
    _true_input_check(torch, asm, asm.plan, K_seq, Acl_seq.cpu().numpy(), B, 1, given, optim, index, count,
                      "N = 33, 17 of 20 by index")


def _c5_loop(torch, api, **kw):
    from mpcasm.ltv_loop import LtvLoop

    form, A, B, given = fr.c5_loop_inputs(api)
    loop = LtvLoop(form, "LIP", fr.C5_BATCH, _dev(torch, A), _dev(torch, B), on_unsolved="hold", **kw)
    loop.given.copy_(_dev(torch, given))
    return loop, A, B, given


def _c5_feedback():
    from mpcasm import problems

    Q, R = problems.lipm_feedback_weights()
    return {"Q": Q, "R": R}


def test_the_loop_at_n100_solves_with_feedback(gpu_api, torch_gpu):
    """The inputs of the CPU premise, tick by tick from the device's own solution, as test_gpu_ltv_loop.py: the
    statuses the restatement gives; an applied row of given within kappa_rollout of the long-double first step on
    A_cl_t; a held row bit for bit; u_0 within the true inputs' bound."""
    torch = torch_gpu
    loop, A, B, given0 = _c5_loop(torch, gpu_api, feedback=_c5_feedback())
    assert loop.horizon == fr.C5_N and loop.ticks_possible == fr.C5_T - fr.C5_N + 1
    assert loop.K_seq.shape == (fr.C5_BATCH, fr.C5_T, 1, 3) and loop.A_cl_seq.shape == (fr.C5_BATCH, fr.C5_T, 3, 3)
    plan = loop.asm.plan
    Acl, Kh = loop.A_cl_seq.cpu().numpy(), loop.K_seq.cpu().numpy()
    kap = rc.kappa_rollout(fr.C5_N, 3, 1)
    seen, applied, held = [], 0, 0
    for t in range(fr.C5_TICKS):
        pre = loop.given.cpu().numpy()
        out = loop.step()
        assert set(out) == {"x", "status", "iters", "u"} and out["u"].shape == (fr.C5_BATCH, 2, fr.C5_N, 1)
        x, status, post, u = (v.cpu().numpy() for v in (out["x"], out["status"], loop.given, out["u"]))
        seen.append(status.tolist())
        for b in range(fr.C5_BATCH):
            if rc.applies(int(status[b]), "hold"):
                ref = rc.first_step_reference(plan, Acl[b, t], B[b, t], pre[b], x[b])
                assert_componentwise(post[b], *ref, kap, "tick %d, instance %d" % (t, b))
                applied += 1
            else:
                assert np.array_equal(post[b], pre[b]), (t, b)
                held += 1
            if np.isfinite(x[b]).all():
                ref = fr.true_inputs(plan, Acl[b, t:t + fr.C5_N], B[b, t:t + fr.C5_N], Kh[b, t:t + fr.C5_N], pre[b],
                                     x[b], dtype=LD)
                assert_componentwise(u[b, :, 0], ref[0][:, 0], ref[1][:, 0], kap, "u_0, tick %d, instance %d" % (t, b))
    print("statuses per tick:", seen, "iterations of the last tick:", out["iters"].tolist())
    assert seen == fr.C5_STATUS and applied == 9 and held == 3


def test_the_loop_with_warm_and_polish_and_what_run_records(gpu_api, torch_gpu):
    torch = torch_gpu
    loop, A, B, given0 = _c5_loop(torch, gpu_api, feedback=_c5_feedback(), warm=True, polish=True)
    res = loop.run(fr.C5_TICKS, record=True)
    assert set(res) == {"status", "iters", "polish", "given", "u"}
    assert res["status"].tolist() == fr.C5_STATUS
    assert res["u"].shape == (fr.C5_TICKS, fr.C5_BATCH, 2, 1) and res["u"].dtype == torch.float64
    assert torch.isfinite(res["u"][:, [0, 2, 3]]).all()
    assert torch.equal(res["given"][1:, 1], res["given"][:-1, 1])          # (instance 1 is held)
    # a gain tensor in the dict's place: the same loop (B, T, m, n), bit for bit
    first, _, _, _ = _c5_loop(torch, gpu_api, feedback=_c5_feedback())
    again, _, _, _ = _c5_loop(torch, gpu_api, feedback=first.K_seq)
    assert torch.equal(again.A_cl_seq, first.A_cl_seq)      # (ltv_close sums A + B K in the sweep's own order)
    a, b = first.run(1, record=True), again.run(1, record=True)
    assert a["status"].tolist() == b["status"].tolist() == fr.C5_STATUS[:1]
    assert set(first.run(1)) == {"status", "iters"}
    # one constant gain for all instances and steps, (m, n) and (B, m, n): the loop runs, K_seq is a sequence
    K0 = first.K_seq[0, 0].contiguous()
    for feedback in (K0, K0[None].expand(fr.C5_BATCH, -1, -1).contiguous()):
        const, _, _, _ = _c5_loop(torch, gpu_api, feedback=feedback)
        assert tuple(const.K_seq.shape[-3:]) == (fr.C5_T, 1, 3)
        out = const.step()
        assert out["status"].tolist() == fr.C5_STATUS[0] and torch.isfinite(out["u"][[0, 2, 3]]).all()


def test_without_feedback_nothing_changes_and_nothing_solves(gpu_api, torch_gpu):
    """Why the feature exists: on the open-loop plant the same inputs are NON_CVX at every tick, and every row of
    given is held."""
    torch = torch_gpu
    loop, A, B, given0 = _c5_loop(torch, gpu_api)
    assert loop.K_seq is None
    res = loop.run(fr.C5_TICKS, record=True)
    assert set(res) == {"status", "iters", "given"}
    assert res["status"].tolist() == fr.C5_OPEN_STATUS
    assert torch.equal(res["given"][-1].cpu(), torch.as_tensor(given0))
    explicit, _, _, _ = _c5_loop(torch, gpu_api, feedback=None)
    assert set(explicit.step()) == {"x", "status", "iters"}
