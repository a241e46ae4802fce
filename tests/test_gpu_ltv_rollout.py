"""GPU: the forward rollout of a plan compiled with ``ltv=`` (csrc/rollout.hip: ``Assembler.rollout``,
``Assembler.advance``, ``Assembler.bind_ltv_window``) against extended precision.  Every shape of
rollout_cases.GPU_SHAPES -- every instance its own per-step plant, initial state and solution -- into NaN-filled
buffers: the rows within ``kappa_rollout (u M + 2^-1022)`` of the oracle in long double on the very fp64 inputs,
the copies of ``given`` and ``optim`` bit for bit, nothing written past ``count``; rows by index; a plant shared
by the batch (stride 0); the goals' distances from the rows; the next ``given`` in place, by index, under a status
mask; the refusals; and the window of a longer sequence bound by pointer."""
import numpy as np
import pytest

import preview_cases as pc
import rollout_cases as rc
import sweep_cases as sc
from helpers import LD, assert_componentwise

pytestmark = pytest.mark.gpu

CHECK_ALL_UP_TO = 130       # unknowns up to which every instance is checked against the reference


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _set_up(api, torch, name, seed):
    from mpcasm import engine

    shape = rc.shape_of(name)
    batch, count = 5, 3
    rng = np.random.default_rng(seed)
    A, Bm = sc.plants(rng, batch, shape)
    form = sc.build(api, rng, shape, plant=(A[0, 0], Bm[0, 0]))
    dyn = sc.dynamics_name(shape)
    asm = engine.Assembler(form, batch=batch, ltv=[dyn])
    asm.bind_ltv(dyn, torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"))
    given = rng.normal(0, 0.3, [batch, asm.ng])
    optim = rng.normal(0, 0.5, [batch, asm.no])
    return shape, form, dyn, asm, A, Bm, given, optim, batch, count, rng


@pytest.mark.parametrize("name", rc.GPU_SHAPES)
def test_rows_and_next_given(gpu_api, torch_gpu, name):
    torch = torch_gpu
    from mpcasm import capi, engine

    shape, form, dyn, asm, A, Bm, given, optim, B, count, rng = _set_up(gpu_api, torch, name, 300 + len(name))
    plan = asm.plan
    f = dict(dtype=torch.float64, device="cuda")
    g, x = torch.as_tensor(given, device="cuda"), torch.as_tensor(optim, device="cuda")
    kap = rc.kappa_rollout(shape.N, shape.n, shape.m)

    # ---- the rows: within the bound below count, untouched from count on --------------------------------
    out = torch.full((B, plan.pmrows), float("nan"), **f)
    assert asm.rollout(g, x, out=out, count=count) is out
    rows = out.cpu().numpy()
    assert np.isnan(rows[count:]).all() and not np.isnan(rows[:count]).any()
    picked = range(count) if asm.no <= CHECK_ALL_UP_TO else (0, count - 1)
    ref = {b: rc.reference_rows(form, dyn, A[b], Bm[b], given[b], optim[b], plan) for b in picked}
    worst = max(assert_componentwise(rows[b], *ref[b], kap, "%s, instance %d" % (name, b)) for b in picked)
    print("componentwise rollout %-12s worst %8.3g u M   kappa %d" % (name, worst, kap))
    # the copies of given and of optim are copies
    recs, _ = engine.rollout_rows(plan)
    copies = 0
    for kind, row0, n, axis, k0, kstep, cv, _ in recs:
        src = {capi.ROLL_GIVEN: given, capi.ROLL_OPTIM: optim}.get(int(kind))
        if src is not None:
            assert kstep == 1 or n == 1
            assert np.array_equal(rows[:count, row0:row0 + n], src[:count, k0:k0 + n]), (kind, row0)
            copies += n
    assert copies == asm.ng + asm.no

    # ---- rows by index: a bigger buffer of given, its rows picked by a permuted index --------------------
    big = torch.as_tensor(rng.normal(0, 1.0, [B + 3, asm.ng]), device="cuda")
    perm = rng.permutation(B + 3)[:count]
    big[torch.as_tensor(perm, device="cuda")] = g[:count]
    for index in (torch.as_tensor(perm.astype(np.int32), device="cuda"), perm):
        by_index = torch.full((B, plan.pmrows), float("nan"), **f)
        asm.rollout(big, x, index=index, out=by_index, count=count)
        assert torch.equal(by_index[:count], out[:count]) and bool(torch.isnan(by_index[count:]).all())

    # ---- the goals' distances take these rows as they are ---------------------------------------------------
    table, ngoals = pc.goal_table(form, plan)
    D = asm.goal_distance(form, out, count=count).cpu().numpy()
    params = asm.params.cpu().numpy()
    for b in picked:
        d, bound = pc.distance_reference(table, ngoals, ref[b][0], ref[b][1], params[b], kap)
        assert (np.abs(D[b].astype(LD) - d) <= bound + LD(2.0 ** -1022)).all(), (name, b, D[b], d, bound)

    # ---- the next given, in place, by a shuffled index into a bigger buffer --------------------------------
    before = big.clone()
    idx = torch.as_tensor(perm.astype(np.int32), device="cuda")
    assert asm.advance(big, x, index=idx, count=count) is big
    after = big.cpu().numpy()
    others = np.setdiff1d(np.arange(B + 3), perm)
    assert np.array_equal(after[others], before.cpu().numpy()[others])
    for b in range(count):       # (x_1 = A_0 x_0 + B_0 u_0 in long double, from the inputs alone)
        assert_componentwise(after[perm[b]], *rc.first_step_reference(plan, A[b, 0], Bm[b, 0], given[b], optim[b]),
                             kap, "%s, next given of instance %d" % (name, b))
    # ... and it is the first sample of the states the rows hold, bit for bit
    for b in range(count):
        x1 = rc.next_given_reference(plan, (rows[b], rows[b]))[0]
        assert np.array_equal(after[perm[b]], x1)
    # a status that does not apply leaves its row exactly as it was
    status = torch.as_tensor(np.array([capi.QP_SOLVED, capi.QP_PRIMAL_INFEASIBLE, capi.QP_SOLVED][:count],
                                      dtype=np.int32), device="cuda")
    masked = before.clone()
    asm.advance(masked, x, index=idx, status=status, apply_mask=engine.APPLY_SOLVED, count=count)
    assert torch.equal(masked[int(perm[1])], before[int(perm[1])])
    keep = torch.ones(B + 3, dtype=torch.bool, device="cuda")
    keep[int(perm[1])] = False
    assert torch.equal(masked[keep], big[keep])
    # without an index instance b is row b
    plain = g.clone()
    asm.advance(plain, x, count=count)
    assert torch.equal(plain[:count], big[torch.as_tensor(perm, device="cuda")]) and torch.equal(plain[count:], g[count:])
    # a host index is checked
    for bad in ([0, 0, 1][:count] if count > 2 else [1, 1], [0, B + 3][:count] + [1] * (count - 2), [-1] + [2] * (count - 1)):
        with pytest.raises(ValueError):
            asm.advance(big, x, index=np.asarray(bad), count=count)
    assert torch.equal(big.cpu(), torch.as_tensor(after))
    # ... and one on the device that points outside `given` writes nothing for that instance
    wild = idx.clone()
    wild[0] = B + 3 + 5
    asm.advance(big, x, index=wild, count=1)
    assert torch.equal(big.cpu(), torch.as_tensor(after))

    # ---- one plant shared by the batch (stride 0): what every instance computes on its own copy of it -----------
    own = np.broadcast_to(A[:1], A.shape).copy(), np.broadcast_to(Bm[:1], Bm.shape).copy()
    asm.bind_ltv(dyn, torch.as_tensor(own[0], device="cuda"), torch.as_tensor(own[1], device="cuda"))
    each = asm.rollout(g, x, count=count).clone()
    each_next = asm.advance(g.clone(), x, count=count)
    asm.bind_ltv(dyn, torch.as_tensor(A[0], device="cuda"), torch.as_tensor(Bm[0], device="cuda"))
    ids = plan.ltv[0]["ids"]
    assert asm._src_stride[ids[0]] == 0 and asm._src_stride[ids[1]] == 0
    shared = torch.full((B, plan.pmrows), float("nan"), **f)
    asm.rollout(g, x, out=shared, count=count)
    assert torch.equal(shared[:count], each[:count]) and bool(torch.isnan(shared[count:]).all())
    assert torch.equal(shared[0], out[0])               # (instance 0 read plant 0 before, too)
    assert torch.equal(asm.advance(g.clone(), x, count=count), each_next)


def test_an_assembler_without_ltv_is_refused(gpu_api, torch_gpu):
    """No launch: ValueError from the engine, MPCASM_ERR_ARG from the C entries."""
    torch = torch_gpu
    from mpcasm import capi, engine

    rng = np.random.default_rng(9)
    shape = rc.shape_of("desc")
    form = sc.build(gpu_api, rng, shape)
    asm = engine.Assembler(form, batch=2)
    f = dict(dtype=torch.float64, device="cuda")
    g, x = torch.zeros((2, asm.ng), **f), torch.zeros((2, asm.no), **f)
    with pytest.raises(ValueError, match="preview_rows"):
        asm.rollout(g, x)
    with pytest.raises(ValueError, match="next_given"):
        asm.advance(g, x)
    # the C entries, with the records and the table of the same formulation compiled as ltv
    as_ltv = engine.compile_plan(form, ltv=["plant"])
    with pytest.raises(capi.MpcasmError) as err:
        engine.rollout_table(asm.plan, *engine.rollout_rows(as_ltv), engine.rollout_sizes(as_ltv))
    assert err.value.status == capi.ERR_ARG
    table = torch.as_tensor(engine.rollout_table(as_ltv), device="cuda")
    out = torch.full((2, asm.plan.pmrows), float("nan"), **f)
    ptrs, strides = asm._src_args()
    lib = capi.load()
    assert lib.mpcasm_ltv_rollout(asm._handle, ptrs, strides, g.data_ptr(), 2, x.data_ptr(), None, table.data_ptr(),
                                  table.numel(), out.data_ptr(), 2, None) == capi.ERR_ARG
    assert lib.mpcasm_ltv_advance(asm._handle, ptrs, strides, g.data_ptr(), 2, x.data_ptr(), None, None,
                                  engine.APPLY_ALL, table.data_ptr(), table.numel(), 2, None) == capi.ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and not bool(g.any())
    # ... and on the plan they are for: a null plan, a negative count; count == 0 answers ok
    ltv = engine.Assembler(form, batch=2, ltv=["plant"])
    ptrs, strides = ltv._src_args()
    args = (ptrs, strides, g.data_ptr(), 2, x.data_ptr(), None, table.data_ptr(), table.numel(), out.data_ptr())
    assert lib.mpcasm_ltv_rollout(None, *args, 2, None) == capi.ERR_ARG
    assert lib.mpcasm_ltv_rollout(ltv._handle, *args, -1, None) == capi.ERR_ARG
    assert lib.mpcasm_ltv_rollout(ltv._handle, *args, 0, None) == capi.OK
    assert lib.mpcasm_ltv_rollout(ltv._handle, ptrs, strides, g.data_ptr(), 1, x.data_ptr(), None, table.data_ptr(),
                                  table.numel(), out.data_ptr(), 2, None) == capi.ERR_ARG     # (given: one row for two)
    # a table that is not this plan's writes nothing
    other = engine.Assembler(sc.build(gpu_api, rng, rc.shape_of("two-n1")), batch=2, ltv=["plant"])
    assert other.plan.pmrows != ltv.plan.pmrows
    wrong = other._rollout_table()
    assert lib.mpcasm_ltv_rollout(ltv._handle, ptrs, strides, g.data_ptr(), 2, x.data_ptr(), None, wrong.data_ptr(),
                                  wrong.numel(), out.data_ptr(), 2, None) == capi.OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    with pytest.raises(ValueError):
        ltv.rollout(g, x, count=3)
    with pytest.raises(ValueError):
        ltv.rollout(g[:, :-1].contiguous(), x)


@pytest.mark.parametrize("shared", [False, True], ids=["per-instance", "shared"])
def test_a_window_bound_by_pointer(gpu_api, torch_gpu, shared):
    """bind_ltv_window(t) reads what bind_ltv reads from a contiguous copy of the window: assemble and rollout
    bit for bit, at t = 0 and at an odd offset (the blocks then start on an odd double)."""
    torch = torch_gpu
    from mpcasm import engine

    shape, T, B = rc.shape_of("lipm-33"), 33 + 4, 3
    rng = np.random.default_rng(41)
    long_shape = shape._replace(N=T)
    A, Bm = sc.plants(rng, B, long_shape)
    if shared:
        A, Bm = A[0], Bm[0]
    form = sc.build(gpu_api, rng, shape)
    asm = engine.Assembler(form, batch=B, ltv=["LIP"])
    At, Bt = torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda")
    g = torch.as_tensor(rng.normal(0, 0.3, [B, asm.ng]), device="cuda")
    x = torch.as_tensor(rng.normal(0, 0.5, [B, asm.no]), device="cuda")
    for t in (0, 3):
        asm.bind_ltv_window("LIP", At, Bt, t)
        ids = asm.plan.ltv[0]["ids"]
        assert asm._src[ids[0]].data_ptr() == At.data_ptr() + 8 * t * 9           # (nothing copied)
        assert asm._src_stride[ids[0]] == (0 if shared else T * 9)
        win = [tuple(v.clone() for v in asm.assemble(g)), asm.rollout(g, x).clone(), asm.advance(g.clone(), x)]
        asm.bind_ltv("LIP", At[..., t:t + shape.N, :, :].contiguous(), Bt[..., t:t + shape.N, :, :].contiguous())
        ref = [asm.assemble(g), asm.rollout(g, x), asm.advance(g.clone(), x)]
        assert all(torch.equal(a, b) for a, b in zip(win[0], ref[0]))
        assert torch.equal(win[1], ref[1]) and torch.equal(win[2], ref[2])
    with pytest.raises(ValueError):
        asm.bind_ltv_window("LIP", At, Bt, T - shape.N + 1)
    with pytest.raises(ValueError):
        asm.bind_ltv_window("LIP", At, Bt, -1)
    with pytest.raises(ValueError):
        asm.bind_ltv_window("LIP", At.transpose(-1, -2), Bt, 0)
