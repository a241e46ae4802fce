"""GPU: mpcasm_qp_warm_store / mpcasm_qp_warm_start against tests/warm_restatement.py -- every launch mixes warm
instances with every way of being cold, through a permuted index into a store of more rows than instances and of
another width than the launch.  x0, y0, rho0, d_warm and every cold z0 are compared bit for bit; a warm z0 is h
bit for bit where h wins and otherwise within (no + 2) u sum_j |G_ij| |x0_j| of the long-double G x0."""
import numpy as np
import pytest

import osqp_restatement as rs
import warm_restatement as wr
from helpers import U64, assert_componentwise

pytestmark = pytest.mark.gpu
TAG = 5
# what instance b of a launch is: by b modulo the list's length
WARM, WRONG_TAG, STATUS_OUT, RHO_ZERO, RHO_NAN, RHO_BIG, NAN_X, NAN_UNREAD, NAN_Y = range(9)
SHAPES = [(1, 1, 67), (5, 3, 67), (36, 76, 67), (34, 72, 67), (63, 5, 67), (64, 70, 67), (65, 70, 67), (129, 4, 67),
          (7, 0, 67), (512, 2048, 3)]


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def store_widths(no, nc):
    """The store's widths for a launch: another bucket's for the biped's two (36 -> 34 and back), narrower at the
    size limit (a store is at most 512 by 2 048), else wider."""
    return {(36, 76): (34, 72), (34, 72): (36, 76), (512, 2048): (509, 2046)}.get((no, nc), (no + 3, nc + 2))


def mixed_case(rng, no, nc, B):
    sno, snc = store_widths(no, nc)
    R = B + 9
    G, h = rng.normal(size=(B, nc, no)), rng.normal(0.0, 0.5 * np.sqrt(no), size=(B, nc))
    SX, SY = rng.normal(size=(R, sno)), rng.normal(size=(R, snc))
    SR = rng.uniform(0.01, 10.0, R)
    SM = np.tile(np.array([[rs.SOLVED, TAG]], dtype=np.int32), (R, 1))
    index = rng.permutation(R)[:B].astype(np.int32)
    # the tables never read the store's last column (NAN_UNREAD sits there); their first entry reads column 0
    col = rng.integers(-1, max(sno - 1, 1), no).astype(np.int32)
    row = rng.integers(-1, max(snc - 1, 1), nc).astype(np.int32)
    col[0] = 0
    if no > 1:
        col[-1] = -1
    if nc:
        row[0] = 0
    if nc > 1:
        row[-1] = -1
    kinds = [WARM, NAN_X, NAN_UNREAD] if B < 9 else list(range(9))
    kind = np.array([kinds[b % len(kinds)] for b in range(B)])
    for b, r in enumerate(index):
        k = kind[b]
        if k == WRONG_TAG:
            SM[r, 1] = TAG + 1
        elif k == STATUS_OUT:
            SM[r, 0] = rs.MAX_ITER
        elif k == RHO_ZERO:
            SR[r] = 0.0
        elif k == RHO_NAN:
            SR[r] = np.nan
        elif k == RHO_BIG:
            SR[r] = 1e7
        elif k == NAN_X:
            SX[r, 0] = np.nan
        elif k == NAN_UNREAD:
            SX[r, sno - 1] = np.nan
            if snc:
                SY[r, snc - 1] = np.nan
        elif k == NAN_Y and nc:
            SY[r, 0] = np.nan
    expect = np.isin(kind, [WARM, NAN_UNREAD]) | ((kind == NAN_Y) & (nc == 0))
    return dict(G=G, h=h, SX=SX, SY=SY, SR=SR, SM=SM, index=index, col=col, row=row, expect=expect.astype(np.int32))


def device_store(torch, engine, case):
    SX, SY = case["SX"], case["SY"]
    store = engine.WarmStore(SX.shape[0], SX.shape[1], SY.shape[1], "cuda")
    for t, v in ((store.x, SX), (store.y, SY), (store.rho, case["SR"]), (store.meta, case["SM"])):
        t.copy_(torch.as_tensor(v, device="cuda"))
    return store


def run_start(torch, engine, case, store, col=None, row=None):
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), device="cuda")
    ws = engine.warm_start_qp(store, dev(case["G"]), dev(case["h"]), dev(case["col"] if col is None else col),
                              dev(case["row"] if row is None else row), TAG, index=dev(case["index"]),
                              warm_mask=engine.WARM_SOLVED, rho_cold=0.1)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ws]


@pytest.mark.parametrize("no,nc,B", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_a_mixed_launch_against_the_restatement(torch_gpu, no, nc, B):
    torch = torch_gpu
    from mpcasm import engine

    rng = np.random.default_rng(100 * no + nc)
    case = mixed_case(rng, no, nc, B)
    store = device_store(torch, engine, case)
    x, y, z, rho, warm = run_start(torch, engine, case, store)
    ref = wr.warm_start(case["G"], case["h"], case["SX"], case["SY"], case["SR"], case["SM"], case["index"],
                        case["col"], case["row"], TAG, wr.qp_bit(rs.SOLVED), 0.1)
    assert np.array_equal(np.array([s.warm for s in ref]), case["expect"])
    assert np.array_equal(warm, case["expect"]) and 0 < warm.sum() < B
    worst, won_total, lost_total = 0.0, 0, 0
    for b, s in enumerate(ref):
        assert same_bits(x[b], s.x) and same_bits(y[b], s.y), b
        assert same_bits(rho[b:b + 1], np.array([s.rho])), b
        if not s.warm:
            assert same_bits(z[b], s.z), b
            continue
        hb = case["h"][b]
        won = bits(z[b]) == bits(hb)
        slack = (no + 2) * U64 * s.mag
        # where h was taken, G x0 is not below it by more than the bound; where it was not, G x0 is not above
        assert (s.gx_ld[won] + slack[won] >= hb[won]).all() and (s.gx_ld[~won] - slack[~won] <= hb[~won]).all(), b
        if (~won).any():
            worst = max(worst, assert_componentwise(z[b][~won], s.gx_ld[~won], s.mag[~won], no + 2,
                                                    "z0 of instance %d" % b))
        won_total, lost_total = won_total + int(won.sum()), lost_total + int((~won).sum())
    print("(%d, %d): worst warm z0 %.2f u M of %d allowed; h won %d rows, G x0 %d"
          % (no, nc, worst, no + 2, won_total, lost_total))
    if nc:
        assert won_total and lost_total
    # entries of -5 and store width + 3 count as -1
    col2, row2 = case["col"].copy(), case["row"].copy()
    for table, width in ((col2, case["SX"].shape[1]), (row2, case["SY"].shape[1])):
        minus = np.flatnonzero(table == -1)
        table[minus[0::2]] = -5
        table[minus[1::2]] = width + 3
    if no > 1:
        assert (col2 != case["col"]).any()
    again = run_start(torch, engine, case, store, col2, row2)
    for a, b_ in zip((x, y, z, rho, warm), again):
        assert same_bits(a, b_)
    # an index outside the store: that instance is cold, nothing else changes
    wild = dict(case, index=case["index"].copy())
    wild["index"][0] = case["SX"].shape[0] + 4
    xw, yw, zw, rw, ww = run_start(torch, engine, wild, store)
    assert ww[0] == 0 and not xw[0].any() and rw[0] == 0.1 and same_bits(zw[0], np.minimum(0.0, case["h"][0]))
    assert same_bits(xw[1:], x[1:]) and same_bits(zw[1:], z[1:]) and np.array_equal(ww[1:], warm[1:])


@pytest.mark.parametrize("no,nc", [(36, 76), (5, 3), (129, 4), (7, 0)])
def test_store_then_start_returns_the_solution_bit_for_bit(torch_gpu, no, nc):
    torch = torch_gpu
    from mpcasm import engine

    rng = np.random.default_rng(7 + no)
    B, R = 67, 80
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), device="cuda")
    x, y, rho = rng.normal(size=(B, no)), rng.normal(size=(B, nc)), rng.uniform(0.01, 10.0, B)
    x[3, 0], y[5:6, :1] = -0.0, -0.0
    codes = np.array(sorted(rs_codes()), dtype=np.int32)
    status = codes[rng.integers(0, codes.size, B)]
    status[:4] = rs.SOLVED
    index = rng.permutation(R)[:B].astype(np.int32)
    store = engine.WarmStore(R, no + 3, nc + 2, "cuda")
    store.x.fill_(7.5), store.y.fill_(-7.5), store.rho.fill_(3.25), store.meta.fill_(9)
    engine.warm_store_qp(store, (dev(x), dev(y), dev(rho), dev(status)), TAG, index=dev(index))
    torch.cuda.synchronize()
    SX, SY, SR, SM = (t.cpu().numpy() for t in (store.x, store.y, store.rho, store.meta))
    # every instance is stored whatever its status, padded with zeros; rows nobody names keep their bits
    assert same_bits(SX[index][:, :no], x) and not SX[index][:, no:].any()
    assert same_bits(SY[index][:, :nc], y) and not SY[index][:, nc:].any()
    assert same_bits(SR[index], rho) and np.array_equal(SM[index], np.stack([status, np.full(B, TAG)], axis=1))
    others = np.setdiff1d(np.arange(R), index)
    assert (SX[others] == 7.5).all() and (SY[others] == -7.5).all() and (SR[others] == 3.25).all() and \
        (SM[others] == 9).all()
    G, h = rng.normal(size=(B, nc, no)), rng.normal(size=(B, nc))
    ident = lambda n: dev(np.arange(n, dtype=np.int32))
    ws = engine.warm_start_qp(store, dev(G), dev(h), ident(no), ident(nc), TAG, index=dev(index))
    torch.cuda.synchronize()
    warm = ws.warm.cpu().numpy()
    assert np.array_equal(warm, (status == rs.SOLVED).astype(np.int32)) and 4 <= warm.sum() < B
    on = warm == 1
    assert same_bits(ws.x.cpu().numpy()[on], x[on]) and same_bits(ws.y.cpu().numpy()[on], y[on])
    assert same_bits(ws.rho.cpu().numpy()[on], rho[on])
    assert not ws.x.cpu().numpy()[~on].any() and (ws.rho.cpu().numpy()[~on] == 0.1).all()
    # an entry of the index outside the store is skipped; a host index is checked
    before = [t.clone() for t in (store.x, store.y, store.rho, store.meta)]
    wild = index.copy()
    wild[:] = R + 2
    engine.warm_store_qp(store, (dev(x), dev(y), dev(rho), dev(status)), TAG + 1, index=dev(wild))
    torch.cuda.synchronize()
    for t, b in zip((store.x, store.y, store.rho, store.meta), before):
        assert torch.equal(t, b)
    with pytest.raises(ValueError):
        engine.warm_store_qp(store, (dev(x), dev(y), dev(rho), dev(status)), TAG, index=wild)


def rs_codes():
    return (rs.SOLVED, rs.MAX_ITER, rs.PRIMAL_INFEASIBLE, rs.DUAL_INFEASIBLE, rs.NON_CVX)


def solvable_batch(torch, rng, no, nc, B):
    qps = [rs.random_qp(rng, no, nc) for _ in range(B)]
    return [torch.as_tensor(np.stack([np.asarray(qp[i]) for qp in qps]), device="cuda").contiguous()
            for i in range(4)]


@pytest.mark.parametrize("no,nc,wide", [(36, 76, False), (5, 3, False), (129, 4, True)])
def test_a_warm_solve_on_an_all_cold_start_is_the_cold_solve(torch_gpu, no, nc, wide):
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h = solvable_batch(torch, np.random.default_rng(no), no, nc, 5)
    solve = engine.solve_qp_wide if wide else engine.solve_qp
    cold = solve(P, q, G, h)
    store = engine.WarmStore(5, no, nc, "cuda")      # fresh: nothing is warm
    ident = lambda n: torch.arange(n, dtype=torch.int32, device="cuda")
    ws = engine.warm_start_qp(store, G, h, ident(no), ident(nc), 0)
    assert int(ws.warm.sum()) == 0
    warm = solve(P, q, G, h, x=ws.x, y=ws.y, z=ws.z, rho=ws.rho)
    torch.cuda.synchronize()
    assert int((cold.status == rs.SOLVED).sum()) > 0
    for name in ("x", "y", "z", "status", "iters", "res", "rho"):
        a, b = getattr(cold, name).cpu().numpy(), getattr(warm, name).cpu().numpy()
        assert same_bits(a, b), name


def test_one_graph_of_start_solve_store_replays_to_the_same_bits(torch_gpu):
    torch = torch_gpu
    from mpcasm import engine

    no, nc, B = 36, 76, 6
    rng = np.random.default_rng(3)
    P, q, G, h = solvable_batch(torch, rng, no, nc, B)
    first = engine.solve_qp(P, q, G, h)
    store = engine.WarmStore(B, no, nc, "cuda")
    engine.warm_store_qp(store, first, TAG)
    store.meta[2, 1] = TAG + 1                      # one cold instance among the warm
    initial = [t.clone() for t in (store.x, store.y, store.rho, store.meta)]
    q2 = (q + 0.05 * torch.as_tensor(rng.normal(size=(B, no)), device="cuda")).contiguous()
    f, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    buf = dict(x=torch.zeros((B, no), **f), y=torch.zeros((B, nc), **f), z=torch.zeros((B, nc), **f),
               rho=torch.zeros(B, **f), warm=torch.zeros(B, **i32), status=torch.zeros(B, **i32),
               iters=torch.zeros(B, **i32), res=torch.zeros((B, 2), **f))
    ident = lambda n: torch.arange(n, dtype=torch.int32, device="cuda")
    cols, rows = ident(no), ident(nc)

    def chain():
        engine.warm_start_qp(store, G, h, cols, rows, TAG, out=tuple(buf[k] for k in ("x", "y", "z", "rho", "warm")))
        sol = engine.solve_qp(P, q2, G, h, rho=buf["rho"], warm=True,
                              out=tuple(buf[k] for k in ("x", "y", "z", "status", "iters", "res")))
        engine.warm_store_qp(store, sol, TAG + 2)

    def snapshot():
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in buf.items()}, [t.clone() for t in (store.x, store.y, store.rho, store.meta)]

    chain()
    eager, eager_store = snapshot()
    assert eager["warm"].tolist() == [1, 1, 0, 1, 1, 1] and int((eager["status"] == rs.SOLVED).sum()) == B
    for t, v in zip((store.x, store.y, store.rho, store.meta), initial):
        t.copy_(v)
    for v in buf.values():
        v.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    graph.replay()
    replayed, replayed_store = snapshot()
    for k in buf:
        assert torch.equal(eager[k], replayed[k]) or same_bits(eager[k].cpu().numpy(), replayed[k].cpu().numpy()), k
    for a, b in zip(eager_store, replayed_store):
        assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    assert replayed_store[3][:, 1].tolist() == [TAG + 2] * B
