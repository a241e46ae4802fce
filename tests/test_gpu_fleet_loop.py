"""GPU: the closed walking loop on the device (WalkerFleet.step / run) and its last step,
mpcasm_next_given, against the host restatement of the reference's loop (tests/fleet_loop_reference.py:
oracle.qp_oracle.assemble, osqp_restatement.solve, oracle.qp_oracle.preview, update_given_collector).
Comparisons are per element or per row of `given`; a walker whose solve decides within 1e-6 of a tie is not judged
on its verdict (sums rounded in another order may flip it)."""
import numpy as np
import pytest

import osqp_restatement as rs
from fleet_loop_reference import HostWalker, host_loop, rest_given
from mpcasm import capi, problems
from mpcasm.walkers import WalkerFleet, step_indicator, steps_in_preview

pytestmark = pytest.mark.gpu
MARGIN = 1e-6
TICKS = 48


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def per_element(dev, ref, rtol, atol=0.0):
    """|dev - ref| <= rtol |ref| + atol for every element; the worst offender in the message."""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(dev - ref) - (rtol * np.abs(ref) + atol)
    i = np.unravel_index(int(np.argmax(err)), err.shape) if err.size else ()
    return bool((err <= 0).all()), (i, dev[i] if err.size else None, ref[i] if err.size else None)


def per_row(dev, ref, rtol):
    """max |dev - ref| <= rtol max |ref| in every row (last axis): a `given` row mixes positions of a few
    tenths with accelerations near zero, and the solver's iterates are only as close as their scale."""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(dev - ref).max(axis=-1) - rtol * np.abs(ref).max(axis=-1)
    i = np.unravel_index(int(np.argmax(err)), err.shape) if err.size else ()
    return bool((err <= 0).all()), (i, float(np.abs(dev[i] - ref[i]).max()), float(np.abs(ref[i]).max()))


# ---- the kernel alone ---------------------------------------------------------------------------------------
def bucket_assembler(api, conf, phase, batch):
    from mpcasm.engine import Assembler

    n = conf.step_samples
    times = np.array([(i + 1) * n - 1 - phase for i in range(conf.num_steps)])
    form = problems.biped(api, conf)
    form.update(step_times=times, step_count=0)
    return form, Assembler(form, batch=batch)


@pytest.mark.parametrize("phase", [0, 7], ids=["34 wide", "36 wide"])
def test_next_given_against_preview_rows(gpu_api, torch_gpu, phase):
    """A permuted index into a larger `given`, fewer instances than the batch, a map with rows, constants and
    kept columns, statuses on both sides of the mask, a step indicator of every instance's own: the mapped
    columns are the oracle's preview of each instance (to 1e-13 of the instance's values) and, with the sources
    shared, preview_rows' gathered (to 1e-13 per element); everything else is left bit for bit."""
    from oracle import qp_oracle as orc
    torch = torch_gpu
    from mpcasm import engine

    conf = problems.BipedConfig(step_samples=8)
    B, count, rows_total = 96, 70, 150
    form, asm = bucket_assembler(gpu_api, conf, phase, B)
    rng = np.random.default_rng(11 + phase)
    # a step indicator of every instance's own, from step times of this bucket's structure (a per-instance
    # source, as a fleet binds it: the kernel reads it at its stride)
    phases = rng.integers(1, 8, B) if phase else np.zeros(B, dtype=np.int64)
    times = np.array([[(i + 1) * 8 - 1 - f for i in range(2)] for f in phases])
    kept = times[steps_in_preview(times, 16)].reshape(B, -1)
    E = torch.as_tensor(step_indicator(kept, 16)[..., None], device="cuda")
    asm.bind_source(("steps", 0), E)
    rules = {"x0_x": [("CoM_x", 3), None, ("CoM_ddot_x", 15)], "x0_y": [("DCM_y", 2), ("(b+n-s)_y", 0), ("s_y", 1)],
             "s0_y": 0.25, "s0_x": [("s_x", 1)], "n_x": -1.5}
    gmap = asm.given_map(rules)
    rows, values = gmap.rows, gmap.values
    assert {int(r) for r in rows if r < 0} == {capi.GIVEN_KEEP, capi.GIVEN_CONST}
    given0 = torch.as_tensor(rng.normal(0, 0.4, (rows_total, asm.ng)), device="cuda")
    optim = torch.as_tensor(rng.normal(0, 0.4, (B, asm.no)), device="cuda")
    idx = rng.permutation(rows_total)[:count].astype(np.int32)
    index = torch.as_tensor(idx, device="cuda")
    codes = np.array(sorted(capi.QP_STATUS), dtype=np.int32)
    status_h = codes[rng.integers(0, codes.size, B)]
    status = torch.as_tensor(status_h, device="cuda")
    given = given0.clone()
    asm.next_given(given, optim, gmap, index=index, status=status, apply_mask=engine.APPLY_SOLVED, count=count)
    g0, g = given0.cpu().numpy(), given.cpu().numpy()
    x_h = optim.cpu().numpy()
    pv = np.zeros((count, asm.plan.pmrows))
    for b in range(count):     # the oracle's rows of this instance, at its own step times
        form.update(step_times=times[b], step_count=0)
        PM = orc.preview_matrices(form)
        for v, (r0, n) in asm.plan.pm_rows.items():
            pv[b, r0:r0 + n] = orc.preview(PM, g0[idx[b]].reshape(-1, 1), x_h[b].reshape(-1, 1), v).ravel()
    applies = np.isin(status_h[:count], [capi.QP_SOLVED, capi.QP_MAX_ITER])
    assert applies.any() and not applies.all()
    named, const, keep = rows >= 0, rows == capi.GIVEN_CONST, rows == capi.GIVEN_KEEP
    for b in range(count):
        r = idx[b]
        if not applies[b]:
            assert np.array_equal(g[r], g0[r]), b
            continue
        ok, worst = per_row(g[r][named], pv[b][rows[named]], 1e-13)
        assert ok, (b, worst)
        assert np.array_equal(g[r][const], values[const])
        assert np.array_equal(g[r][keep], g0[r][keep])
    untouched = np.setdiff1d(np.arange(rows_total), idx)
    assert np.array_equal(g[untouched], g0[untouched])
    # with the sources shared by the batch: preview_rows' rows, gathered, per element
    assert asm.rebind_sources(form)
    shared = given0.clone()
    asm.next_given(shared, optim, gmap, index=index, count=count)
    prow = asm.preview_rows(given0.index_select(0, index.long()), optim, count=count).cpu().numpy()
    sh = shared.cpu().numpy()
    for b in range(count):
        ok, worst = per_element(sh[idx[b]][named], prow[b][rows[named]], 1e-13)
        assert ok, ("shared", b, worst)
    asm.bind_source(("steps", 0), E)
    # every instance applies without a status: the same values where the mask held nothing back
    again = given0.clone()
    asm.next_given(again, optim, gmap, index=index, count=count)
    a = again.cpu().numpy()
    assert np.array_equal(a[idx[applies]], g[idx[applies]])
    # an index from the host is checked: out of range / repeated rows are refused, nothing is launched
    for bad in ([rows_total] + list(idx[1:count]), [idx[0]] * count):
        with pytest.raises(ValueError):
            asm.next_given(again, optim, gmap, index=np.array(bad), count=count)
    # ... and one on the device that points outside `given` writes nothing for that instance
    wild = index.clone()
    wild[0] = rows_total + 5
    before = again.clone()
    asm.next_given(again, optim, gmap, index=wild, count=1)
    assert torch.equal(again, before)
    # a map of the other bucket's plan is refused on the host
    other = bucket_assembler(gpu_api, conf, 7 - phase, B)[1]
    with pytest.raises(ValueError):
        asm.next_given(again, optim, other.given_map(rules), index=index, count=count)


def test_next_given_refuses_a_sweep_plan(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm.engine import Assembler

    form = problems.lipm_ltv(gpu_api, N=20)
    asm = Assembler(form, batch=4, ltv=["LIP"])
    assert asm.plan.ltv
    var = next(iter(asm.plan.given_ID))
    with pytest.raises(capi.MpcasmError) as e:
        asm.given_map({var: 0.0})
    assert e.value.status == capi.ERR_LIMIT
    lib = capi.load()
    given = torch.zeros((4, asm.ng), dtype=torch.float64, device="cuda")
    optim = torch.zeros((4, max(asm.no, 1)), dtype=torch.float64, device="cuda")
    words = torch.zeros(16, dtype=torch.int32, device="cuda")
    ptrs, strides = asm._src_args()
    rc = lib.mpcasm_next_given(asm._handle, ptrs, strides, given.data_ptr(), 4, optim.data_ptr(), None, None, 0,
                               words.data_ptr(), 16, asm._workspace().data_ptr(), 4, None)
    assert rc == capi.ERR_LIMIT


# ---- the fleet, teacher-forced: every tick from the device's own rows -----------------------------------------
def test_a_fleet_of_4096_walkers_tick_by_tick(gpu_api, torch_gpu):
    torch = torch_gpu
    conf = problems.BipedConfig(step_samples=8)
    B = 4096
    fleet = WalkerFleet(B, conf=conf, api=gpu_api, on_unsolved="hold")
    given = fleet.start_at_rest()
    form = problems.biped(gpu_api, conf)
    host = HostWalker(form, conf, 0, "hold")
    rng = np.random.default_rng(5)
    samples = checked = 0
    for tick in range(TICKS):
        pre = given.cpu().numpy()
        times, counts = fleet.clock.step_times.copy(), fleet.clock.step_count.copy()
        out = fleet.step()
        post = given.cpu().numpy()
        pick = set(rng.choice(B, 32, replace=False).tolist())
        per_walker = {}
        for entry in out:
            ids = entry["index"].cpu().numpy()
            pick.update((int(ids[0]), int(ids[-1])))
            st, it = entry["status"].cpu().numpy(), entry["iters"].cpu().numpy()
            for row, b in enumerate(ids):
                per_walker[int(b)] = (int(st[row]), int(it[row]))
        assert sorted(per_walker) == list(range(B))
        for b in sorted(pick):
            samples += 1
            sol, nxt = host.solve(pre[b], times[b], counts[b])
            if sol.margin <= MARGIN:
                continue
            checked += 1
            assert per_walker[b] == (sol.status, sol.iters), (tick, b, per_walker[b], sol.status, sol.iters)
            ok, worst = per_row(post[b], nxt, 1e-9)
            assert ok, (tick, b, worst)
    assert checked >= 0.9 * samples, (checked, samples)


# ---- free runs: eight walkers against eight host loops ---------------------------------------------------------
@pytest.mark.parametrize("policy", ["hold", "apply"])
def test_eight_walkers_walk_like_the_host_loop(gpu_api, torch_gpu, policy):
    conf = problems.BipedConfig(step_samples=8)
    fleet = WalkerFleet(8, phases=np.arange(8), conf=conf, api=gpu_api, on_unsolved=policy)
    fleet.start_at_rest()
    res = fleet.run(TICKS, record=True)
    status, iters, trail = (res[k].cpu().numpy() for k in ("status", "iters", "given"))
    assert status.shape == (TICKS, 8) and trail.shape == (TICKS + 1, 8, fleet.given_len)
    form = problems.biped(gpu_api, conf)
    com_x = form.given_ID["x0_x"][0]
    for phase in range(8):
        st, it, tr, margin = host_loop(form, conf, phase, TICKS, policy)
        assert margin > MARGIN, (phase, margin)
        assert np.array_equal(status[:, phase], st), (phase, status[:, phase], st)
        assert np.array_equal(iters[:, phase], it), (phase, iters[:, phase], it)
        # (under "apply" the iterates a primal-infeasible verdict stops at -- a diverging sequence -- become the
        # next state: the two loops' rounding grows faster there, 1.1e-8 of the row at worst measured)
        ok, worst = per_row(trail[:, phase], tr, 1e-8 if policy == "hold" else 1e-7)
        assert ok, (phase, worst)
        unsolved = np.flatnonzero(st != rs.SOLVED)
        if policy == "hold":
            if phase >= 4:
                assert 1 <= unsolved.size <= 4, (phase, st)
            for t in unsolved:      # held: the row after the tick is the row before it, bit for bit
                assert np.array_equal(trail[t + 1, phase], trail[t, phase]), (phase, t)
            assert trail[-1, phase, com_x] > trail[0, phase, com_x] + 0.1, phase
        elif phase >= 4:
            assert unsolved.size > 0, (phase, st)
    assert np.array_equal(trail[0], np.broadcast_to(rest_given(form, conf), trail[0].shape))


# ---- graphs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side_by_side", [False, True], ids=["one after the other", "side by side"])
def test_closed_ticks_replayed_from_graphs(gpu_api, torch_gpu, side_by_side):
    torch = torch_gpu
    conf = problems.BipedConfig(step_samples=8)
    B = 600
    ticks = 2 * 2 * conf.step_samples + 3
    eager = WalkerFleet(B, conf=conf, api=gpu_api)
    graphs = WalkerFleet(B, conf=conf, api=gpu_api, graphs=True, side_by_side=side_by_side)
    eager.start_at_rest()
    graphs.start_at_rest()
    a = eager.run(ticks, record=True)
    b = graphs.run(ticks, record=True)
    assert len(graphs._step_graphs) == 2 * conf.step_samples
    for k in ("given", "status", "iters"):
        assert torch.equal(a[k], b[k]), k
    assert int((a["status"] == capi.QP_SOLVED).sum()) > 0.9 * a["status"].numel()


def test_a_step_reads_nothing_back(gpu_api, torch_gpu):
    torch = torch_gpu
    conf = problems.BipedConfig(step_samples=8)
    fleet = WalkerFleet(512, conf=conf, api=gpu_api)
    fleet.start_at_rest()
    fleet.run(2 * 2 * conf.step_samples)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(16):
            fleet.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
