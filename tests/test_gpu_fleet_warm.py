"""GPU: the closed loops with a warm start (WalkerFleet(warm=True), LtvLoop(warm=True)) -- the fleet against the
restatement's closed warm loop (tests/warm_restatement.py), teacher-forced as test_gpu_fleet_loop.py's fleet is:
every tick of the restatement is posed at the device's own ``given`` and starts from the device's own record."""
import numpy as np
import pytest

import osqp_restatement as rs
import rollout_cases as rc
import warm_restatement as wr
from mpcasm import capi, problems
from mpcasm.walkers import WalkerFleet

pytestmark = pytest.mark.gpu
MARGIN = 1e-6


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def per_walker(out, key):
    """``key`` of a step's entries, in walker order."""
    pairs = []
    for entry in out:
        pairs += list(zip(entry["index"].cpu().numpy().tolist(), entry[key].cpu().numpy().tolist()))
    return np.array([v for _, v in sorted(pairs)])


def test_eight_walkers_against_the_restated_warm_loop(gpu_api, torch_gpu):
    conf = problems.BipedConfig(step_samples=8)
    ticks = 20
    fleet = WalkerFleet(8, phases=np.arange(8), conf=conf, api=gpu_api, warm=True)
    given = fleet.start_at_rest()
    assert fleet.warm_store is None
    trail, status, iters, warm, records = [given.cpu().numpy()], [], [], [], []
    for _ in range(ticks):
        out = fleet.step()
        trail.append(given.cpu().numpy())
        status.append(per_walker(out, "status"))
        iters.append(per_walker(out, "iters"))
        warm.append(per_walker(out, "warm"))
        store = fleet.warm_store
        records.append([t.cpu().numpy() for t in (store.x, store.y, store.rho, store.meta)])
    status, iters, warm = np.array(status), np.array(iters), np.array(warm)
    # the rule: cold at tick 0 and after every tick whose status was not SOLVED
    assert not warm[0].any()
    assert np.array_equal(warm[1:], (status[:-1] == rs.SOLVED).astype(warm.dtype))
    print("warm share after tick 0: %.3f; unsolved walker-ticks: %d" % (warm[1:].mean(), (status != rs.SOLVED).sum()))
    # every record is this tick's, whatever the status
    for t, (_x, _y, _rho, meta) in enumerate(records):
        assert np.array_equal(meta[:, 0], status[t]) and (meta[:, 1] == t % 16).all()
    form = problems.biped(gpu_api, conf)
    judged = total = 0
    for b in range(8):
        def forced(t, g, sol, record, b=b):
            x, y, rho, meta = records[t]
            record.update(x=x[b], y=y[b], rho=float(rho[b]), status=int(meta[b, 0]))
            return trail[t + 1][b]

        host = wr.warm_loop(form, conf, b, ticks, given=trail[0][b], forced=forced)
        for t, tick in enumerate(host):
            assert tick.warm == warm[t, b], (b, t)
            total += 1
            if tick.sol.margin < MARGIN:
                continue
            judged += 1
            assert (status[t, b], iters[t, b]) == (tick.sol.status, tick.sol.iters), \
                (b, t, status[t, b], iters[t, b], tick.sol.status, tick.sol.iters, tick.warm)
    print("judged %d of %d walker-ticks; device iterations: warm ticks %.1f, cold ticks %.1f"
          % (judged, total, iters[warm == 1].mean(), iters[warm == 0].mean()))
    assert judged >= 0.9 * total, (judged, total)


def test_warm_ticks_replayed_from_graphs(gpu_api, torch_gpu):
    torch = torch_gpu
    conf = problems.BipedConfig(step_samples=8)
    B, ticks = 64, 2 * 2 * conf.step_samples + 3
    eager = WalkerFleet(B, conf=conf, api=gpu_api, warm=True)
    graphs = WalkerFleet(B, conf=conf, api=gpu_api, warm=True, graphs=True)
    eager.start_at_rest()
    graphs.start_at_rest()
    a = eager.run(ticks, record=True)
    b = graphs.run(ticks, record=True)
    assert len(graphs._step_graphs) == 2 * conf.step_samples
    for k in ("given", "status", "iters"):
        assert torch.equal(a[k], b[k]), k
    assert int((a["status"] == capi.QP_SOLVED).sum()) > 0.9 * a["status"].numel()
    for s, t in zip((eager.warm_store.x, eager.warm_store.rho, eager.warm_store.meta),
                    (graphs.warm_store.x, graphs.warm_store.rho, graphs.warm_store.meta)):
        assert torch.equal(s, t)


def test_a_warm_step_reads_nothing_back(gpu_api, torch_gpu):
    torch = torch_gpu
    conf = problems.BipedConfig(step_samples=8)
    fleet = WalkerFleet(64, conf=conf, api=gpu_api, warm=True)
    fleet.start_at_rest()
    fleet.run(2 * conf.step_samples)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(16):
            fleet.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_warm_false_is_the_fleet_without_the_argument(gpu_api, torch_gpu):
    torch = torch_gpu
    conf = problems.BipedConfig(step_samples=8)
    plain = WalkerFleet(16, conf=conf, api=gpu_api)
    off = WalkerFleet(16, conf=conf, api=gpu_api, warm=False)
    plain.start_at_rest()
    off.start_at_rest()
    a, b = plain.run(20, record=True), off.run(20, record=True)
    for k in ("given", "status", "iters"):
        assert torch.equal(a[k], b[k]), k
    assert off.warm_store is None
    # ... and the warm fleet does walk on: fewer iterations for the same walk
    on = WalkerFleet(16, conf=conf, api=gpu_api, warm=True)
    on.start_at_rest()
    c = on.run(20, record=True)
    assert int(c["iters"][1:].sum()) < int(a["iters"][1:].sum())


def test_the_ltv_loop_warm(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm.ltv_loop import LtvLoop

    form, A, B, given0 = rc.loop_inputs(gpu_api)
    dev = lambda v: torch.as_tensor(v, device="cuda")
    totals = {}
    for warm in (False, True):
        loop = LtvLoop(form, "LIP", rc.LOOP_BATCH, dev(A), dev(B), warm=warm)
        loop.given.copy_(dev(given0))
        status, iters, flags = [], [], []
        for _ in range(rc.LOOP_TICKS):
            out = loop.step()
            assert ("warm" in out) == warm
            status.append(out["status"].cpu().numpy().copy())
            iters.append(out["iters"].cpu().numpy().copy())
            if warm:
                flags.append(out["warm"].cpu().numpy().copy())
        status, iters = np.array(status), np.array(iters)
        for b, want in rc.LOOP_STATUS.items():
            assert (status[:, b] == want).all(), (warm, b, status[:, b])
        solved = [b for b, want in rc.LOOP_STATUS.items() if want == rs.SOLVED]
        totals[warm] = int(iters[:, solved].sum())
        if warm:
            flags = np.array(flags)
            assert not flags[0].any()
            assert not flags[:, 1].any()                 # held: primal infeasible, cold every tick
            assert flags[1:][:, solved].all()
    print("iterations of the solved instances over %d ticks: cold %d, warm %d"
          % (rc.LOOP_TICKS, totals[False], totals[True]))
    assert totals[True] <= totals[False]
