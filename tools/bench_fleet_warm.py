#!/usr/bin/env python3
"""The closed walking loop of a fleet with and without the warm start (WalkerFleet(warm=...).step) on one device:
4 096 biped walkers (phases b % 8) from rest, 48 ticks, cold and warm in the same process with interleaved
windows, eager and replayed from graphs.  hipEvents on the current stream; writes profiles/fleet_warm_bench.json
and prints a short form as one JSON line.

* ms per closed tick, cold and warm: per window the mean and median over its ticks; the medians of the windows
* the split of a tick between assembly, warm start, solve, store and next_given (events between the pieces, per
  bucket, summed per tick), over one more cycle run piece by piece
* iterations: mean over walker-ticks, mean of the per-tick maximum, the share of warm instances, statuses
* the two new launches alone at the batch on the 36-wide bucket, against their bytes at 6.3 TB/s

bench_fleet_warm.py [--batch 4096] [--ticks 48] [--windows 5] [--out profiles/fleet_warm_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-interface_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mpcasm import engine, problems  # noqa: E402
from mpcasm.walkers import WalkerFleet  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed_ticks(fleet, ticks):
    """Per-tick ms of ``ticks`` steps from rest, and iterations, statuses and warm flags (walker order)."""
    fleet.start_at_rest()
    torch.cuda.synchronize()
    marks = [ev() for _ in range(ticks + 1)]
    i32 = dict(dtype=torch.int32, device="cuda")
    iters, status = torch.zeros((ticks, fleet.batch), **i32), torch.zeros((ticks, fleet.batch), **i32)
    warm = torch.zeros((ticks, fleet.batch), **i32)
    marks[0].record()
    for t in range(ticks):
        out = fleet.step()
        marks[t + 1].record()
        for entry in out:      # (after the tick's last event: not in its time)
            idx = entry["index"].long()
            iters[t].index_copy_(0, idx, entry["iters"])
            status[t].index_copy_(0, idx, entry["status"])
            if "warm" in entry:
                warm[t].index_copy_(0, idx, entry["warm"])
    torch.cuda.synchronize()
    ms = [marks[t].elapsed_time(marks[t + 1]) for t in range(ticks)]
    return ms, iters.cpu().numpy(), status.cpu().numpy(), warm.cpu().numpy()


def window_summary(windows):
    means = [statistics.fmean(ms) for ms in windows]
    medians = [statistics.median(ms) for ms in windows]
    return {"tick_ms_mean": round(statistics.median(means), 4), "tick_ms_median": round(statistics.median(medians), 4),
            "windows_tick_ms_mean": [round(v, 4) for v in means],
            "windows_tick_ms_median": [round(v, 4) for v in medians]}


def split_cycle(fleet, ticks):
    """``ticks`` closed ticks made of the steps of WalkerFleet.step (each bucket's solve stage), with events between:
    per-tick ms of every piece (summed over the buckets)."""
    names = ["assemble", "warm_start", "solve", "store", "next_given"]
    parts = {k: [] for k in names}
    period = 2 * fleet.conf.step_samples
    for _ in range(ticks):
        marks = []
        given = fleet.given_buffer()
        for item in fleet._bucket_inputs():
            bucket = fleet.buckets[item["p"]]
            asm, stage, n = bucket["asm"], bucket["stage"], item["idx"].size
            e = [ev() for _ in range(6)]
            asm.bind_source(("steps", 0), item["E"])
            e[0].record()
            P, q, G, h = asm.assemble(given, count=n, index=item["index"], params=item["params"])
            e[1].record()
            stage.start(G[:n], h[:n], item.get("groups", ()), (item["key"] - 1) % period, index=item["index"], count=n)
            e[2].record()
            sol = stage.solve(P[:n], q[:n], G[:n], h[:n], count=n)
            e[3].record()
            if stage.warm:
                stage.store(sol, item["key"], index=item["index"])
            e[4].record()
            asm.next_given(given, sol.x, bucket["gmap"], index=item["index"], status=sol.status,
                           apply_mask=stage.apply_mask, count=n)
            e[5].record()
            marks.append(e)
        fleet.clock.tick()
        fleet._ticks += 1
        torch.cuda.synchronize()
        for i, k in enumerate(names):
            parts[k].append(sum(e[i].elapsed_time(e[i + 1]) for e in marks))
    return {k: {"ms_mean": round(statistics.fmean(v), 4), "ms_median": round(statistics.median(v), 4),
                "ms_max": round(max(v), 4)} for k, v in parts.items()}


def iteration_stats(iters, status, warm):
    codes, counts = np.unique(status, return_counts=True)
    return {"mean_over_walker_ticks": round(float(iters.mean()), 1),
            "mean_of_tick_max": round(float(iters.max(1).mean()), 1), "max": int(iters.max()),
            "warm_share": round(float(warm.mean()), 4),
            "warm_share_after_tick_0": round(float(warm[1:].mean()), 4),
            "statuses": {str(int(c)): int(k) for c, k in zip(codes, counts)},
            "per_tick_mean": [round(float(v), 1) for v in iters.mean(1)],
            "per_tick_max": [int(v) for v in iters.max(1)]}


def event_ms(fn, reps=50, runs=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = ev(), ev()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return {"ms": round(statistics.median(out), 4), "ms_min": round(min(out), 4), "ms_max": round(max(out), 4)}


def launches_alone(batch, no=36, nc=76):
    """The two launches at ``batch`` instances of the 36-wide bucket, every instance warm, a permuted index."""
    f = dict(dtype=torch.float64, device="cuda")
    G, h = torch.randn((batch, nc, no), **f), torch.randn((batch, nc), **f)
    store = engine.WarmStore(batch, no, nc, "cuda")
    x, y = torch.randn((batch, no), **f), torch.randn((batch, nc), **f)
    rho = torch.full((batch,), 0.5, **f)
    status = torch.ones(batch, dtype=torch.int32, device="cuda")
    index = torch.randperm(batch, device="cuda").to(torch.int32)
    ident = lambda n: torch.arange(n, dtype=torch.int32, device="cuda")
    cols, rows = ident(no), ident(nc)
    out = (torch.empty_like(x), torch.empty_like(y), torch.empty_like(y), torch.empty_like(rho),
           torch.empty_like(status))
    store_ms = event_ms(lambda: engine.warm_store_qp(store, (x, y, rho, status), 1, index=index))
    start_ms = event_ms(lambda: engine.warm_start_qp(store, G, h, cols, rows, 1, index=index, out=out))
    assert int(out[4].sum()) == batch
    store_bytes = batch * (2 * 8 * (no + nc) + 8 + 8 + 4 + 4 + 8)
    start_bytes = batch * (8 * nc * no + 8 * nc + 8 * (no + nc) + 8 + 8 + 4 + 8 * (no + 2 * nc) + 8 + 4)
    res = {}
    for name, ms, nbytes in (("warm_store", store_ms, store_bytes), ("warm_start", start_ms, start_bytes)):
        floor = nbytes / HBM_BYTES_PER_S * 1e3
        res[name] = dict(ms, bytes=nbytes, ms_at_6p3_TBps=round(floor, 5), times_floor=round(ms["ms"] / floor, 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=48)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_warm_bench.json"))
    a = ap.parse_args()
    conf = problems.BipedConfig(step_samples=8)
    cycle = 2 * conf.step_samples
    if a.ticks % cycle:
        raise SystemExit("--ticks: whole cycles of %d ticks (every window then starts at the same place)" % cycle)
    api = problems.load_api("mpc_interface")
    result = {"what": "WalkerFleet.step, warm=False against warm=True (start from the shifted last solution)",
              "batch": a.batch, "step_samples": conf.step_samples, "ticks": a.ticks, "windows": a.windows,
              "device": torch.cuda.get_device_name(),
              "cpu_projection": {"iterations_ratio": 0.17, "tick_ms": 1.0, "cold_tick_ms": 3.2}}
    for name, graphs in (("eager", False), ("graphs", True)):
        fleets = {"cold": WalkerFleet(a.batch, conf=conf, api=api, graphs=graphs, warm=False),
                  "warm": WalkerFleet(a.batch, conf=conf, api=api, graphs=graphs, warm=True)}
        for fleet in fleets.values():      # one cycle to compile kernels / capture graphs, the device warm
            fleet.start_at_rest()
            fleet.run(cycle)
        windows = {"cold": [], "warm": []}
        stats = {}
        for _ in range(a.windows):         # interleaved: cold, warm, cold, warm, ...
            for kind, fleet in fleets.items():
                ms, iters, status, warm = timed_ticks(fleet, a.ticks)
                windows[kind].append(ms)
                stats[kind] = iteration_stats(iters, status, warm)
        result[name] = {kind: window_summary(w) for kind, w in windows.items()}
        result[name]["warm_over_cold_mean"] = round(result[name]["warm"]["tick_ms_mean"] /
                                                    result[name]["cold"]["tick_ms_mean"], 3)
        result[name]["warm_over_cold_median"] = round(result[name]["warm"]["tick_ms_median"] /
                                                      result[name]["cold"]["tick_ms_median"], 3)
        if not graphs:
            result["iterations"] = stats
            result["iterations"]["warm_over_cold"] = round(stats["warm"]["mean_over_walker_ticks"] /
                                                           stats["cold"]["mean_over_walker_ticks"], 3)
            result["split_per_tick"] = {}
            for kind, fleet in fleets.items():
                fleet.start_at_rest()
                result["split_per_tick"][kind] = split_cycle(fleet, cycle)
    result["launches_alone"] = launches_alone(a.batch)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f)
        f.write("\n")
    short = dict(result)
    short["iterations"] = {k: ({kk: vv for kk, vv in v.items() if not kk.startswith("per_tick")}
                               if isinstance(v, dict) else v) for k, v in result["iterations"].items()}
    print(json.dumps(short))


if __name__ == "__main__":
    main()
