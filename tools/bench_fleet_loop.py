#!/usr/bin/env python3
"""The closed walking loop of a fleet (WalkerFleet.step: assemble, cold solve to 1e-3, next `given`) on one
device: 4 096 biped walkers (phases b % 8) from rest, three cycles of the fleet's 2 * step_samples places
(48 ticks), eager and replayed from graphs.  hipEvents on the current stream; writes
profiles/fleet_loop_bench.json and prints it as one JSON line.

* ms per closed tick: every tick timed on its own (median, mean, max) and the whole run
* the split of a tick between assembly, solve and next_given (events between them, per bucket, summed per
  tick), over one more cycle run piece by piece
* iterations per tick: mean, median and max over the walkers, and the tick whose slowest walker is slowest
* next_given against preview_rows on the 36-wide bucket at the same batch (it evaluates a subset of the
  same rows and writes 8 of 40 columns in place)

bench_fleet_loop.py [--batch 4096] [--cycles 3] [--out profiles/fleet_loop_bench.json]"""
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


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed_ticks(fleet, ticks):
    """Per-tick ms of ``ticks`` steps, and the iteration counts of each (walker order)."""
    marks = [ev() for _ in range(ticks + 1)]
    iters = torch.zeros((ticks, fleet.batch), dtype=torch.int32, device="cuda")
    status = torch.zeros((ticks, fleet.batch), dtype=torch.int32, device="cuda")
    marks[0].record()
    for t in range(ticks):
        out = fleet.step()
        marks[t + 1].record()
        for entry in out:      # (after the tick's last event: not in its time)
            idx = entry["index"].long()
            iters[t].index_copy_(0, idx, entry["iters"])
            status[t].index_copy_(0, idx, entry["status"])
    torch.cuda.synchronize()
    ms = [marks[t].elapsed_time(marks[t + 1]) for t in range(ticks)]
    return ms, iters.cpu().numpy(), status.cpu().numpy()


def summary(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_mean": round(statistics.fmean(ms), 4),
            "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "ms_total": round(sum(ms), 3)}


def split_cycle(fleet, ticks):
    """``ticks`` closed ticks made of the steps of WalkerFleet.step (each bucket's solve stage), with events between:
    per-tick ms of assembly, solve and next_given (summed over the buckets)."""
    parts = {"assemble": [], "solve": [], "next_given": []}
    for _ in range(ticks):
        marks = []
        given = fleet.given_buffer()
        for item in fleet._bucket_inputs():
            bucket = fleet.buckets[item["p"]]
            asm, stage, n = bucket["asm"], bucket["stage"], item["idx"].size
            e = [ev() for _ in range(4)]
            asm.bind_source(("steps", 0), item["E"])
            e[0].record()
            P, q, G, h = asm.assemble(given, count=n, index=item["index"], params=item["params"])
            e[1].record()
            stage.start(G[:n], h[:n], (), 0, count=n)
            sol = stage.solve(P[:n], q[:n], G[:n], h[:n], count=n)
            e[2].record()
            asm.next_given(given, sol.x, bucket["gmap"], index=item["index"], status=sol.status,
                           apply_mask=stage.apply_mask, count=n)
            e[3].record()
            marks.append(e)
        fleet.clock.tick()
        fleet._ticks += 1
        torch.cuda.synchronize()
        for k, (a, b) in zip(parts, ((0, 1), (1, 2), (2, 3))):
            parts[k].append(sum(e[a].elapsed_time(e[b]) for e in marks))
    return {k: {"ms_mean": round(statistics.fmean(v), 4), "ms_median": round(statistics.median(v), 4),
                "ms_max": round(max(v), 4)} for k, v in parts.items()}


def iteration_stats(iters, status):
    per_tick = [{"tick": t, "mean": round(float(it.mean()), 1), "median": float(np.median(it)),
                 "max": int(it.max()), "unsolved": int((st != engine.QP_SOLVED).sum())}
                for t, (it, st) in enumerate(zip(iters, status))]
    worst = max(per_tick, key=lambda r: r["max"])
    return {"mean_over_all": round(float(iters.mean()), 1), "mean_of_tick_max": round(float(iters.max(1).mean()), 1),
            "max": int(iters.max()), "worst_tick": worst, "per_tick": per_tick}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_loop_bench.json"))
    a = ap.parse_args()
    conf = problems.BipedConfig(step_samples=8)
    cycle = 2 * conf.step_samples
    ticks = a.cycles * cycle
    api = problems.load_api("mpc_interface")
    result = {"what": "WalkerFleet.step (assemble + cold solve_qp to 1e-3 + next_given)", "batch": a.batch,
              "step_samples": conf.step_samples, "ticks": ticks, "device": torch.cuda.get_device_name()}

    for name, graphs in (("eager", False), ("graphs", True)):
        fleet = WalkerFleet(a.batch, conf=conf, api=api, graphs=graphs)
        # one cycle to compile kernels / capture graphs; then from rest again (a whole cycle later every
        # walker is at the same place of its step cycle, with two more steps counted: the same QPs)
        fleet.start_at_rest()
        fleet.run(cycle)
        fleet.start_at_rest()
        ms, iters, status = timed_ticks(fleet, ticks)
        result[name] = summary(ms)
        result[name]["per_tick_ms"] = [round(x, 4) for x in ms]
        if not graphs:
            result["iterations"] = iteration_stats(iters, status)
            result["split_per_tick"] = split_cycle(fleet, cycle)
            # next_given against preview_rows on the 36-wide bucket, all walkers, same batch
            bucket = fleet.buckets[max(fleet.buckets)]
            asm = bucket["asm"]
            g = fleet.given_buffer().clone()
            x = torch.randn((a.batch, asm.no), dtype=torch.float64, device="cuda") * 0.1
            index = torch.randperm(a.batch, device="cuda").to(torch.int32)
            status_all = torch.ones(a.batch, dtype=torch.int32, device="cuda")
            rows = torch.empty((a.batch, asm.plan.pmrows), dtype=torch.float64, device="cuda")
            result["next_given_vs_preview_rows"] = {
                "no": asm.no, "mapped_columns": int((bucket["gmap"].rows >= 0).sum()),
                "constant_columns": int((bucket["gmap"].rows == -2).sum()), "preview_rows": asm.plan.pmrows,
                "preview_rows_ms": event_ms(lambda: asm.preview_rows(g, x, out=rows)),
                "next_given_ms": event_ms(lambda: asm.next_given(g, x, bucket["gmap"], index=index,
                                                                 status=status_all))}
    result["graphs_over_eager"] = round(result["graphs"]["ms_mean"] / result["eager"]["ms_mean"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f)
        f.write("\n")
    short = {k: v for k, v in result.items() if k not in ("iterations",)}
    for k in ("eager", "graphs"):
        short[k] = {kk: vv for kk, vv in result[k].items() if kk != "per_tick_ms"}
    short["iterations"] = {k: v for k, v in result["iterations"].items() if k != "per_tick"}
    print(json.dumps(short))


if __name__ == "__main__":
    main()
