#!/usr/bin/env python3
"""What steering costs a fleet (WalkerFleet(commands=True)) on one device: 4 096 biped walkers (phases b % 8),
the plain fleet and the steered one in the same process with interleaved windows, replayed from graphs.
hipEvents on the current stream; writes profiles/fleet_commands_bench.json and prints it as one JSON line.

* ms per assemble-only tick (WalkerFleet.tick on the fleet's own given buffer) and per closed tick with the warm
  start (WalkerFleet(warm=True).step), commands off and on: per window the mean and median over its ticks; the
  medians of the windows
* Assembler.apply_param_map alone on the 36-wide bucket at the batch (18 records, a permuted index, signs)
* the device memory the per-place cache holds in both modes (the tensors of WalkerFleet._cache, after a cycle)

bench_fleet_commands.py [--batch 4096] [--ticks 48] [--windows 5] [--out profiles/fleet_commands_bench.json]"""
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

from mpcasm import problems  # noqa: E402
from mpcasm.walkers import COMMAND_COLUMNS, WalkerFleet  # noqa: E402


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed(fleet, ticks, closed):
    """Per-tick ms of ``ticks`` ticks from rest."""
    given = fleet.start_at_rest()
    torch.cuda.synchronize()
    marks = [ev() for _ in range(ticks + 1)]
    marks[0].record()
    for t in range(ticks):
        if closed:
            fleet.step()
        else:
            fleet.tick(given)
        marks[t + 1].record()
    torch.cuda.synchronize()
    return [marks[t].elapsed_time(marks[t + 1]) for t in range(ticks)]


def window_summary(windows):
    means = [statistics.fmean(ms) for ms in windows]
    medians = [statistics.median(ms) for ms in windows]
    return {"tick_ms_mean": round(statistics.median(means), 4), "tick_ms_median": round(statistics.median(medians), 4),
            "windows_tick_ms_mean": [round(v, 4) for v in means],
            "windows_tick_ms_median": [round(v, 4) for v in medians]}


def cache_bytes(fleet):
    """Bytes of device memory in the fleet's per-place cache, by what they hold."""
    out = {}
    for entry in fleet._cache.values():
        for item in entry:
            for name, value in item.items():
                tensors = [value] if torch.is_tensor(value) else \
                    [t for group in value for t in group if torch.is_tensor(t)] if name == "groups" else []
                for t in tensors:
                    out[name] = out.get(name, 0) + t.numel() * t.element_size()
    out["total"] = sum(out.values())
    return out


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


def map_alone(fleet, batch):
    """apply_param_map at ``batch`` instances on the fleet's 36-wide bucket: eager calls back to back, and the same
    launch replayed from a graph of 20."""
    bucket = fleet.buckets[2]
    asm, pmap = bucket["asm"], bucket["pmap"]
    index = torch.randperm(batch, device="cuda").to(torch.int32)
    sign = torch.as_tensor(np.where(np.arange(batch) % 2, 1.0, -1.0), device="cuda")
    call = lambda: asm.apply_param_map(pmap, fleet.commands, index=index, sign=sign, count=batch)
    res = {"records": pmap.nrecs, "stores": batch * pmap.nrecs, "eager_call": event_ms(call)}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(20):
            call()
    per = event_ms(graph.replay, reps=10)
    res["in_a_graph_of_20"] = {k: round(v / 20, 5) for k, v in per.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=48)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_commands_bench.json"))
    a = ap.parse_args()
    conf = problems.BipedConfig(step_samples=8)
    cycle = 2 * conf.step_samples
    if a.ticks % cycle:
        raise SystemExit("--ticks: whole cycles of %d ticks (every window then starts at the same place)" % cycle)
    api = problems.load_api("mpc_interface")
    result = {"what": "WalkerFleet from graphs, commands=False (the per-place parameter clones) against "
                      "commands=True (one apply_param_map per bucket and tick)",
              "batch": a.batch, "step_samples": conf.step_samples, "ticks": a.ticks, "windows": a.windows,
              "device": torch.cuda.get_device_name(), "columns": list(COMMAND_COLUMNS)}
    steered = None
    for name, closed, kw in (("assemble_only_tick", False, {}), ("closed_tick_warm", True, {"warm": True})):
        fleets = {"plain": WalkerFleet(a.batch, conf=conf, api=api, graphs=True, **kw),
                  "commands": WalkerFleet(a.batch, conf=conf, api=api, graphs=True, commands=True, **kw)}
        for fleet in fleets.values():      # one cycle to compile kernels and capture the graphs
            timed(fleet, cycle, closed)
        windows = {kind: [] for kind in fleets}
        for _ in range(a.windows):         # interleaved: plain, commands, plain, commands, ...
            for kind, fleet in fleets.items():
                windows[kind].append(timed(fleet, a.ticks, closed))
        result[name] = {kind: window_summary(w) for kind, w in windows.items()}
        for stat in ("mean", "median"):
            result[name]["commands_minus_plain_us_" + stat] = round(
                1e3 * (result[name]["commands"]["tick_ms_" + stat] - result[name]["plain"]["tick_ms_" + stat]), 2)
        result[name]["cache_bytes"] = {kind: cache_bytes(fleet) for kind, fleet in fleets.items()}
        steered = fleets["commands"]
    result["apply_param_map_alone"] = map_alone(steered, a.batch)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
