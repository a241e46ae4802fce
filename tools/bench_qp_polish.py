#!/usr/bin/env python3
"""mpcasm_qp_polish on 4 096 biped QPs (N = 16, 36 unknowns, 76 limits) taken from the closed loop of a fleet a
few ticks after a start in which the walkers stand slightly apart: hipEvents around back-to-back calls on a warm
device, each figure from `--runs` windows of `--reps` calls (median, min, max across the windows).  Writes
profiles/qp_polish_bench.json and prints it as one JSON line.

* the polish alone, on the iterates of a cold solve to 1e-3: every call starts from the same iterates, restored
  by device copies that are timed on their own and subtracted
* solve_qp to 1e-3 (OSQP's default); solve_qp to 1e-2 followed by the polish; solve_qp to 1e-3 followed by it
* for each of those and for the plain solve to 1e-2: the share DONE / REJECTED / SKIPPED and the median and the
  largest |x - x_tight|_inf over the instances, x_tight the same QP solved to 1e-9
* WalkerFleet.step at the same number of walkers with and without polish, eager and replayed from graphs

bench_qp_polish.py [--batch 4096] [--reps 20] [--runs 5] [--out profiles/qp_polish_bench.json]"""
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

from mpcasm import capi, engine, problems  # noqa: E402
from mpcasm.walkers import WalkerFleet  # noqa: E402


def event_ms(fn, reps, runs):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def spread(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def loop_qps(api, conf, batch):
    """``batch`` QPs of the 36-wide bucket, five closed ticks into the walk of a fleet large enough to hold them."""
    n = conf.step_samples
    walkers = -(-batch * n // (n - 1)) + n
    fleet = WalkerFleet(walkers, conf=conf, api=api)
    given = fleet.start_at_rest()
    rng = np.random.default_rng(8)
    given += torch.as_tensor(rng.normal(0.0, 2e-3, tuple(given.shape)), device=given.device)
    for _ in range(5):
        fleet.step()
    entry = max(fleet.tick(given), key=lambda e: e["P"].shape[0])
    assert entry["P"].shape[0] >= batch, (entry["P"].shape, batch)
    return tuple(entry[k][:batch].clone() for k in ("P", "q", "G", "h"))


def quality(x, tight, verdict=None):
    err = (x - tight).abs().amax(dim=1)
    ok = torch.isfinite(err)
    out = {"x_err_median": float(err[ok].median()), "x_err_max": float(err[ok].max())}
    if verdict is not None:
        n = verdict.numel()
        for name, code in (("done", capi.POLISH_DONE), ("rejected", capi.POLISH_REJECTED),
                           ("skipped", capi.POLISH_SKIPPED)):
            sel = verdict == code
            out[name] = round(int(sel.sum()) / n, 4)
            if int((sel & ok).sum()):
                out["x_err_median_" + name] = float(err[sel & ok].median())
    return out


def fleet_ms(api, conf, batch, polish, graphs, cycles=2):
    cycle = 2 * conf.step_samples
    fleet = WalkerFleet(batch, conf=conf, api=api, graphs=graphs, polish=polish)
    fleet.start_at_rest()
    for _ in range(cycle):            # kernels compiled, graphs captured; then from rest again
        fleet.step()
    fleet.start_at_rest()
    ticks = cycles * cycle
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(ticks + 1)]
    done = torch.zeros((), dtype=torch.int64, device="cuda")
    marks[0].record()
    for t in range(ticks):
        out = fleet.step()
        marks[t + 1].record()
        if polish:
            for entry in out:
                done += (entry["polish"] == capi.POLISH_DONE).sum()
    torch.cuda.synchronize()
    ms = [marks[t].elapsed_time(marks[t + 1]) for t in range(ticks)]
    res = {"ms_median": round(statistics.median(ms), 4), "ms_mean": round(statistics.fmean(ms), 4),
           "ms_max": round(max(ms), 4), "ticks": ticks}
    if polish:
        res["done_share"] = round(int(done) / (ticks * batch), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qp_polish_bench.json"))
    a = ap.parse_args()
    B = a.batch
    api = problems.load_api("mpc_interface")
    conf = problems.BipedConfig(step_samples=8)
    P, q, G, h = loop_qps(api, conf, B)
    no, nc = P.shape[1], G.shape[1]
    result = {"what": "mpcasm_qp_polish", "batch": B, "no": no, "nc": nc, "device": torch.cuda.get_device_name(),
              "lds_bytes_per_instance": engine.qp_polish_lds_bytes(no, nc),
              "solve_lds_bytes_per_instance": engine.qp_solve_lds_bytes(no, nc), "reps": a.reps, "runs": a.runs}
    tight = engine.solve_qp(P, q, G, h, eps_abs=1e-9, eps_rel=1e-9, max_iter=200000)
    result["tight_1e-9"] = {"solved": int((tight.status == engine.QP_SOLVED).sum()),
                            "iters_mean": round(float(tight.iters.double().mean()), 1), "iters_max": int(tight.iters.max())}

    def solve(eps, polish):
        return engine.solve_qp(P, q, G, h, eps_abs=eps, eps_rel=eps, polish=polish)

    for eps in (1e-3, 1e-2):
        plain, polished = solve(eps, False), solve(eps, True)
        tag = "%.0e" % eps
        result["solve_" + tag] = dict(
            spread(event_ms(lambda: solve(eps, False), a.reps, a.runs)), **quality(plain.x, tight.x),
            solved=int((plain.status == engine.QP_SOLVED).sum()), iters_mean=round(float(plain.iters.double().mean()), 1))
        result["solve_%s_then_polish" % tag] = dict(
            spread(event_ms(lambda: solve(eps, True), a.reps, a.runs)), **quality(polished.x, tight.x, polished.polish))
        active = ((h - plain.z) < plain.y).sum(dim=1).double()
        result["solve_" + tag]["active_rows_mean"] = round(float(active.mean()), 1)

    # the polish alone: from the same iterates every call
    sol = solve(1e-3, False)
    keep = [t.clone() for t in (sol.x, sol.y, sol.z)]
    work = [t.clone() for t in keep]
    verdict = torch.empty(B, dtype=torch.int32, device="cuda")
    res = torch.empty((B, 2), dtype=torch.float64, device="cuda")

    def restore():
        for w, k in zip(work, keep):
            w.copy_(k)

    def polish():
        restore()
        engine.polish_qp(P, q, G, h, work, status=sol.status, out=(verdict, res))

    copy_ms = event_ms(restore, a.reps, a.runs)
    pol_ms = event_ms(polish, a.reps, a.runs)
    result["polish_alone"] = dict(spread([p - statistics.median(copy_ms) for p in pol_ms]),
                                  restore_copies_ms=round(statistics.median(copy_ms), 4))
    for refine in (0, 3):
        def fixed():
            restore()
            engine.polish_qp(P, q, G, h, work, status=sol.status, refine_iters=refine, out=(verdict, res))
        ms = event_ms(fixed, a.reps, a.runs)
        result["polish_alone_refine_%d" % refine] = spread([p - statistics.median(copy_ms) for p in ms])

    result["fleet_step"] = {}
    for graphs in (False, True):
        for pol in (False, True):
            key = "%s%s" % ("graphs" if graphs else "eager", "_polish" if pol else "")
            result["fleet_step"][key] = fleet_ms(api, conf, B, pol, graphs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
