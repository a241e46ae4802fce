#!/usr/bin/env python3
"""mpcasm_qp_sens on 4 096 biped QPs (N = 16, 36 unknowns, 76 limits, tools/bench_qp_polish.py's, from the closed loop
of a fleet) and mpcasm_qp_sens_wide on 4 096 C3 QPs (problems.lipm3d, 96 x 196, tools/bench_qp_polish_wide.py's), with
those tools' method: hipEvents around back-to-back calls on a warm device, each figure the median (and min, max) of
`--runs` windows of `--reps` calls.  Writes profiles/qp_sens_bench.json and prints it as one JSON line.  Nothing here
is a gate: a new capability has no earlier figure to hold it to.

Per case, on the iterates of solve_qp*(..., polish=True) and standard normal rx, ry, the windows INTERLEAVED in one
process (polish, sensitivity, sensitivity with the dense gradients, then the three again, `--runs` times), so that a
drift of the device's clock falls on all three alike:

* the polish alone on the iterates of the plain solve -- every call starts from the same iterates, restored by device
  copies that are timed on their own and subtracted
* qp_sensitivity* writing u, w, lres only; the same with gP and gG (want_P, want_G) into fixed tensors
* the shares DONE / SKIPPED / SINGULAR, the median and the largest lres over the DONE instances, the bytes of gP and
  gG a call writes, the LDS (and the workspace and workgroups of the wide entry)

bench_qp_sens.py [--batch 4096] [--reps 10] [--runs 5] [--cases biped,c3] [--out profiles/qp_sens_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-interface_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mpcasm import capi, engine, problems  # noqa: E402


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def case(P, q, G, h, wide, reps, runs):
    B, no, nc = P.shape[0], P.shape[1], G.shape[1]
    out = {"batch": B, "no": no, "nc": nc, "entry": "mpcasm_qp_sens_wide" if wide else "mpcasm_qp_sens"}
    kw = {}
    if wide:
        lds, work_bytes, groups = engine.qp_sens_wide_info(no, nc, B)
        out.update(lds_bytes_per_workgroup=lds, work_bytes=work_bytes, workgroups=groups)
        kw["work"] = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
    else:
        out["lds_bytes_per_instance"] = engine.qp_sens_lds_bytes(no, nc)
    solve = engine.solve_qp_wide if wide else engine.solve_qp
    polish_qp = engine.polish_qp_wide if wide else engine.polish_qp
    sens = engine.qp_sensitivity_wide if wide else engine.qp_sensitivity
    plain = solve(P, q, G, h)
    sol = solve(P, q, G, h, polish=True)
    out["solved"] = int((sol.status == engine.QP_SOLVED).sum())
    out["polished"] = int((sol.polish == capi.POLISH_DONE).sum())
    rng = torch.Generator(device="cuda").manual_seed(5)
    rx = torch.randn((B, no), dtype=torch.float64, device="cuda", generator=rng)
    ry = torch.randn((B, nc), dtype=torch.float64, device="cuda", generator=rng)
    f64 = dict(dtype=torch.float64, device="cuda")
    u, w, lres = torch.zeros((B, no), **f64), torch.zeros((B, nc), **f64), torch.zeros((B,), **f64)
    gP, gG = torch.zeros((B, no, no), **f64), torch.zeros((B, nc, no), **f64)
    verdict = torch.zeros((B,), dtype=torch.int32, device="cuda")
    out["dense_gradient_bytes"] = (gP.numel() + gG.numel()) * 8

    keep = [t.clone() for t in (plain.x, plain.y, plain.z)]
    iterate = [t.clone() for t in keep]
    pverdict = torch.empty(B, dtype=torch.int32, device="cuda")
    pres = torch.empty((B, 2), **f64)

    def restore():
        for a, k in zip(iterate, keep):
            a.copy_(k)

    def polish():
        restore()
        polish_qp(P, q, G, h, iterate, status=plain.status, out=(pverdict, pres), **kw)

    def lean():
        sens(P, G, h, sol, rx, ry, status=sol.status, out=(u, w, None, None, verdict, lres), **kw)

    def dense():
        sens(P, G, h, sol, rx, ry, status=sol.status, want_P=True, want_G=True, out=(u, w, gP, gG, verdict, lres), **kw)

    fns = {"restore_copies": restore, "polish_alone": polish, "sens": lean, "sens_dense": dense}
    for fn in fns.values():                                      # (warm: every kernel has run)
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps))
    copy_ms = statistics.median(ms["restore_copies"])
    out["polish_alone"] = dict(spread([p - copy_ms for p in ms["polish_alone"]]), restore_copies_ms=round(copy_ms, 4))
    out["sens"] = spread(ms["sens"])
    out["sens_dense"] = spread(ms["sens_dense"])
    out["sens_over_polish"] = round(out["sens"]["ms"] / out["polish_alone"]["ms"], 4)
    out["sens_dense_over_polish"] = round(out["sens_dense"]["ms"] / out["polish_alone"]["ms"], 4)
    out["dense_store_gb_per_s"] = round(out["dense_gradient_bytes"] / 1e6 /
                                        max(out["sens_dense"]["ms"] - out["sens"]["ms"], 1e-9), 1)
    n = verdict.numel()
    done = verdict == capi.SENS_DONE
    for name, code in (("done", capi.SENS_DONE), ("skipped", capi.SENS_SKIPPED), ("singular", capi.SENS_SINGULAR)):
        out[name] = round(int((verdict == code).sum()) / n, 4)
    if int(done.sum()):
        out["lres_median"], out["lres_max"] = float(lres[done].median()), float(lres[done].max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cases", default="biped,c3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qp_sens_bench.json"))
    a = ap.parse_args()
    cases = a.cases.split(",")
    api = problems.load_api("mpc_interface")
    result = {"what": "mpcasm_qp_sens, mpcasm_qp_sens_wide", "device": torch.cuda.get_device_name(), "reps": a.reps,
              "runs": a.runs}
    if "biped" in cases:
        from bench_qp_polish import loop_qps

        P, q, G, h = loop_qps(api, problems.BipedConfig(step_samples=8), a.batch)
        result["biped_%d" % a.batch] = case(P, q, G, h, False, a.reps, a.runs)
    if "c3" in cases:
        rng = np.random.default_rng(31)
        form = problems.lipm3d(api, N=32)
        given = rng.normal(0, 0.02, [a.batch, form.given_len])
        given[:, 6] += 0.85
        P, q, G, h = (t.clone() for t in engine.Assembler(form, batch=a.batch).assemble(given))
        result["c3_%d" % a.batch] = case(P, q, G, h, True, a.reps, a.runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
