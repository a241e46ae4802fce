#!/usr/bin/env python3
"""Assembler.given_vjp and given_jvp (mpcasm_assemble_vjp, mpcasm_assemble_jvp) on 4 096 instances of the reduced biped
(N = 16; S, U shared, and once more with lti=["LIP"]: horizon tables generated on chip) and of C3 (problems.lipm3d),
with tools/bench_qp_sens.py's method: hipEvents around back-to-back calls on a warm device, each figure the median
(and min, max) of `--runs` windows of `--reps` calls.  Writes profiles/assemble_adjoint_bench.json and prints it as one
JSON line.  Nothing here is a gate: a new capability has no earlier figure to hold it to.

Per case the windows are INTERLEAVED in one process (vjp, jvp, preview_rows, the dense route, then again, `--runs`
times), so that a drift of the device's clock falls on all alike:

* given_vjp(gq, gh) and given_jvp(d) into fixed tensors
* preview_rows(given, optim) on the same plan: the yardstick -- the operator reads the sources, params and the
  cotangents once and writes ng (or no + nc) doubles per instance, so it should sit near two such launches
* the only route without these entries: asm.preview_matrices() (the dense [Mg | Mo] of every instance in memory) and
  two batched matrix-vector products over it, t = Mo gq and Mg' t -- the traffic of forming J' g from d_PM; the
  weights, schedules and arrows a caller would put between the two are left out, so this is a lower bound of the
  route.  A plan compiled with lti= has no preview matrices: no such line.

bench_assemble_adjoint.py [--batch 4096] [--reps 10] [--runs 5] [--cases biped,biped-lti,c3] [--out ...]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-interface_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mpcasm import engine, problems  # noqa: E402


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


def case(asm, given, dense, reps, runs):
    B, ng, no, nc = asm.batch, asm.ng, asm.no, asm.nc
    info = asm.adjoint_info()
    out = {"batch": B, "ng": ng, "no": no, "nc": nc, "preview_row_count": asm.plan.pmrows, "lds_bytes": info.lds,
           "workgroups_per_cu": info.per_cu, "index_words": info.index_words,
           "preview_route": list(asm.preview_route() or ())}
    gen = torch.Generator(device="cuda").manual_seed(5)
    f64 = dict(dtype=torch.float64, device="cuda")
    gq, gh = torch.randn((B, no), generator=gen, **f64), torch.randn((B, nc), generator=gen, **f64)
    d, optim = torch.randn((B, ng), generator=gen, **f64), torch.randn((B, no), generator=gen, **f64)
    gg, dq, dh = torch.zeros((B, ng), **f64), torch.zeros((B, no), **f64), torch.zeros((B, nc), **f64)
    rows = torch.zeros((B, asm.plan.pmrows), **f64)
    fns = {"given_vjp": lambda: asm.given_vjp(gq, gh, out=gg),
           "given_jvp": lambda: asm.given_jvp(d, out=(dq, dh)),
           "preview_rows": lambda: asm.preview_rows(given, optim, out=rows)}
    if dense:
        def through_pm():
            PM = asm.preview_matrices()
            t = torch.bmm(PM[:, :, ng:], gq.unsqueeze(2))
            return torch.bmm(PM[:, :, :ng].transpose(1, 2), t)

        fns["preview_matrices_and_products"] = through_pm
        out["preview_matrix_bytes"] = B * asm.plan.pmrows * (ng + no) * 8
    for fn in fns.values():                                      # (warm: every kernel has run)
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps))
    for k in fns:
        out[k] = spread(ms[k])
    out["vjp_over_preview_rows"] = round(out["given_vjp"]["ms"] / out["preview_rows"]["ms"], 3)
    out["jvp_over_preview_rows"] = round(out["given_jvp"]["ms"] / out["preview_rows"]["ms"], 3)
    if dense:
        out["dense_route_over_vjp"] = round(out["preview_matrices_and_products"]["ms"] / out["given_vjp"]["ms"], 2)
    return out


def clocks():
    try:
        text = subprocess.run(["rocm-smi", "--showclocks"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True,
                              timeout=20).stdout
        return [line.strip() for line in text.splitlines() if "sclk" in line or "mclk" in line][:4]
    except (OSError, subprocess.SubprocessError):
        return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cases", default="biped,biped-lti,c3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble_adjoint_bench.json"))
    a = ap.parse_args()
    cases = a.cases.split(",")
    api = problems.load_api("mpc_interface")
    rng = np.random.default_rng(31)
    props = torch.cuda.get_device_properties(0)
    result = {"what": "mpcasm_assemble_vjp, mpcasm_assemble_jvp", "device": torch.cuda.get_device_name(),
              "compute_units": props.multi_processor_count, "clocks": clocks(), "reps": a.reps, "runs": a.runs}
    for name in ("biped", "biped-lti"):
        if name in cases:
            form = problems.biped(api, problems.BipedConfig(step_samples=8), reduced=True)
            form.update(step_times=np.array([6, 14]), step_count=0)
            asm = engine.Assembler(form, batch=a.batch, lti=["LIP"] if name == "biped-lti" else ())
            given = torch.as_tensor(rng.normal(0, 0.05, [a.batch, form.given_len]), device="cuda")
            result["%s_%d" % (name, a.batch)] = case(asm, given, name == "biped", a.reps, a.runs)
            del asm
    if "c3" in cases:
        form = problems.lipm3d(api, N=32)
        given = rng.normal(0, 0.02, [a.batch, form.given_len])
        given[:, 6] += 0.85
        asm = engine.Assembler(form, batch=a.batch)
        result["c3_%d" % a.batch] = case(asm, torch.as_tensor(given, device="cuda"), True, a.reps, a.runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
