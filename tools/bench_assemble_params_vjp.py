#!/usr/bin/env python3
"""Assembler.params_vjp (mpcasm_assemble_params_vjp) on 4 096 instances of the reduced biped (N = 16; S, U shared, and
once more with lti=["LIP"]: horizon tables generated on chip) and of C3 (problems.lipm3d), with
tools/bench_assemble_adjoint.py's method: hipEvents around back-to-back calls on a warm device, each figure the median
(and min, max) of `--runs` windows of `--reps` calls.  Writes profiles/assemble_params_adjoint_bench.json and prints it
as one JSON line.  Nothing here is a gate: a new capability has no earlier figure to hold it to.

The expectation, stated before the run: params_vjp makes three forward row passes (V_o x, V_o u, V_g given) and a
short gather where given_vjp makes one forward and one transposed pass, so it should land within a small multiple of
given_vjp -- and far below what the dense route pays for merely WRITING dL/dP and dL/dG, before anything contracts
them with the assembly.

Per case, on the polished solutions of solve_qp*(assemble(given), polish=True) and a standard normal loss gradient,
the windows are INTERLEAVED in one process (`--runs` times round the list), so that a drift of the device's clock
falls on all alike:

* params_vjp(given, x, u, y . active, w, verdict) into a fixed tensor
* given_vjp(-u, w) on the same plan
* qp_sensitivity*(want_P=True, want_G=True) and the same with want_*=False: their difference is the cost of writing
  the dense gradients
* asm.preview_matrices(): the dense [Mg | Mo] a contraction of those gradients would have to read.  A plan compiled
  with lti= has no preview matrices: no such line.

bench_assemble_params_vjp.py [--batch 4096] [--reps 10] [--runs 5] [--cases biped,biped-lti,c3] [--out ...]"""
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


def case(asm, given, wide, dense, reps, runs):
    B, ng, no, nc = asm.batch, asm.ng, asm.no, asm.nc
    info, ginfo = asm.params_adjoint_info(), asm.adjoint_info()
    out = {"batch": B, "ng": ng, "no": no, "nc": nc, "n_params": int(asm.params.shape[1]), "lds_bytes": info.lds,
           "workgroups_per_cu": info.per_cu, "index_words": info.index_words, "given_vjp_lds_bytes": ginfo.lds,
           "given_vjp_workgroups_per_cu": ginfo.per_cu}
    P, q, G, h = (t.clone() for t in asm.assemble(given))
    solve = engine.solve_qp_wide if wide else engine.solve_qp
    sens = engine.qp_sensitivity_wide if wide else engine.qp_sensitivity
    kw = {}
    if wide:
        _, work_bytes, _ = engine.qp_sens_wide_info(no, nc, B)
        kw["work"] = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
    sol = solve(P, q, G, h, polish=True)
    gen = torch.Generator(device="cuda").manual_seed(5)
    f64 = dict(dtype=torch.float64, device="cuda")
    rx, ry = torch.randn((B, no), generator=gen, **f64), torch.randn((B, nc), generator=gen, **f64)
    u, w, lres = torch.zeros((B, no), **f64), torch.zeros((B, nc), **f64), torch.zeros((B,), **f64)
    gP, gG = torch.zeros((B, no, no), **f64), torch.zeros((B, nc, no), **f64)
    verdict = torch.zeros((B,), dtype=torch.int32, device="cuda")
    out["dense_gradient_bytes"] = (gP.numel() + gG.numel()) * 8

    def lean():
        sens(P, G, h, sol, rx, ry, status=sol.status, out=(u, w, None, None, verdict, lres), **kw)

    def with_dense():
        sens(P, G, h, sol, rx, ry, status=sol.status, want_P=True, want_G=True, out=(u, w, gP, gG, verdict, lres), **kw)

    lean()
    torch.cuda.synchronize()
    out["sens_done"] = round(int((verdict == capi.SENS_DONE).sum()) / B, 4)
    y = sol.y * ((h - sol.z) < sol.y)
    minus_u = -u
    gp, gg = torch.zeros((B, out["n_params"]), **f64), torch.zeros((B, ng), **f64)
    fns = {"params_vjp": lambda: asm.params_vjp(given, sol.x, u, y, w, verdict=verdict, out=gp),
           "given_vjp": lambda: asm.given_vjp(minus_u, w, out=gg),
           "sens": lean, "sens_dense": with_dense}
    if dense:
        fns["preview_matrices"] = asm.preview_matrices
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
    writes = out["sens_dense"]["ms"] - out["sens"]["ms"]
    out["dense_writes_ms"] = round(writes, 4)
    out["params_vjp_over_given_vjp"] = round(out["params_vjp"]["ms"] / out["given_vjp"]["ms"], 3)
    out["dense_writes_over_params_vjp"] = round(writes / out["params_vjp"]["ms"], 2)
    if dense:
        out["preview_matrices_over_params_vjp"] = round(out["preview_matrices"]["ms"] / out["params_vjp"]["ms"], 2)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble_params_adjoint_bench.json"))
    a = ap.parse_args()
    cases = a.cases.split(",")
    api = problems.load_api("mpc_interface")
    rng = np.random.default_rng(31)
    props = torch.cuda.get_device_properties(0)
    result = {"what": "mpcasm_assemble_params_vjp", "device": torch.cuda.get_device_name(),
              "compute_units": props.multi_processor_count, "clocks": clocks(), "reps": a.reps, "runs": a.runs}
    for name in ("biped", "biped-lti"):
        if name in cases:
            form = problems.biped(api, problems.BipedConfig(step_samples=8), reduced=True)
            form.update(step_times=np.array([6, 14]), step_count=0)
            asm = engine.Assembler(form, batch=a.batch, lti=["LIP"] if name == "biped-lti" else ())
            given = torch.as_tensor(rng.normal(0, 0.01, [a.batch, form.given_len]), device="cuda")
            result["%s_%d" % (name, a.batch)] = case(asm, given, False, name == "biped", a.reps, a.runs)
            del asm
    if "c3" in cases:
        form = problems.lipm3d(api, N=32)
        given = rng.normal(0, 0.02, [a.batch, form.given_len])
        given[:, 6] += 0.85
        asm = engine.Assembler(form, batch=a.batch)
        result["c3_%d" % a.batch] = case(asm, torch.as_tensor(given, device="cuda"), True, True, a.reps, a.runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
