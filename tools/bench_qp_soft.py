#!/usr/bin/env python3
"""Soft limits in the QP solvers, measured: writes profiles/qp_soft_bench.json (and prints it as one JSON line).
Every comparison is in this one process on one device; nothing here is a gate.

* per iteration, at 4 096 biped QPs (36 x 76, mpcasm_qp_solve*) and 4 096 C3 QPs (96 x 196, mpcasm_qp_solve_wide*)
  straight out of mpcasm_assemble, all four eps 0, rho fixed, `--iters` iterations with a check every 25: the soft
  entry with every row soft, the soft entry with every lin = +inf, the hard entry.  hipEvents around `--reps`
  back-to-back calls, `--runs` windows, taken in turn (soft, all-inf, hard, soft, ...) so that drift falls on all
  three alike; median, min and max across the windows
* with `--parent-lib PATH` (a libmpcasm.so built from the parent commit): the hard entries of this build against
  the parent's on the same tensors, windows alternating; the expectation is "inside the run-to-run spread", which
  is recorded next to it
* WalkerFleet.step from rest for 48 ticks, with and without soft=(1e3, 0): statuses per tick, the iterations of
  the slowest walker and ms per tick (a synchronize per tick: the launch overhead is in both)

bench_qp_soft.py [--batch 4096] [--iters 200] [--reps 5] [--runs 5] [--ticks 48] [--parent-lib PATH]"""
import argparse
import ctypes
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


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def in_turn(fns, reps, runs):
    """``{name: [ms per call, one per window]}``, the windows of the variants taken in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            out[name].append(window_ms(fn, reps))
    return out


def spread(ms, iters):
    us = [1e3 * m / iters for m in ms]
    return {"us_per_iter": round(statistics.median(us), 3), "us_min": round(min(us), 3), "us_max": round(max(us), 3),
            "ms_per_call": round(statistics.median(ms), 4)}


def raw_hard(lib, entry, P, q, G, h, iters, kinv):
    """The hard entry ``entry`` of ``lib`` (this build's or the parent's) on fixed buffers, through ctypes."""
    B, no, nc = P.shape[0], P.shape[1], G.shape[1]
    f, i32 = dict(dtype=torch.float64, device=P.device), dict(dtype=torch.int32, device=P.device)
    x, y, z = torch.empty((B, no), **f), torch.empty((B, nc), **f), torch.empty((B, nc), **f)
    rho, res = torch.empty(B, **f), torch.empty((B, 2), **f)
    status, its = torch.empty(B, **i32), torch.empty(B, **i32)
    fn = getattr(lib, entry)
    fn.restype, fn.argtypes = capi.SIGNATURES[entry]

    def call():
        rho.fill_(engine.OSQP_RHO)
        rc = fn(no, nc, P.data_ptr(), q.data_ptr(), G.data_ptr(), h.data_ptr(), x.data_ptr(), y.data_ptr(),
                z.data_ptr(), 0, rho.data_ptr(), engine.OSQP_SIGMA, engine.OSQP_ALPHA, 0.0, 0.0, 0.0, 0.0, iters, 25,
                0, status.data_ptr(), its.data_ptr(), res.data_ptr(), B, kinv.data_ptr() if kinv is not None else None,
                0, None)
        assert rc == 0, rc
        return x
    return call


def per_iteration(name, solve, entry, P, q, G, h, a, parent):
    n = a.iters
    fixed = dict(eps_abs=0.0, eps_rel=0.0, eps_prim_inf=0.0, eps_dual_inf=0.0, max_iter=n, check_every=25,
                 adaptive_rho_interval=0)
    nc, dev = G.shape[1], P.device
    f = dict(dtype=torch.float64, device=dev)
    soft = (torch.full((nc,), 1e3, **f), torch.zeros(nc, **f))
    hard_rows = (torch.full((nc,), float("inf"), **f), torch.zeros(nc, **f))
    kinv = torch.empty(tuple(P.shape), **f)
    ms = in_turn({"soft_all_rows_soft": lambda: solve(P, q, G, h, kinv=kinv, soft=soft, **fixed),
                  "soft_all_rows_inf": lambda: solve(P, q, G, h, kinv=kinv, soft=hard_rows, **fixed),
                  "hard": lambda: solve(P, q, G, h, kinv=kinv, **fixed)}, a.reps, a.runs)
    out = {"what": name, "batch": P.shape[0], "no": P.shape[1], "nc": nc, "iters": n}
    out.update({k: spread(v, n) for k, v in ms.items()})
    if parent is not None:
        here, there = raw_hard(capi.load(), entry, P, q, G, h, n, kinv), raw_hard(parent, entry, P, q, G, h, n, kinv)
        assert torch.equal(here().clone(), there().clone()), "the hard entry's iterates moved"
        ms = in_turn({"this_build": here, "parent": there}, a.reps, a.runs)
        out["hard_entry_against_parent"] = {k: spread(v, n) for k, v in ms.items()}
        out["hard_entry_against_parent"]["ratio_of_medians"] = round(
            statistics.median(ms["this_build"]) / statistics.median(ms["parent"]), 4)
        out["hard_entry_against_parent"]["iterates_bit_equal"] = True
    return out


def fleet_from_rest(B, ticks, soft):
    fleet = WalkerFleet(B, conf=problems.BipedConfig(step_samples=8), soft=soft)
    fleet.start_at_rest()
    rows = []
    for _ in range(ticks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fleet.step()
        e1.record()
        torch.cuda.synchronize()
        status = torch.cat([o["status"] for o in out]).cpu().numpy()
        iters = torch.cat([o["iters"] for o in out]).cpu().numpy()
        codes, counts = np.unique(status, return_counts=True)
        rows.append({"ms": round(e0.elapsed_time(e1), 3), "iters_max": int(iters.max()),
                     "status": {capi.QP_STATUS.get(int(c), str(int(c))): int(k) for c, k in zip(codes, counts)}})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=48)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qp_soft_bench.json"))
    a = ap.parse_args()
    B = a.batch
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    api = problems.load_api("mpc_interface")
    rng = np.random.default_rng(8)
    result = {"what": "soft limits in mpcasm_qp_solve*", "device": torch.cuda.get_device_name(0), "reps": a.reps,
              "runs": a.runs, "lds_bytes_per_instance": {
                  "biped_hard": engine.qp_solve_lds_bytes(36, 76),
                  "biped_soft": engine.qp_solve_soft_lds_bytes(36, 76),
                  "c3_hard": engine.qp_solve_wide_info(96, 196)[0],
                  "c3_soft": engine.qp_solve_wide_soft_info(96, 196)[0]}}

    form = problems.biped(api, problems.BipedConfig(step_samples=8))
    form.update(step_times=np.array([6, 14]), step_count=0)
    given = rng.normal(0, 0.001, [B, form.given_len])
    P, q, G, h = (t.clone() for t in engine.Assembler(form, batch=B).assemble(given))
    result["biped"] = per_iteration("mpcasm_qp_solve[_soft]", engine.solve_qp, "mpcasm_qp_solve", P, q, G, h, a, parent)

    form = problems.lipm3d(api, N=32)
    given = rng.normal(0, 0.02, [B, form.given_len])
    given[:, 6] += 0.85
    P, q, G, h = (t.clone() for t in engine.Assembler(form, batch=B).assemble(given))
    result["c3"] = per_iteration("mpcasm_qp_solve_wide[_soft]", engine.solve_qp_wide, "mpcasm_qp_solve_wide", P, q, G,
                                 h, a, parent)

    result["fleet_from_rest"] = {"batch": B, "ticks": a.ticks, "hard": fleet_from_rest(B, a.ticks, None),
                                 "soft_1e3_0": fleet_from_rest(B, a.ticks, (1e3, 0.0))}
    text = json.dumps(result)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
