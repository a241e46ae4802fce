#!/usr/bin/env python3
"""mpcasm_qp_solve_wide on the BASELINE shapes the LDS path refuses, with tools/bench_qp_solve.py's hipEvent
windows (median, min and max across `--runs` windows of `--reps` back-to-back calls).  Writes
profiles/qp_solve_wide_bench.json and prints it as one JSON line.

* C3 (problems.lipm3d, 96 x 196) at 4 096 instances from `assemble`: cold to 1e-3 and the warm next tick
  (a new `given`, K^-1 and rho kept; the restoring copies timed on their own and subtracted), with K^-1 in
  LDS and in d_kinv (MPCASM_QP_WIDE_KINV)
* C5-shaped QPs (200 x 404, random, solvable) at 2 048; C4's shape (384 x 1 536) at `--c4-batch`
* the biped (36 x 76) at 4 096 through the wide path and through solve_qp
Per case: mean and max iterations, the time per iteration of the batch (ms / max iterations: the batch runs as
long as its slowest instance) and the fraction of a streaming floor -- the bytes of G (plus K^-1 when it is
off chip) times the batch, read once per iteration at 6.3 TB/s (the achievable HBM rate).

bench_qp_solve_wide.py [--reps 5] [--runs 3] [--c4-batch 256]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-interface_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from mpcasm import engine, problems  # noqa: E402

HBM = 6.3e12


def event_ms(fn, reps, runs):
    for _ in range(2):
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


def figures(ms, sol, no, nc, batch, kinv_streamed):
    it = sol.iters.double()
    imax = max(int(it.max()), 1)
    per_iter = statistics.median(ms) / imax
    streamed = 8 * (nc * no + (no * no if kinv_streamed else 0)) * batch
    floor_ms = streamed / HBM * 1e3
    return dict(spread(ms), iters_mean=round(float(it.mean()), 1), iters_max=int(it.max()),
                solved=int((sol.status == engine.QP_SOLVED).sum()), ms_per_iter=round(per_iter, 5),
                floor_ms_per_iter=round(floor_ms, 5), fraction_of_floor=round(floor_ms / per_iter, 3))


def case(P, q, G, h, reps, runs, home, warm_given=None, asm=None):
    """cold (and, with asm, the warm next tick) with K^-1 in `home` ("lds", "global" or None: the default)."""
    if home is None:
        os.environ.pop("MPCASM_QP_WIDE_KINV", None)
    else:
        os.environ["MPCASM_QP_WIDE_KINV"] = home
    B, no, nc = P.shape[0], P.shape[1], G.shape[1]
    lds, on = engine.qp_solve_wide_info(no, nc)
    kinv = torch.empty((B, no, no), dtype=torch.float64, device="cuda")
    sol = engine.solve_qp_wide(P, q, G, h, kinv=kinv)
    out = {"kinv_on_chip": on, "lds_bytes_per_instance": lds,
           "cold_1e-3": figures(event_ms(lambda: engine.solve_qp_wide(P, q, G, h, kinv=kinv), reps, runs), sol,
                                no, nc, B, not on)}
    if asm is not None:
        rho = torch.full((B,), engine.OSQP_RHO, dtype=torch.float64, device="cuda")
        first = engine.solve_qp_wide(P, q, G, h, rho=rho, kinv=kinv)
        keep = [t.clone() for t in (first.x, first.y, first.z, rho, kinv)]
        P2, q2, G2, h2 = (t.clone() for t in asm.assemble(warm_given))
        work = [t.clone() for t in keep]

        def restore():
            for w, k in zip(work, keep):
                w.copy_(k)

        def warm():
            restore()
            return engine.solve_qp_wide(P2, q2, G2, h2, *work[:3], rho=work[3], kinv=work[4], kinv_valid=True)

        sol = warm()
        copy_ms = statistics.median(event_ms(restore, reps, runs))
        warm_ms = [w - copy_ms for w in event_ms(warm, reps, runs)]
        out["warm_next_tick"] = dict(figures(warm_ms, sol, no, nc, B, not on), restore_copies_ms=round(copy_ms, 4))
    os.environ.pop("MPCASM_QP_WIDE_KINV", None)
    return out


def random_batch(rng, B, no, nc):
    import osqp_restatement as rs

    qps = [rs.random_qp(rng, no, nc) for _ in range(min(B, 16))]
    P, q, G, h = (np.stack(a) for a in zip(*qps))
    reps = (B + len(qps) - 1) // len(qps)
    return [torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * reps)[:B]), device="cuda") for a in (P, q, G, h)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--c4-batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qp_solve_wide_bench.json"))
    a = ap.parse_args()
    api = problems.load_api("mpc_interface")
    result = {"what": "mpcasm_qp_solve_wide", "reps": a.reps, "runs": a.runs, "hbm_bytes_per_s": HBM}

    # C3 from the assembly
    B = 4096
    form = problems.lipm3d(api, N=32)
    rng = np.random.default_rng(31)
    given = rng.normal(0, 0.02, [B, form.given_len])
    given[:, 6] += 0.85
    asm = engine.Assembler(form, batch=B)
    P, q, G, h = (t.clone() for t in asm.assemble(given))
    nxt = given + rng.normal(0, 0.005, given.shape)
    result["c3_4096"] = {home: case(P, q, G, h, a.reps, a.runs, home, nxt, asm) for home in ("lds", "global")}
    result["c3_4096"]["default_kinv_on_chip"] = engine.qp_solve_wide_info(96, 196)[1]

    # C5-shaped and C4-shaped random QPs
    result["c5_shape_2048"] = case(*random_batch(rng, 2048, 200, 404), a.reps, a.runs, None)
    result["c4_shape_%d" % a.c4_batch] = case(*random_batch(rng, a.c4_batch, 384, 1536), 1, a.runs, None)

    # the biped through both paths
    bf = problems.biped(api, problems.BipedConfig(step_samples=8))
    bf.update(step_times=np.array([6, 14]), step_count=0)
    bg = np.random.default_rng(8).normal(0, 0.001, [B, bf.given_len])
    P, q, G, h = (t.clone() for t in engine.Assembler(bf, batch=B).assemble(bg))
    wide = case(P, q, G, h, a.reps, a.runs, None)
    sol = engine.solve_qp(P, q, G, h)
    lds_ms = event_ms(lambda: engine.solve_qp(P, q, G, h), a.reps, a.runs)
    result["biped_4096"] = {"solve_qp_wide": wide, "solve_qp": figures(lds_ms, sol, 36, 76, B, False)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
