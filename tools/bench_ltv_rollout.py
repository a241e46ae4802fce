#!/usr/bin/env python3
"""The forward rollout of a plan compiled with ltv= (csrc/rollout.hip) on BASELINE config C5 -- problems.lipm_ltv,
N = 100, every instance its own (A_k, B_k) (problems.ltv_lipm_steps) -- at 2 048 and 16 384 instances, with
tools/bench_qp_solve_wide.py's hipEvent windows (median, min and max across `--runs` windows of `--reps`
back-to-back calls).  Writes profiles/ltv_rollout_bench.json and prints it as one JSON line.

Per batch size:
* `rollout` (Assembler.rollout: every preview row) and `advance` (Assembler.advance: the next given), each with
  the bytes the algorithm has to move -- (A_k, B_k), given and optim read once, the rows written once; for the
  advance A_0, B_0, the first sample of every input and the row of given -- and the time those bytes take at
  `hbm_bytes_per_s`, the achievable HBM rate the other bench files use;
* one LtvLoop.step() (window -> assemble -> solve_qp_wide, cold -> advance) and its parts timed on their own; the
  solver's status counts and iterations on the assembled C5 QPs are recorded as they come (no problem scaling:
  whether OSQP's iteration converges on them is a finding, not a gate).
At 2 048 only, in the same process: the route to the same rows without the rollout -- fill_su(ltv=True), a second
Assembler without ltv= with S, U bound per instance, preview_rows -- its time, the ratio, and the largest relative
difference between the two routes' rows.

bench_ltv_rollout.py [--reps 20] [--runs 5] [--batches 2048 16384] [--no-loop]"""
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
from mpcasm.ltv_loop import LtvLoop  # noqa: E402

HBM = 6.3e12
N, EXTRA_STEPS, DISTINCT = 100, 4, 64


def event_ms(fn, reps, runs, warm=2):
    for _ in range(warm):
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


def with_floor(ms, nbytes):
    floor = nbytes / HBM * 1e3
    return dict(spread(ms), algorithmic_bytes=int(nbytes), floor_ms=round(floor, 4),
                fraction_of_floor=round(floor / statistics.median(ms), 3))


def sequences(api, batch):
    """(batch, N + EXTRA_STEPS, 3, 3) and (..., 3, 1): DISTINCT different sequences, every instance its own copy."""
    T = N + EXTRA_STEPS
    seqs = [problems.ltv_lipm_steps(api, N=T, theta=2 * np.pi * i / DISTINCT) for i in range(DISTINCT)]
    A, B = np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs])
    reps = (batch + DISTINCT - 1) // DISTINCT
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(np.concatenate([v] * reps)[:batch]), device="cuda")
    return dev(A), dev(B)


def one_batch(api, form, batch, a, with_parent):
    out = {}
    A_seq, B_seq = sequences(api, batch)
    A, B = A_seq[:, :N].contiguous(), B_seq[:, :N].contiguous()
    rng = np.random.default_rng(17)
    given = torch.as_tensor(rng.normal(0, 0.02, [batch, form.given_len]), device="cuda")
    asm = engine.Assembler(form, batch=batch, ltv=["LIP"])
    asm.bind_ltv("LIP", A, B)
    n, m, axes, ng, no, pmrows = 3, 1, 2, asm.ng, asm.no, asm.plan.pmrows
    optim = torch.as_tensor(rng.normal(0, 0.1, [batch, no]), device="cuda")
    rows = torch.empty((batch, pmrows), dtype=torch.float64, device="cuda")
    out["sizes"] = dict(batch=batch, N=N, n=n, m=m, axes=axes, ng=ng, no=no, preview_rows=pmrows)
    out["rollout"] = with_floor(event_ms(lambda: asm.rollout(given, optim, out=rows), a.reps, a.runs),
                                8 * batch * (N * n * n + N * n * m + ng + no + pmrows))
    scratch = given.clone()
    out["advance"] = with_floor(event_ms(lambda: asm.advance(scratch, optim), a.reps, a.runs),
                                8 * batch * (n * n + n * m + axes * m + 2 * ng))
    if with_parent:
        plain = engine.Assembler(form, batch=batch)
        S = torch.empty((batch, N, n, n), dtype=torch.float64, device="cuda")
        U = torch.empty((batch, m, N, N, n), dtype=torch.float64, device="cuda")
        prow = torch.empty((batch, pmrows), dtype=torch.float64, device="cuda")

        def fill():
            engine.fill_su(A, B, N, ltv=True, out=(S, U))

        def preview():
            for j in range(m):
                plain.bind_source(("LIP", j), U[:, j], check=False)
            plain.bind_source(("LIP", m), S)
            plain.preview_rows(given, optim, out=prow)

        def route():
            fill()
            preview()

        ms = event_ms(route, a.reps, a.runs)
        asm.rollout(given, optim, out=rows)
        torch.cuda.synchronize()
        scale = rows.abs().amax(dim=0).clamp_min(1e-300)
        out["fill_su_then_preview_rows"] = dict(
            spread(ms), fill_su=spread(event_ms(fill, a.reps, a.runs)),
            preview_rows=spread(event_ms(preview, a.reps, a.runs)),
            workspace_bytes=int(8 * batch * (N * n * n + m * N * N * n)),
            rows_max_difference_relative_to_each_row_s_largest=float(((rows - prow).abs() / scale).max()))
        out["rollout_speedup_over_that_route"] = round(statistics.median(ms) / out["rollout"]["ms"], 2)
        del plain, S, U, prow
    if not a.no_loop:
        loop = LtvLoop(form, "LIP", batch, A_seq, B_seq)
        start = given.clone()

        def step():
            if loop.t >= loop.ticks_possible:
                loop.t = 0
                loop.given.copy_(start)
            return loop.step()

        loop.given.copy_(start)
        first = step()
        torch.cuda.synchronize()
        status = first["status"].cpu().numpy()
        iters = first["iters"].double()
        lp = {"status_counts_first_tick": {capi.QP_STATUS.get(int(s), str(int(s))): int((status == s).sum())
                                           for s in np.unique(status)},
              "iters_mean": round(float(iters.mean()), 1), "iters_max": int(iters.max())}
        reps, runs = (2, 2) if batch <= 4096 else (1, 1)
        lp["step"] = spread(event_ms(step, reps, runs, warm=0))
        lasm, stage = loop.asm, loop.stage
        lasm.bind_ltv_window("LIP", A_seq, B_seq, 0)
        P, q, G, h = lasm.assemble(start)
        lp["assemble"] = spread(event_ms(lambda: lasm.assemble(start), 5, 3))
        qp = stage.buffers

        def solve():
            stage.start(G, h, (), 0)
            stage.solve(P, q, G, h)

        lp["solve_qp_wide_cold"] = spread(event_ms(solve, reps, runs, warm=0))
        lp["advance"] = spread(event_ms(lambda: lasm.advance(scratch, qp["x"], status=qp["status"]), a.reps, a.runs))
        out["ltv_loop"] = lp
        del loop
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[2048, 16384])
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ltv_rollout_bench.json"))
    a = ap.parse_args()
    api = problems.load_api("mpc_interface")
    form = problems.lipm_ltv(api, N=N)
    result = {"what": "mpcasm_ltv_rollout / mpcasm_ltv_advance / LtvLoop.step on C5 (lipm_ltv, N = 100)",
              "reps": a.reps, "runs": a.runs, "hbm_bytes_per_s": HBM,
              "device": torch.cuda.get_device_name(0)}
    for batch in a.batches:
        result["c5_%d" % batch] = one_batch(api, form, batch, a, with_parent=batch == 2048)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
