#!/usr/bin/env python3
"""Pre-stabilised prediction (csrc/feedback.hip) on BASELINE config C5 -- problems.lipm_ltv, N = 100, every
instance its own (A_k, B_k) over T = 118 steps (problems.ltv_lipm_steps), the feedback of
problems.lipm_feedback_weights -- at 2 048 and 16 384 instances, with tools/bench_ltv_rollout.py's hipEvent
windows (median, min and max across `--runs` windows of `--reps` back-to-back calls, synchronised before and after).
Writes profiles/ltv_feedback_bench.json and prints it as one JSON line.

Per batch size:
* `ltv_lqr` over the whole sequence (once per loop) and `ltv_close` on its gains, each with the bytes it has to
  move and the time those take at `hbm_bytes_per_s`;
* `true_inputs` (every tick);
* one LtvLoop(feedback=...).step() and its parts -- assemble, cold solve_qp_wide, true_inputs, advance -- timed on
  their own, with the status histogram and the mean and largest iteration count of each of the first three ticks;
* beside them, unchanged, what profiles/ltv_rollout_bench.json records for the loop WITHOUT feedback: attempted
  factorisations (every instance NON_CVX after no iteration), quoted for the reader and not a gate.

bench_ltv_feedback.py [--reps 20] [--runs 5] [--batches 2048 16384]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-interface_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mpcasm import capi, engine, problems  # noqa: E402
from mpcasm.ltv_loop import LtvLoop  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ltv_rollout import HBM, event_ms, spread, with_floor  # noqa: E402

N, T, DISTINCT = 100, 118, 64
OPEN_LOOP_STEP_MS = {2048: 45.14, 16384: 336.3}     # profiles/ltv_rollout_bench.json: c5_*.ltv_loop.step.ms


def sequences(api, batch):
    """(batch, T, 3, 3) and (batch, T, 3, 1): DISTINCT different sequences, every instance its own copy."""
    seqs = [problems.ltv_lipm_steps(api, N=T, theta=2 * np.pi * i / DISTINCT) for i in range(DISTINCT)]
    A, B = np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs])
    reps = (batch + DISTINCT - 1) // DISTINCT
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(np.concatenate([v] * reps)[:batch]), device="cuda")
    return dev(A), dev(B)


def tick_stats(out):
    status = out["status"].cpu().numpy()
    iters = out["iters"].double()
    return {"status_counts": {capi.QP_STATUS.get(int(s), str(int(s))): int((status == s).sum())
                              for s in np.unique(status)},
            "iters_mean": round(float(iters.mean()), 1), "iters_max": int(iters.max())}


def one_batch(api, form, batch, a):
    out = {}
    n, m, axes = 3, 1, 2
    A_seq, B_seq = sequences(api, batch)
    Q, R = problems.lipm_feedback_weights()
    Qd, Rd = torch.as_tensor(Q, device="cuda"), torch.as_tensor(R, device="cuda")
    K_seq, Acl_seq, info = engine.ltv_lqr(A_seq, B_seq, Qd, Rd)
    assert int((info >= 0).sum()) == 0
    out["sizes"] = dict(batch=batch, N=N, T=T, n=n, m=m, axes=axes)
    out["ltv_lqr"] = with_floor(event_ms(lambda: engine.ltv_lqr(A_seq, B_seq, Qd, Rd), a.reps, a.runs),
                                8 * batch * T * (2 * n * n + 2 * n * m))
    out["ltv_close"] = with_floor(event_ms(lambda: engine.ltv_close(A_seq, B_seq, K_seq), a.reps, a.runs),
                                  8 * batch * T * (2 * n * n + 2 * n * m))
    rng = np.random.default_rng(17)
    start = torch.as_tensor(rng.normal(0, 0.02, [batch, form.given_len]), device="cuda")
    loop = LtvLoop(form, "LIP", batch, A_seq, B_seq, feedback={"Q": Qd, "R": Rd})
    loop.given.copy_(start)
    ticks = []
    for _ in range(3):
        ticks.append(tick_stats(loop.step()))
    torch.cuda.synchronize()
    lp = {"first_three_ticks": ticks}

    def step():
        if loop.t >= loop.ticks_possible:
            loop.t = 0
            loop.given.copy_(start)
        return loop.step()

    reps, runs = (2, a.runs) if batch <= 4096 else (1, a.runs)
    lp["step"] = spread(event_ms(step, reps, runs, warm=1))
    lasm, stage = loop.asm, loop.stage
    lasm.bind_ltv_window("LIP", loop.A_cl_seq, B_seq, 0)
    P, q, G, h = lasm.assemble(start)
    lp["assemble"] = spread(event_ms(lambda: lasm.assemble(start), 5, a.runs))
    qp = stage.buffers

    def solve():
        stage.start(G, h, (), 0)
        stage.solve(P, q, G, h)

    lp["solve_qp_wide_cold"] = spread(event_ms(solve, reps, runs, warm=1))
    u = torch.empty((batch, axes, N, m), dtype=torch.float64, device="cuda")
    out["true_inputs"] = with_floor(
        event_ms(lambda: lasm.true_inputs(K_seq, 0, start, qp["x"], out=u), a.reps, a.runs),
        8 * batch * (N * (n * n + n * m + m * n) + lasm.ng + lasm.no + axes * N * m))
    lp["true_inputs"] = {k: out["true_inputs"][k] for k in ("ms", "ms_min", "ms_max")}
    scratch = start.clone()
    lp["advance"] = spread(event_ms(lambda: lasm.advance(scratch, qp["x"], status=qp["status"]), a.reps, a.runs))
    lp["open_loop_step_ms_in_ltv_rollout_bench"] = OPEN_LOOP_STEP_MS.get(batch)
    out["ltv_loop_with_feedback"] = lp
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[2048, 16384])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ltv_feedback_bench.json"))
    a = ap.parse_args()
    api = problems.load_api("mpc_interface")
    form = problems.lipm_ltv(api, N=N)
    result = {"what": "mpcasm_ltv_lqr / mpcasm_ltv_close / mpcasm_ltv_true_inputs / LtvLoop(feedback=).step on C5 "
                      "(lipm_ltv, N = 100, T = 118)",
              "reps": a.reps, "runs": a.runs, "hbm_bytes_per_s": HBM, "device": torch.cuda.get_device_name(0),
              "open_loop_note": "open_loop_step_ms_in_ltv_rollout_bench: the loop without feedback, every instance "
                                "NON_CVX after 0 iterations -- attempted factorisations, quoted, not a gate"}
    for batch in a.batches:
        result["c5_%d" % batch] = one_batch(api, form, batch, a)
        torch.cuda.empty_cache()
        print("c5_%d measured" % batch, file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
