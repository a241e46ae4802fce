#!/usr/bin/env python3
"""Limits and costs on the true input of a pre-stabilised plan (mpcasm_ltv_augment, LtvLoop(true_input=True)) on
BASELINE config C5 -- N = 100, every instance its own (A_k, B_k) over T = 118 steps, the feedback of
problems.lipm_feedback_weights -- at 2 048 and 16 384 instances, in one process, every shape run before it is
timed, with tools/bench_ltv_rollout.py's hipEvent windows (median, min and max across `--runs` windows of `--reps`
back-to-back calls).  Writes profiles/ltv_true_input_bench.json and prints it as one JSON line.

Per batch size:
* `ltv_augment` alone beside `ltv_close`, each with the bytes it has to move and the time those take at
  `hbm_bytes_per_s`;
* `assemble` of the 4-state plan (problems.lipm_ltv_true_input, input limit 0.1: 804 rows, the sweep kernel's
  generic instantiation) beside the 3-state plan of the loop without `true_input` (problems.lipm_ltv: 404 rows);
* LtvLoop(feedback=, true_input=True).step() with the limit beside LtvLoop(feedback=).step(), the same plants, gains
  and initial states: the step, and the status histogram and iteration counts of each of the first three ticks.

Nothing here is a gate.

bench_ltv_true_input.py [--reps 20] [--runs 5] [--batches 2048 16384]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-interface_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mpcasm import engine, problems  # noqa: E402
from mpcasm.ltv_loop import LtvLoop  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ltv_feedback import N, T, sequences, tick_stats  # noqa: E402
from bench_ltv_rollout import HBM, event_ms, spread, with_floor  # noqa: E402

LIMIT = 0.1


def loop_figures(loop, start, window, a, batch):
    """The first three ticks' statistics, the step and the assembly of one loop from `start`."""
    loop.given.copy_(start)
    ticks = [tick_stats(loop.step()) for _ in range(3)]
    torch.cuda.synchronize()

    def step():
        if loop.t >= loop.ticks_possible:
            loop.t = 0
            loop.given.copy_(start)
        return loop.step()

    reps = 2 if batch <= 4096 else 1
    figures = {"rows": loop.asm.nc, "unknowns": loop.asm.no, "first_three_ticks": ticks,
               "step": spread(event_ms(step, reps, a.runs, warm=1))}
    loop.asm.bind_ltv_window("LIP", window[0], window[1], 0)
    figures["assemble"] = spread(event_ms(lambda: loop.asm.assemble(start), 5, a.runs))
    figures["kernel"] = loop.asm.last_kernel()
    return figures


def one_batch(api, forms, batch, a):
    out = {}
    n, m = 3, 1
    A_seq, B_seq = sequences(api, batch)
    Q, R = problems.lipm_feedback_weights()
    Qd, Rd = torch.as_tensor(Q, device="cuda"), torch.as_tensor(R, device="cuda")
    K_seq, _, info = engine.ltv_lqr(A_seq, B_seq, Qd, Rd, want_closed=False)
    assert int((info >= 0).sum()) == 0
    out["sizes"] = dict(batch=batch, N=N, T=T, n=n, m=m, axes=2)
    steps, nz = batch * T, n + m
    read = 8 * steps * (n * n + n * m + m * n)
    out["ltv_close"] = with_floor(event_ms(lambda: engine.ltv_close(A_seq, B_seq, K_seq), a.reps, a.runs),
                                  read + 8 * steps * n * n)
    out["ltv_augment"] = with_floor(event_ms(lambda: engine.ltv_augment(A_seq, B_seq, K_seq), a.reps, a.runs),
                                    read + 8 * steps * (nz * nz + nz * m + m * nz))
    rng = np.random.default_rng(17)
    x0 = rng.normal(0, 0.02, [batch, 6])
    z0 = np.zeros([batch, 8])
    z0[:, 0:3], z0[:, 4:7] = x0[:, 0:3], x0[:, 3:6]
    plain = LtvLoop(forms[0], "LIP", batch, A_seq, B_seq, feedback=K_seq)
    out["ltv_loop_feedback"] = loop_figures(plain, torch.as_tensor(x0, device="cuda"), (plain.A_cl_seq, B_seq), a,
                                            batch)
    del plain
    torch.cuda.empty_cache()
    true = LtvLoop(forms[1], "LIP", batch, A_seq, B_seq, feedback=K_seq, true_input=True)
    out["ltv_loop_true_input"] = loop_figures(true, torch.as_tensor(z0, device="cuda"), (true.At_seq, true.Bt_seq), a,
                                              batch)
    out["ltv_loop_true_input"]["input_limit"] = LIMIT
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[2048, 16384])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ltv_true_input_bench.json"))
    a = ap.parse_args()
    api = problems.load_api("mpc_interface")
    forms = (problems.lipm_ltv(api, N=N), problems.lipm_ltv_true_input(api, N=N, input_limit=LIMIT))
    result = {"what": "mpcasm_ltv_augment and LtvLoop(feedback=, true_input=True, input limit 0.1).step beside "
                      "mpcasm_ltv_close and LtvLoop(feedback=).step on C5 (N = 100, T = 118)",
              "reps": a.reps, "runs": a.runs, "hbm_bytes_per_s": HBM, "device": torch.cuda.get_device_name(0)}
    for batch in a.batches:
        result["c5_%d" % batch] = one_batch(api, forms, batch, a)
        torch.cuda.empty_cache()
        print("c5_%d measured" % batch, file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
