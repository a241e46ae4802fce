#!/usr/bin/env python3
"""mpcasm_qp_solve on 4 096 biped QPs straight out of mpcasm_assemble (the walking loop's tick,
biped_mpc_loop.py:50-60): hipEvents around back-to-back calls on a warm device, each figure from `--runs`
windows of `--reps` calls (median, min, max across the windows).  Prints one JSON line.

* cold: x = 0, rho = 0.1, to eps 1e-3 (OSQP's default) and to eps 1e-5; mean and max iterations
* warm: the next tick (a new `given`, P and G unchanged) from the last iterate with K^-1 and rho kept; every
  call starts from the same state, restored by device copies that are timed on their own and subtracted
* the mode's own cost: solve_qp with check_every = max_iter, all four eps 0 and rho fixed (one check, at the
  end) against mpcasm_admm with its residuals, both `--iters` iterations

bench_qp_solve.py [--batch 4096] [--reps 20] [--runs 5] [--iters 200]"""
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

from mpcasm import engine, problems  # noqa: E402


def event_ms(fn, reps, runs):
    """Per-call ms of ``fn`` over ``runs`` windows of ``reps`` back-to-back calls, after warm-up calls."""
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


def iters_of(sol):
    it = sol.iters.double()
    return {"iters_mean": round(float(it.mean()), 1), "iters_max": int(it.max()),
            "solved": int((sol.status == engine.QP_SOLVED).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    B = a.batch
    api = problems.load_api("mpc_interface")
    form = problems.biped(api, problems.BipedConfig(step_samples=8))
    form.update(step_times=np.array([6, 14]), step_count=0)
    rng = np.random.default_rng(8)
    given = rng.normal(0, 0.001, [B, form.given_len])
    asm = engine.Assembler(form, batch=B)
    P, q, G, h = (t.clone() for t in asm.assemble(given))
    result = {"what": "mpcasm_qp_solve", "batch": B, "no": P.shape[1], "nc": G.shape[1],
              "lds_bytes_per_instance": engine.qp_solve_lds_bytes(P.shape[1], G.shape[1]),
              "reps": a.reps, "runs": a.runs}

    for name, eps in (("cold_1e-3", 1e-3), ("cold_1e-5", 1e-5)):
        sol = engine.solve_qp(P, q, G, h, eps_abs=eps, eps_rel=eps)
        result[name] = dict(spread(event_ms(lambda: engine.solve_qp(P, q, G, h, eps_abs=eps, eps_rel=eps),
                                            a.reps, a.runs)), **iters_of(sol))

    # the next tick: what the first left behind, a new `given`
    kinv = torch.empty(tuple(P.shape), dtype=torch.float64, device="cuda")
    rho = torch.full((B,), engine.OSQP_RHO, dtype=torch.float64, device="cuda")
    first = engine.solve_qp(P, q, G, h, rho=rho, kinv=kinv)
    keep = [t.clone() for t in (first.x, first.y, first.z, rho, kinv)]
    P2, q2, G2, h2 = asm.assemble(given + rng.normal(0, 0.0005, given.shape))
    assert torch.equal(P2, P)
    work = [t.clone() for t in keep]

    def restore():
        for w, k in zip(work, keep):
            w.copy_(k)

    def warm():
        restore()
        return engine.solve_qp(P2, q2, G2, h2, *work[:3], rho=work[3], kinv=work[4], kinv_valid=True)

    sol = warm()
    copy_ms = event_ms(restore, a.reps, a.runs)
    warm_ms = event_ms(warm, a.reps, a.runs)
    result["warm_next_tick"] = dict(spread([w - statistics.median(copy_ms) for w in warm_ms]), **iters_of(sol),
                                    restore_copies_ms=round(statistics.median(copy_ms), 4))

    # the mode itself: the same iterations, one check at the end, against the plain iteration
    n = a.iters
    fixed = dict(eps_abs=0.0, eps_rel=0.0, eps_prim_inf=0.0, eps_dual_inf=0.0, max_iter=n, check_every=n,
                 adaptive_rho_interval=0)
    s_ms = event_ms(lambda: engine.solve_qp(P, q, G, h, **fixed), a.reps, a.runs)
    a_ms = event_ms(lambda: engine.admm(P, q, G, h, iters=n), a.reps, a.runs)
    # and the cost of checking every 25 iterations, nothing stopping early
    c_ms = event_ms(lambda: engine.solve_qp(P, q, G, h, **dict(fixed, check_every=25)), a.reps, a.runs)
    result["fixed_%d_iters" % n] = {"solve_qp_one_check": spread(s_ms), "admm": spread(a_ms),
                                    "solve_qp_check_every_25": spread(c_ms)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
