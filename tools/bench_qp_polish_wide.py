#!/usr/bin/env python3
"""mpcasm_qp_polish_wide on the shapes mpcasm_qp_solve_wide was built for, with tools/bench_qp_polish.py's method:
hipEvents around back-to-back calls on a warm device (every shape run first, untimed), each figure the median (and
min, max) of `--runs` windows of `--reps` calls.  Writes profiles/qp_polish_wide_bench.json and prints it as one
JSON line.  Nothing here is a gate: a new capability has no earlier figure to hold it to.

* C3 (problems.lipm3d, 96 x 196) at 4 096 instances from `assemble`; C5-shaped QPs (200 x 404, random, solvable)
  at 2 048 and C4's shape (384 x 1 536) at `--c4-batch`, tools/bench_qp_solve_wide.py's batches
* per case: solve_qp_wide to 1e-3 (cold, OSQP's defaults); the polish alone on that solve's iterates -- every call
  starts from the same iterates, restored by device copies that are timed on their own and subtracted; the shares
  DONE / REJECTED / SKIPPED; the median and the largest |x - x_tight|_inf before and after, x_tight the same QP
  solved by solve_qp_wide to 1e-9; the LDS of a workgroup, the workspace and the workgroups of the launch; the
  polish alone with 128, 256, 384 and 512 workgroups (MPCASM_QP_POLISH_WIDE_GROUPS)

bench_qp_polish_wide.py [--reps 5] [--runs 5] [--c4-batch 256] [--cases c3,c5,c4] [--out ...]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-interface_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mpcasm import capi, engine, problems  # noqa: E402


GROUPS = (128, 256, 384, 512)


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


def quality(x, tight, solved, verdict=None):
    err = (x - tight).abs().amax(dim=1)
    ok = torch.isfinite(err) & solved
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


def random_batch(rng, B, no, nc):
    import osqp_restatement as rs

    qps = [rs.random_qp(rng, no, nc) for _ in range(min(B, 16))]
    P, q, G, h = (np.stack(a) for a in zip(*qps))
    reps = (B + len(qps) - 1) // len(qps)
    return [torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * reps)[:B]), device="cuda") for a in (P, q, G, h)]


def case(P, q, G, h, reps, runs, tight_iter):
    B, no, nc = P.shape[0], P.shape[1], G.shape[1]
    lds, work_bytes, groups = engine.qp_polish_wide_info(no, nc, B)
    out = {"batch": B, "no": no, "nc": nc, "lds_bytes_per_workgroup": lds, "work_bytes": work_bytes,
           "workgroups": groups, "kinv_on_chip_in_the_solve": engine.qp_solve_wide_info(no, nc)[1]}
    kinv = torch.empty((B, no, no), dtype=torch.float64, device="cuda")
    work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
    solve = lambda: engine.solve_qp_wide(P, q, G, h, kinv=kinv)
    sol = solve()
    solved = sol.status == engine.QP_SOLVED
    tight = engine.solve_qp_wide(P, q, G, h, eps_abs=1e-9, eps_rel=1e-9, max_iter=tight_iter, kinv=kinv)
    both = solved & (tight.status == engine.QP_SOLVED)
    out["tight_1e-9"] = {"solved": int((tight.status == engine.QP_SOLVED).sum()), "max_iter": tight_iter,
                         "iters_mean": round(float(tight.iters.double().mean()), 1)}
    keep = [t.clone() for t in (sol.x, sol.y, sol.z)]
    iterate = [t.clone() for t in keep]
    verdict = torch.empty(B, dtype=torch.int32, device="cuda")
    res = torch.empty((B, 2), dtype=torch.float64, device="cuda")

    def restore():
        for w, k in zip(iterate, keep):
            w.copy_(k)

    def polish(refine=engine.OSQP_POLISH_REFINE):
        restore()
        engine.polish_qp_wide(P, q, G, h, iterate, status=sol.status, refine_iters=refine, out=(verdict, res),
                              work=work)

    polish()                                                    # (the shape warmed, the verdicts of one call kept)
    torch.cuda.synchronize()
    active = ((h - sol.z) < sol.y).sum(dim=1).double()
    out["solve_1e-3"] = dict(spread(event_ms(solve, reps, runs)), **quality(sol.x, tight.x, both),
                             solved=int(solved.sum()), iters_mean=round(float(sol.iters.double().mean()), 1),
                             active_rows_mean=round(float(active[solved].mean()), 1) if int(solved.sum()) else None)
    out["polished"] = quality(iterate[0], tight.x, both, verdict)
    copy_ms = statistics.median(event_ms(restore, reps, runs))
    out["polish_alone"] = dict(spread([p - copy_ms for p in event_ms(polish, reps, runs)]),
                               restore_copies_ms=round(copy_ms, 4))
    out["polish_alone_refine_0"] = spread([p - copy_ms for p in event_ms(lambda: polish(0), reps, runs)])
    out["polish_over_solve"] = round(out["polish_alone"]["ms"] / out["solve_1e-3"]["ms"], 4)
    # fewer workgroups than the cap (MPCASM_QP_POLISH_WIDE_GROUPS): one, one and a half and two per CU of 256
    out["polish_alone_by_workgroups"] = {}
    for groups in GROUPS:
        if groups > min(B, capi.POLISH_WIDE_CAP):
            continue
        os.environ["MPCASM_QP_POLISH_WIDE_GROUPS"] = str(groups)
        try:
            assert engine.qp_polish_wide_info(no, nc, B)[2] == groups
            out["polish_alone_by_workgroups"][str(groups)] = spread([p - copy_ms for p in event_ms(polish, reps, runs)])
        finally:
            del os.environ["MPCASM_QP_POLISH_WIDE_GROUPS"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--c4-batch", type=int, default=256)
    ap.add_argument("--tight-iter", type=int, default=20000)
    ap.add_argument("--cases", default="c3,c5,c4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qp_polish_wide_bench.json"))
    a = ap.parse_args()
    cases = a.cases.split(",")
    api = problems.load_api("mpc_interface")
    result = {"what": "mpcasm_qp_polish_wide", "device": torch.cuda.get_device_name(), "reps": a.reps,
              "runs": a.runs, "workgroup_cap": capi.POLISH_WIDE_CAP}
    rng = np.random.default_rng(31)
    if "c3" in cases:
        B = 4096
        form = problems.lipm3d(api, N=32)
        given = rng.normal(0, 0.02, [B, form.given_len])
        given[:, 6] += 0.85
        P, q, G, h = (t.clone() for t in engine.Assembler(form, batch=B).assemble(given))
        result["c3_4096"] = case(P, q, G, h, a.reps, a.runs, a.tight_iter)
    if "c5" in cases:
        result["c5_shape_2048"] = case(*random_batch(rng, 2048, 200, 404), a.reps, a.runs, a.tight_iter)
    if "c4" in cases:
        result["c4_shape_%d" % a.c4_batch] = case(*random_batch(rng, a.c4_batch, 384, 1536), 1, a.runs, a.tight_iter)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
