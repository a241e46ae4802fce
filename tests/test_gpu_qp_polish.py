"""GPU: mpcasm_qp_polish (csrc/polish.hip) against tests/polish_restatement.py -- its verdicts, the accuracy of the
points it accepts, what it leaves untouched -- on the shapes at which each loop of the kernel can go wrong, on the
biped's own QPs, and inside the closed loop of WalkerFleet, launch by launch and replayed from graphs.

The yardstick of an accepted point is the plain fp64 restatement on the device's own input iterate: the kernel
may err 8 times as much as that (the project's margin for another order of summation,
tests/test_gpu_solver_precision.py), or stay within the rounding magnitude of solver_reference.res_bounds where
that is larger.  A verdict is compared only where the restatement decides at least 1e-6 from a tie.

The accuracy tests print ``qp-polish-precision: ...`` lines (pytest -s) and keep the worst ratio per shape in
profiles/qp_polish_precision.txt."""
import functools
import os

import numpy as np
import pytest

import polish_restatement as pr
import solver_reference as sr
from helpers import LD
from mpcasm import capi, problems

pytestmark = pytest.mark.gpu
MARGIN = 1e-6
YARD = 8.0
PAD = 2                                     # rows of NaN behind the batch
PLAIN, WRONG, NAN, INFEASIBLE, UNSTATED = (0, 1, 2), 3, 4, 5, 6
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       "qp_polish_precision.txt")
HEAD = ("# mpcasm_qp_polish, accepted points: worst (device residual) / max(8 x the fp64 restatement's, the res_bounds\n"
        "# magnitude) per shape, primal and dual; written by tests/test_gpu_qp_polish.py\n")


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def record(key, text):
    """One line per shape in profiles/qp_polish_precision.txt (a checkout that cannot be written is left alone)."""
    print("qp-polish-precision: %-18s %s" % (key, text))
    try:
        lines = {}
        if os.path.exists(PROFILE):
            for line in open(PROFILE):
                if not line.startswith("#") and line.strip():
                    lines[line[:18].strip()] = line.rstrip("\n")
        lines[key] = "%-18s %s" % (key, text)
        with open(PROFILE, "w") as f:
            f.write(HEAD + "".join(lines[k] + "\n" for k in sorted(lines)))
    except OSError:
        pass


@functools.lru_cache(maxsize=None)
def problem(no, nc, na):
    """Seven complementary QPs of one shape (numpy, never changed): stacked ``P, q, G, h`` and the constructed
    active sets."""
    rng = np.random.default_rng([no, nc, na, 70])
    qps = [pr.complementary_qp(rng, no, nc, na) for _ in range(7)]
    return tuple(np.stack([qp[i] for qp in qps]) for i in (0, 1, 2, 3, 6))


def padded(torch, host, fill=float("nan")):
    """``host`` (B, ...) on the device with PAD rows of ``fill`` behind it: ``(whole, view of the first B)``."""
    B = host.shape[0]
    whole = torch.full((B + PAD,) + tuple(host.shape[1:]), fill, dtype=torch.float64, device="cuda")
    whole[:B].copy_(torch.as_tensor(host))
    return whole, whole[:B]


def judge(qp, start, status, dev, what):
    """One polish call against the restatement.  ``qp``: stacked numpy P, q, G, h; ``start``: the iterates and res
    that went in (numpy); ``status``: numpy or None; ``dev``: what came back (numpy x, y, z, polish, res).  Returns
    the restatement's results and the worst accuracy ratios (primal, dual) over the accepted instances."""
    P, q, G, h = qp
    x0, y0, z0, res0 = start
    x1, y1, z1, verdict, res1 = dev
    B, no, nc = P.shape[0], P.shape[1], G.shape[1]
    outs, worst = [], [0.0, 0.0]
    for b in range(B):
        out = pr.polish(P[b], q[b], G[b], h[b], x0[b], y0[b], z0[b], status=None if status is None else status[b])
        outs.append(out)
        # (a) no synthetic instance is near a tie; the verdict is the restatement's
        assert out.margin >= MARGIN, (what, b, out.margins)
        assert verdict[b] == out.polish, (what, b, int(verdict[b]), out.polish, out.margins)
        same = lambda a, c: np.array_equal(a.view(np.int64), c.view(np.int64))
        if out.polish != pr.DONE:
            # (c) skipped and rejected instances keep their bits
            assert same(x1[b], x0[b]) and same(y1[b], y0[b]) and same(z1[b], z0[b]) and same(res1[b], res0[b]), (what, b)
            continue
        # (b) an accepted point: its residuals in long double against the restatement's on the same input
        rp, rd, Mp, Md = sr.residuals(P[b], q[b], G[b], x1[b], y1[b], z1[b])
        bp, bd = sr.res_bounds(no, nc, Mp, Md)
        fp, fd = sr.residuals(P[b], q[b], G[b], out.x, out.y, out.z)[:2]
        ratios = float(rp) / max(YARD * float(fp), bp), float(rd) / max(YARD * float(fd), bd)
        assert ratios[0] <= 1.0 and ratios[1] <= 1.0, (what, b, float(rp), float(fp), bp, float(rd), float(fd), bd)
        worst = [max(w, r) for w, r in zip(worst, ratios)]
        assert np.isfinite(x1[b]).all() and (y1[b] >= 0).all()
        assert not y1[b][~out.active].any(), (what, b)                       # exactly 0 off the active set
        gx = G[b].astype(LD) @ x1[b].astype(LD)                              # z^ = min(G x^, h) to rounding
        assert float(np.abs(z1[b].astype(LD) - np.minimum(gx, h[b].astype(LD))).max(initial=0)) <= bp, (what, b)
        assert (z1[b] <= h[b]).all()
        assert abs(res1[b, 0] - float(rp)) <= bp and abs(res1[b, 1] - float(rd)) <= bd, (what, b, res1[b], rp, rd)
    return outs, worst


@pytest.mark.parametrize("no,nc,na", pr.SHAPES, ids=["%dx%d-na%d" % s for s in pr.SHAPES])
def test_verdicts_accuracy_and_untouched_outputs(gpu_api, torch_gpu, no, nc, na):
    """(a), (b), (c) on seven instances of the shape: three plain, one with a wrong active set, one NON_CVX by its
    status with NaN iterates, one PRIMAL_INFEASIBLE by its status, one MAX_ITER by its status; then all seven again
    without a status (the NaN one is read then, and rejected)."""
    torch = torch_gpu
    from mpcasm import engine

    qp, constructed = problem(no, nc, na)[:4], problem(no, nc, na)[4]
    B = qp[0].shape[0]
    dP, dq, dG, dh = (torch.as_tensor(a, device="cuda") for a in qp)
    sol = engine.solve_qp(dP, dq, dG, dh)
    assert sol.status.tolist() == [capi.QP_SOLVED] * B
    assert sol.polish is None
    x0, y0, z0, res0 = (t.cpu().numpy().copy() for t in (sol.x, sol.y, sol.z, sol.res))
    status = sol.status.cpu().numpy().copy()
    guess = (qp[3][WRONG] - z0[WRONG]) < y0[WRONG]
    if na < nc:
        y0[WRONG], row = pr.wrong_active_set(qp[3][WRONG], y0[WRONG], z0[WRONG], guess)
    x0[NAN], y0[NAN], z0[NAN], res0[NAN] = np.nan, np.nan, np.nan, np.nan
    status[NAN], status[INFEASIBLE], status[UNSTATED] = capi.QP_NON_CVX, capi.QP_PRIMAL_INFEASIBLE, capi.QP_MAX_ITER
    worst = [0.0, 0.0]
    seen = []
    for what, st in (("with status", status), ("status NULL", None)):
        wx, x = padded(torch, x0)
        wy, y = padded(torch, y0)
        wz, z = padded(torch, z0)
        wr, res = padded(torch, res0)
        verdict = torch.full((B + PAD,), -99, dtype=torch.int32, device="cuda")
        dst = None if st is None else torch.as_tensor(st, device="cuda")
        got = engine.polish_qp(dP, dq, dG, dh, (x, y, z), status=dst, out=(verdict[:B], res))
        assert got[0] is x and got[3].data_ptr() == verdict.data_ptr()
        torch.cuda.synchronize()
        for whole in (wx, wy, wz, wr):                                  # (c) nothing behind the batch
            assert torch.isnan(whole[B:]).all()
        assert verdict[B:].tolist() == [-99] * PAD
        dev = tuple(t.cpu().numpy() for t in (x, y, z, verdict[:B], res))
        outs, w = judge(qp, (x0, y0, z0, res0), st, dev, "%dx%d na %d, %s" % (no, nc, na, what))
        worst = [max(a, b) for a, b in zip(worst, w)]
        seen.append([o.polish for o in outs])
        # the premises: the plain instances are polished, to exactly the constructed active set
        for b in PLAIN:
            assert outs[b].polish == pr.DONE and np.array_equal(outs[b].active, constructed[b])
            assert outs[b].margins["active"] >= 0.5
    first, second = seen
    assert first[NAN] == first[INFEASIBLE] == first[UNSTATED] == pr.SKIPPED
    assert second[NAN] == pr.REJECTED and second[INFEASIBLE] == second[UNSTATED] == pr.DONE
    if na < nc:
        assert first[WRONG] == second[WRONG] == (pr.REJECTED if na < no else pr.SKIPPED)
    record("%dx%d-na%d" % (no, nc, na), "primal %.3f  dual %.3f" % tuple(worst))


def test_skipped_when_the_active_set_outgrows_the_unknowns(gpu_api, torch_gpu):
    """(5, 12) with every y positive: na = 12 > no = 5, SKIPPED, nothing written, with and without d_res."""
    torch = torch_gpu
    from mpcasm import engine

    rng = np.random.default_rng(12)
    qps = [pr.complementary_qp(rng, 5, 12, 3) for _ in range(3)]
    P, q, G, h = (torch.as_tensor(np.stack([qp[i] for qp in qps]), device="cuda") for i in range(4))
    sol = engine.solve_qp(P, q, G, h)
    y = (h - sol.z) + 1.0
    before = [t.clone() for t in (sol.x, y, sol.z)]
    x, y, z, verdict, res = engine.polish_qp(P, q, G, h, (sol.x, y, sol.z), status=sol.status)
    assert verdict.tolist() == [capi.POLISH_SKIPPED] * 3
    assert all(torch.equal(a, b) for a, b in zip(before, (x, y, z)))
    assert torch.isnan(res).all()
    verdict.fill_(-99)
    rc = capi.load().mpcasm_qp_polish(5, 12, P.data_ptr(), q.data_ptr(), G.data_ptr(), h.data_ptr(), x.data_ptr(),
                                      y.data_ptr(), z.data_ptr(), None, 1e-6, 3, verdict.data_ptr(), None, 3, None)
    assert rc == capi.OK and verdict.tolist() == [capi.POLISH_SKIPPED] * 3


# ---- the biped's own QPs ---------------------------------------------------------------------------------------
def test_the_bipeds_qps_polished_after_the_solve(gpu_api, torch_gpu):
    """(d) 64 biped QPs a few ticks into the closed loop of a fleet whose walkers start slightly apart:
    solve_qp(..., polish=True) against the restatement on solve_qp's own iterates (a cold solve is deterministic)."""
    torch = torch_gpu
    from mpcasm import engine
    from mpcasm.walkers import WalkerFleet

    conf = problems.BipedConfig(step_samples=8)
    B = 64
    fleet = WalkerFleet(B, conf=conf, api=gpu_api)
    given = fleet.start_at_rest()
    rng = np.random.default_rng(3)
    given += torch.as_tensor(rng.normal(0.0, 2e-3, tuple(given.shape)), device=given.device)
    for _ in range(5):
        fleet.step()
    total = checked = done = 0
    worst = [0.0, 0.0]
    for entry in fleet.tick(given):
        P, q, G, h = (entry[k].clone() for k in ("P", "q", "G", "h"))
        plain = engine.solve_qp(P, q, G, h)
        sol = engine.solve_qp(P, q, G, h, polish=True)
        assert sol.polish is not None and torch.equal(plain.status, sol.status) and torch.equal(plain.iters, sol.iters)
        qp = tuple(t.cpu().numpy() for t in (P, q, G, h))
        x0, y0, z0, res0, status = (t.cpu().numpy() for t in (plain.x, plain.y, plain.z, plain.res, plain.status))
        x1, y1, z1, res1, verdict = (t.cpu().numpy() for t in (sol.x, sol.y, sol.z, sol.res, sol.polish))
        no, nc = qp[0].shape[1], qp[2].shape[1]
        for b in range(qp[0].shape[0]):
            total += 1
            out = pr.polish(qp[0][b], qp[1][b], qp[2][b], qp[3][b], x0[b], y0[b], z0[b], status=status[b])
            if out.margin < MARGIN:
                continue
            checked += 1
            assert verdict[b] == out.polish, (b, int(verdict[b]), out.polish, out.margins)
            if out.polish != pr.DONE:
                assert np.array_equal(x1[b], x0[b]) and np.array_equal(y1[b], y0[b]) and np.array_equal(z1[b], z0[b])
                assert np.array_equal(res1[b], res0[b])
                continue
            done += 1
            rp, rd, Mp, Md = sr.residuals(qp[0][b], qp[1][b], qp[2][b], x1[b], y1[b], z1[b])
            bp, bd = sr.res_bounds(no, nc, Mp, Md)
            fp, fd = sr.residuals(qp[0][b], qp[1][b], qp[2][b], out.x, out.y, out.z)[:2]
            ratios = float(rp) / max(YARD * float(fp), bp), float(rd) / max(YARD * float(fd), bd)
            assert ratios[0] <= 1.0 and ratios[1] <= 1.0, (b, float(rp), float(fp), bp, float(rd), float(fd), bd)
            worst = [max(w, r) for w, r in zip(worst, ratios)]
            assert (y1[b] >= 0).all() and not y1[b][~out.active].any()
            assert abs(res1[b, 0] - float(rp)) <= bp and abs(res1[b, 1] - float(rd)) <= bd
    assert total == B and checked >= 0.9 * total, (checked, total)
    assert done > 0, (done, checked)
    record("biped-64", "primal %.3f  dual %.3f  (%d of %d judged, %d DONE)" % (worst[0], worst[1], checked, total, done))


# ---- inside the closed loop --------------------------------------------------------------------------------------
def walk(torch, fleet, ticks):
    """``ticks`` closed ticks: status, polish (when the fleet polishes) and the trail of ``given``, in walker order."""
    given = fleet.given_buffer()
    i32 = dict(dtype=torch.int32, device=given.device)
    status, polish = torch.zeros((ticks, fleet.batch), **i32), torch.full((ticks, fleet.batch), -99, **i32)
    trail = torch.empty((ticks + 1,) + tuple(given.shape), dtype=given.dtype, device=given.device)
    trail[0].copy_(given)
    for t in range(ticks):
        for entry in fleet.step():
            index = entry["index"].long()
            status[t].index_copy_(0, index, entry["status"])
            if "polish" in entry:
                polish[t].index_copy_(0, index, entry["polish"])
        trail[t + 1].copy_(given)
    return status, polish, trail


def test_polished_ticks_replayed_from_graphs(gpu_api, torch_gpu):
    """(e) two rounds of the step cycle at 64 walkers: the graphs give the status, polish and given of launch by
    launch; the polish changes the walk; and polish=False is the fleet of before."""
    torch = torch_gpu
    from mpcasm.walkers import WalkerFleet

    conf = problems.BipedConfig(step_samples=8)
    B, ticks = 64, 2 * 2 * conf.step_samples
    eager = WalkerFleet(B, conf=conf, api=gpu_api, polish=True)
    graphs = WalkerFleet(B, conf=conf, api=gpu_api, polish=True, graphs=True)
    eager.start_at_rest()
    graphs.start_at_rest()
    a = walk(torch, eager, ticks)
    b = walk(torch, graphs, ticks)
    assert len(graphs._step_graphs) == 2 * conf.step_samples
    for name, u, v in zip(("status", "polish", "given"), a, b):
        assert torch.equal(u, v), name
    verdicts = a[1]
    assert set(verdicts.unique().tolist()) <= {capi.POLISH_DONE, capi.POLISH_SKIPPED, capi.POLISH_REJECTED}
    assert int((verdicts == capi.POLISH_DONE).sum()) > 0
    # an instance that is not solved is never polished
    assert bool(((a[0] == capi.QP_SOLVED) | (verdicts == capi.POLISH_SKIPPED)).all())
    off = WalkerFleet(B, conf=conf, api=gpu_api, polish=False)
    plain = WalkerFleet(B, conf=conf, api=gpu_api)
    off.start_at_rest()
    plain.start_at_rest()
    c = walk(torch, off, 2 * conf.step_samples)
    d = walk(torch, plain, 2 * conf.step_samples)
    for name, u, v in zip(("status", "polish", "given"), c, d):
        assert torch.equal(u, v), name
    assert (c[1] == -99).all()                      # (no "polish" in the results of a fleet that does not polish)
    assert not torch.equal(a[2][:c[2].shape[0]], c[2])
