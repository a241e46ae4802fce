"""GPU: mpcasm_qp_polish_wide (csrc/polish_wide.hip) held to tests/polish_restatement.py as
tests/test_gpu_qp_polish.py holds mpcasm_qp_polish, by that test's own ``judge``: the verdict is the restatement's
wherever that is at least 1e-6 from a tie; an accepted point's residuals, recomputed in long double, stay within
max(8 x the fp64 restatement's, solver_reference.res_bounds); y^ is exactly 0 off the active set, z^ = min(G x^, h);
skipped and rejected instances and the rows behind the batch keep their bits.  On the shapes at which each loop of
the kernel can go wrong (tests/polish_wide_cases.py), on more instances than the launch has workgroups, beside
mpcasm_qp_polish where both apply, on assembled C3 QPs, inside LtvLoop and replayed from a graph.

The iterates are engine.solve_qp_wide's.  The accuracy tests print ``qp-polish-wide-precision: ...`` lines
(pytest -s) and keep the worst ratio per shape in profiles/qp_polish_wide_precision.txt."""
import os

import numpy as np
import pytest

import polish_restatement as pr
import polish_wide_cases as cases
import rollout_cases as rc
import solver_reference as sr
from mpcasm import capi
from polish_wide_cases import INFEASIBLE, NAN, PLAIN, UNSTATED, WRONG
from helpers import LD
from test_gpu_qp_polish import MARGIN, PAD, YARD, padded
from test_gpu_qp_solve_wide import c3_batch

pytestmark = pytest.mark.gpu
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       "qp_polish_wide_precision.txt")
HEAD = ("# mpcasm_qp_polish_wide, accepted points: worst (device residual) / max(8 x the fp64 restatement's, the\n"
        "# res_bounds magnitude) per shape, primal and dual; written by tests/test_gpu_qp_polish_wide.py\n")


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def record(key, text):
    """One line per shape in profiles/qp_polish_wide_precision.txt (a checkout that cannot be written is left
    alone)."""
    print("qp-polish-wide-precision: %-18s %s" % (key, text))
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


def same(a, c):
    return np.array_equal(a.view(np.int64), c.view(np.int64))


def accepted(P, q, G, h, out, x1, y1, z1, res1, what):
    """An accepted point against the yardstick: its residuals in long double within max(8 x the fp64 restatement's
    on the same input, res_bounds), y^ exactly 0 off the active set, z^ = min(G x^, h), d_res the residuals.  Returns
    the two ratios (a residual of exactly 0 -- every one without limits -- is 0 of any bound, a bound of 0 too)."""
    no, nc = P.shape[0], G.shape[0]
    rp, rd, Mp, Md = sr.residuals(P, q, G, x1, y1, z1)
    bp, bd = sr.res_bounds(no, nc, Mp, Md)
    fp, fd = sr.residuals(P, q, G, out.x, out.y, out.z)[:2]
    ratios = []
    for r, f, bound in ((rp, fp, bp), (rd, fd, bd)):
        limit = max(YARD * float(f), bound)
        assert float(r) <= limit, (what, float(rp), float(fp), bp, float(rd), float(fd), bd)
        ratios.append(float(r) / limit if float(r) > 0.0 else 0.0)
    assert np.isfinite(x1).all() and (y1 >= 0).all(), what
    assert not y1[~out.active].any(), what                                   # exactly 0 off the active set
    gx = G.astype(LD) @ x1.astype(LD)                                        # z^ = min(G x^, h) to rounding
    assert float(np.abs(z1.astype(LD) - np.minimum(gx, h.astype(LD))).max(initial=0)) <= bp, what
    assert (z1 <= h).all(), what
    assert abs(res1[0] - float(rp)) <= bp and abs(res1[1] - float(rd)) <= bd, (what, res1, rp, rd)
    return ratios


def judge(qp, start, status, dev, what):
    """tests/test_gpu_qp_polish.py's judge, restated (that one divides by a bound that is 0 without limits).  ``qp``:
    stacked numpy P, q, G, h; ``start``: the iterates and res that went in; ``status``: numpy or None; ``dev``: what
    came back (x, y, z, polish, res).  Returns the restatement's results and the worst ratios (primal, dual)."""
    P, q, G, h = qp
    x0, y0, z0, res0 = start
    x1, y1, z1, verdict, res1 = dev
    outs, worst = [], [0.0, 0.0]
    for b in range(P.shape[0]):
        out = pr.polish(P[b], q[b], G[b], h[b], x0[b], y0[b], z0[b], status=None if status is None else status[b])
        outs.append(out)
        # no synthetic instance is near a tie; the verdict is the restatement's
        assert out.margin >= MARGIN, (what, b, out.margins)
        assert verdict[b] == out.polish, (what, b, int(verdict[b]), out.polish, out.margins)
        if out.polish != pr.DONE:                  # skipped and rejected instances keep their bits
            assert same(x1[b], x0[b]) and same(y1[b], y0[b]) and same(z1[b], z0[b]) and same(res1[b], res0[b]), (what, b)
            continue
        ratios = accepted(P[b], q[b], G[b], h[b], out, x1[b], y1[b], z1[b], res1[b], (what, b))
        worst = [max(w, r) for w, r in zip(worst, ratios)]
    return outs, worst


def solved_start(torch, qp):
    """engine.solve_qp_wide's iterates of the stacked QPs, all SOLVED: device P, q, G, h and numpy copies of
    x, y, z, res, status."""
    from mpcasm import engine

    dev = tuple(torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in qp)
    sol = engine.solve_qp_wide(*dev)
    assert sol.status.tolist() == [capi.QP_SOLVED] * qp[0].shape[0]
    assert sol.polish is None
    return dev, [t.cpu().numpy().copy() for t in (sol.x, sol.y, sol.z, sol.res, sol.status)]


def seven(torch, no, nc, na):
    """The seven instances of a shape as the narrow test poses them: three plain, one with a wrong active set (where
    the shape has an inactive row), one NON_CVX by its status with NaN iterates, one PRIMAL_INFEASIBLE and one
    MAX_ITER by their status."""
    full = cases.problem(no, nc, na)
    qp = full[:4]
    dev, (x0, y0, z0, res0, status) = solved_start(torch, qp)
    if na < nc:
        guess = (qp[3][WRONG] - z0[WRONG]) < y0[WRONG]
        y0[WRONG] = pr.wrong_active_set(qp[3][WRONG], y0[WRONG], z0[WRONG], guess)[0]
    x0[NAN], y0[NAN], z0[NAN], res0[NAN] = np.nan, np.nan, np.nan, np.nan
    status[NAN], status[INFEASIBLE], status[UNSTATED] = capi.QP_NON_CVX, capi.QP_PRIMAL_INFEASIBLE, capi.QP_MAX_ITER
    return qp, full[4], dev, (x0, y0, z0, res0), status


def polish_padded(torch, dev, start, st, entry=None):
    """One polish call on copies of ``start`` with PAD rows of NaN behind the batch; what came back, as numpy."""
    from mpcasm import engine

    entry = entry or engine.polish_qp_wide
    B = start[0].shape[0]
    wholes, views = zip(*(padded(torch, a) for a in start))
    x, y, z, res = views
    verdict = torch.full((B + PAD,), -99, dtype=torch.int32, device="cuda")
    dst = None if st is None else torch.as_tensor(st, device="cuda")
    got = entry(*dev, (x, y, z), status=dst, out=(verdict[:B], res))
    assert got[0] is x and got[3].data_ptr() == verdict.data_ptr()
    torch.cuda.synchronize()
    for whole in wholes:                                                # nothing behind the batch
        assert torch.isnan(whole[B:]).all()
    assert verdict[B:].tolist() == [-99] * PAD
    return tuple(t.cpu().numpy() for t in (x, y, z, verdict[:B], res))


@pytest.mark.parametrize("no,nc,na", cases.SHAPES, ids=cases.IDS(cases.SHAPES))
def test_verdicts_accuracy_and_untouched_outputs(gpu_api, torch_gpu, no, nc, na):
    """The seven instances of the shape with their status, then all seven again without one (the NaN one is read
    then, and rejected)."""
    torch = torch_gpu
    qp, constructed, dev, start, status = seven(torch, no, nc, na)
    worst, seen = [0.0, 0.0], []
    for what, st in (("with status", status), ("status NULL", None)):
        got = polish_padded(torch, dev, start, st)
        outs, w = judge(qp, start, st, got, "wide %dx%d na %d, %s" % (no, nc, na, what))
        worst = [max(a, b) for a, b in zip(worst, w)]
        seen.append([o.polish for o in outs])
        for b in PLAIN:                  # the premises: polished, to exactly the constructed active set
            assert outs[b].polish == pr.DONE and np.array_equal(outs[b].active, constructed[b])
            assert outs[b].margins["active"] >= 0.5
    first, second = seen
    assert first[NAN] == first[INFEASIBLE] == first[UNSTATED] == pr.SKIPPED
    # (without a status the last two are read and decided like any other -- the restatement's verdict, held above;
    # instances 4 to 6 of a shape are not among those whose active-set guess test_qp_polish_wide_cpu.py confirms)
    assert second[NAN] == pr.REJECTED and pr.SKIPPED not in (second[INFEASIBLE], second[UNSTATED])
    if na < nc:
        assert first[WRONG] == second[WRONG] == pr.REJECTED
    record("%dx%d-na%d" % (no, nc, na), "primal %.3f  dual %.3f" % tuple(worst))


def test_the_largest_shape(gpu_api, torch_gpu):
    """(512, 520, 100), once: two plain instances and one with a wrong active set."""
    torch = torch_gpu
    full = cases.largest()
    qp = full[:4]
    dev, (x0, y0, z0, res0, status) = solved_start(torch, qp)
    guess = (qp[3][2] - z0[2]) < y0[2]
    y0[2] = pr.wrong_active_set(qp[3][2], y0[2], z0[2], guess)[0]
    start = (x0, y0, z0, res0)
    got = polish_padded(torch, dev, start, status)
    outs, worst = judge(qp, start, status, got, "wide %dx%d na %d" % cases.LARGEST)
    assert [o.polish for o in outs] == [pr.DONE, pr.DONE, pr.REJECTED]
    for b in (0, 1):
        assert np.array_equal(outs[b].active, full[4][b])
    record("%dx%d-na%d" % cases.LARGEST, "primal %.3f  dual %.3f" % tuple(worst))


def test_more_instances_than_workgroups(gpu_api, torch_gpu):
    """2 CAP + 3 instances, the seven of (36, 76, 20) over and over: every workgroup takes a second instance, three
    of them a third, of another kind than the one before it -- and every copy comes back as the first copy did, so
    no instance sees what the one before it left in LDS or in the workspace."""
    torch = torch_gpu
    from mpcasm import engine

    qp, constructed, dev, start, status = seven(torch, 36, 76, 20)
    batch = 2 * capi.POLISH_WIDE_CAP + 3
    assert engine.qp_polish_wide_info(36, 76, batch)[2] == capi.POLISH_WIDE_CAP < batch
    pick = torch.arange(batch, device="cuda") % 7
    P, q, G, h = (t[pick].contiguous() for t in dev)
    x, y, z, res = (torch.as_tensor(a, device="cuda")[pick].contiguous() for a in start)
    st = torch.as_tensor(status, device="cuda")[pick].contiguous()
    work = torch.full((engine.qp_polish_wide_info(36, 76, batch)[1],), 0xFF, dtype=torch.uint8, device="cuda")
    verdict = torch.full((batch,), -99, dtype=torch.int32, device="cuda")
    engine.polish_qp_wide(P, q, G, h, (x, y, z), status=st, out=(verdict, res), work=work)
    torch.cuda.synchronize()
    assert torch.equal(verdict, verdict[:7][pick])
    for t in (x, y, z, res):
        assert torch.equal(bits64(t), bits64(t[:7][pick].contiguous()))
    first = verdict[:7].tolist()
    assert [first[b] for b in PLAIN] == [pr.DONE] * 3 and first[WRONG] == pr.REJECTED
    assert first[NAN] == first[INFEASIBLE] == first[UNSTATED] == pr.SKIPPED
    # ... and the first copy is what a launch of its own gives
    alone = polish_padded(torch, dev, start, status)
    for t, a in zip((x, y, z, verdict, res), alone):
        assert np.array_equal(t[:7].cpu().numpy(), a, equal_nan=True)


@pytest.mark.parametrize("no,nc,na", cases.BOTH, ids=cases.IDS(cases.BOTH))
def test_both_kernels_where_both_apply(gpu_api, torch_gpu, no, nc, na):
    """mpcasm_qp_polish and mpcasm_qp_polish_wide on the same iterates: the same verdicts, both within the yardstick
    (two methods for one system: the bits may differ)."""
    torch = torch_gpu
    from mpcasm import engine

    qp, constructed, dev, start, status = seven(torch, no, nc, na)
    verdicts = []
    for name, entry in (("narrow", engine.polish_qp), ("wide", engine.polish_qp_wide)):
        got = polish_padded(torch, dev, start, status, entry=entry)
        judge(qp, start, status, got, "%s %dx%d na %d" % (name, no, nc, na))
        verdicts.append(got[3].tolist())
    assert verdicts[0] == verdicts[1]
    assert pr.DONE in verdicts[0]


def test_skipped_when_the_active_set_outgrows_the_unknowns(gpu_api, torch_gpu):
    """(5, 12) with every y positive: na = 12 > no = 5, SKIPPED, nothing written, with and without d_res."""
    torch = torch_gpu
    from mpcasm import engine

    rng = np.random.default_rng(12)
    qps = [pr.complementary_qp(rng, 5, 12, 3) for _ in range(3)]
    P, q, G, h = (torch.as_tensor(np.stack([qp[i] for qp in qps]), device="cuda") for i in range(4))
    sol = engine.solve_qp_wide(P, q, G, h)
    y = (h - sol.z) + 1.0
    before = [t.clone() for t in (sol.x, y, sol.z)]
    x, y, z, verdict, res = engine.polish_qp_wide(P, q, G, h, (sol.x, y, sol.z), status=sol.status)
    assert verdict.tolist() == [capi.POLISH_SKIPPED] * 3
    assert all(torch.equal(a, b) for a, b in zip(before, (x, y, z)))
    assert torch.isnan(res).all()
    verdict.fill_(-99)
    need = engine.qp_polish_wide_info(5, 12, 3)[1]
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc_ = capi.load().mpcasm_qp_polish_wide(5, 12, P.data_ptr(), q.data_ptr(), G.data_ptr(), h.data_ptr(),
                                            x.data_ptr(), y.data_ptr(), z.data_ptr(), None, 1e-6, 3,
                                            verdict.data_ptr(), None, 3, work.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert rc_ == capi.OK and verdict.tolist() == [capi.POLISH_SKIPPED] * 3
    assert all(torch.equal(a, b) for a, b in zip(before, (x, y, z)))


def judge_solved(qp, plain, polished, what):
    """The check of the assembled batches: every instance against the restatement on the solve's own iterate, those
    nearer than 1e-6 to a tie left out.  ``plain``, ``polished``: numpy (x, y, z, res, status) before and
    (x, y, z, res, verdict) after.  Returns (solved, judged, done, worst ratios)."""
    P, q, G, h = qp
    x0, y0, z0, res0, status = plain
    x1, y1, z1, res1, verdict = polished
    solved = judged = done = 0
    worst = [0.0, 0.0]
    for b in range(P.shape[0]):
        if status[b] != capi.QP_SOLVED:
            assert verdict[b] == pr.SKIPPED, (what, b)
            assert same(x1[b], x0[b]) and same(y1[b], y0[b]) and same(z1[b], z0[b]) and same(res1[b], res0[b])
            continue
        solved += 1
        out = pr.polish(P[b], q[b], G[b], h[b], x0[b], y0[b], z0[b], status=status[b])
        if out.margin < MARGIN:
            continue
        judged += 1
        assert verdict[b] == out.polish, (what, b, int(verdict[b]), out.polish, out.margins)
        if out.polish != pr.DONE:
            assert same(x1[b], x0[b]) and same(y1[b], y0[b]) and same(z1[b], z0[b]) and same(res1[b], res0[b])
            continue
        done += 1
        ratios = accepted(P[b], q[b], G[b], h[b], out, x1[b], y1[b], z1[b], res1[b], (what, b))
        worst = [max(w, r) for w, r in zip(worst, ratios)]
    return solved, judged, done, worst


def test_assembled_c3_polished_after_the_solve(gpu_api, torch_gpu):
    """64 assembled C3 QPs: solve_qp_wide(..., polish=True) against the restatement on solve_qp_wide's own iterates
    (a cold solve is deterministic)."""
    torch = torch_gpu
    from mpcasm import engine

    B = 64
    form, asm, given = c3_batch(gpu_api, B)
    P, q, G, h = (t.clone() for t in asm.assemble(given))
    plain = engine.solve_qp_wide(P, q, G, h)
    sol = engine.solve_qp_wide(P, q, G, h, polish=True)
    assert plain.polish is None and isinstance(sol, engine.PolishedQpSolution)
    assert torch.equal(plain.status, sol.status) and torch.equal(plain.iters, sol.iters)
    qp = tuple(t.cpu().numpy() for t in (P, q, G, h))
    before = tuple(t.cpu().numpy() for t in (plain.x, plain.y, plain.z, plain.res, plain.status))
    after = tuple(t.cpu().numpy() for t in (sol.x, sol.y, sol.z, sol.res, sol.polish))
    solved, judged, done, worst = judge_solved(qp, before, after, "c3")
    assert solved > 0 and judged >= 0.9 * solved, (judged, solved)
    assert done > 0, (done, judged)
    record("c3-64", "primal %.3f  dual %.3f  (%d solved, %d judged, %d DONE)" % (worst[0], worst[1], solved, judged, done))


def test_the_ltv_loop_polishes(gpu_api, torch_gpu):
    """LtvLoop on rollout_cases' loop: polish=False is the loop built without the argument, bit for bit; polish=True
    polishes the solved instances and only them, and the first tick's polished points meet the yardstick."""
    torch = torch_gpu
    from mpcasm.ltv_loop import LtvLoop

    form, A, B, given0 = rc.loop_inputs(gpu_api)
    dev = lambda v: torch.as_tensor(v, device="cuda")

    def build(**kw):
        loop = LtvLoop(form, "LIP", rc.LOOP_BATCH, dev(A), dev(B), **kw)
        loop.given.copy_(dev(given0))
        return loop

    plain, off, on = build(), build(polish=False), build(polish=True)
    a, b = plain.run(3, record=True), off.run(3, record=True)
    assert set(a) == set(b) == {"status", "iters", "given"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert set(build(polish=False).step()) == {"x", "status", "iters"}
    # the first tick of the polishing loop, against the restatement on that tick's QPs and the plain loop's iterate
    ref = build()
    P, q, G, h = (t.clone() for t in ref.asm.assemble(ref.given))
    ref.step()
    seen, polished = ref.stage.buffers, on.stage.buffers      # (the loops' solver buffers, by name)
    before = tuple(seen[k].cpu().numpy().copy() for k in ("x", "y", "z", "res", "status"))
    out = on.step()
    assert set(out) == {"x", "status", "iters", "polish"}
    assert torch.equal(out["status"], seen["status"]) and torch.equal(out["iters"], seen["iters"])
    after = tuple(t.cpu().numpy().copy() for t in (polished["x"], polished["y"], polished["z"], polished["res"], out["polish"]))
    solved, judged, done, worst = judge_solved(tuple(t.cpu().numpy() for t in (P, q, G, h)), before, after, "ltv tick 0")
    assert done > 0, (solved, judged, done)
    record("ltv-loop-tick0", "primal %.3f  dual %.3f  (%d solved, %d judged, %d DONE)" % (worst[0], worst[1], solved, judged, done))
    # three ticks in all
    rest = on.run(2)
    assert set(rest) == {"status", "iters", "polish"}
    status = torch.cat([out["status"][None], rest["status"]])
    verdicts = torch.cat([out["polish"][None], rest["polish"]])
    assert set(verdicts.unique().tolist()) <= {capi.POLISH_DONE, capi.POLISH_SKIPPED, capi.POLISH_REJECTED}
    assert bool(((status == capi.QP_SOLVED) | (verdicts == capi.POLISH_SKIPPED)).all())
    assert int((verdicts == capi.POLISH_DONE).sum()) > 0
    assert bool((status != capi.QP_SOLVED).any())          # (instance 1 is primal infeasible: skipped)


def test_a_polished_c3_tick_captured_in_one_graph(gpu_api, torch_gpu):
    """assemble + solve_qp_wide + polish_qp_wide of 64 C3 instances in one graph, a single chain on one stream, the
    results and the workspace at fixed addresses: two replays on new `given` equal the eager calls bit for bit."""
    torch = torch_gpu
    from mpcasm import engine

    B = 64
    form, asm, given = c3_batch(gpu_api, B, seed=9)
    no, nc = asm.no, asm.nc
    f, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    gbuf = torch.as_tensor(given, device="cuda")
    out = (torch.zeros((B, no), **f), torch.zeros((B, nc), **f), torch.zeros((B, nc), **f), torch.zeros(B, **i32),
           torch.zeros(B, **i32), torch.zeros((B, 2), **f))
    verdict = torch.zeros(B, **i32)
    work = torch.empty(engine.qp_polish_wide_info(no, nc, B)[1], dtype=torch.uint8, device="cuda")

    def tick(g, out, verdict, work):
        P, q, G, h = asm.assemble(g)
        sol = engine.solve_qp_wide(P, q, G, h, out=out)
        engine.polish_qp_wide(P, q, G, h, sol, status=sol.status, out=(verdict, sol.res), work=work)
        return sol

    tick(gbuf, out, verdict, work)                     # (shapes warmed, the LDS limit raised outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick(gbuf, out, verdict, work)
    rng = np.random.default_rng(10)
    for _ in range(2):
        new = given + rng.normal(0, 0.01, given.shape)
        gbuf.copy_(torch.as_tensor(new, device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in out + (verdict,)]
        fresh = tuple(torch.zeros_like(t) for t in out)
        v2 = torch.zeros(B, **i32)
        tick(torch.as_tensor(new, device="cuda"), fresh, v2, torch.empty_like(work))
        torch.cuda.synchronize()
        for a, b in zip(replayed, fresh + (v2,)):
            assert torch.equal(bits64(a), bits64(b))
        assert int((v2 == capi.POLISH_DONE).sum()) > 0


def bits64(t):
    import torch

    return t.view(torch.int64) if t.dtype == torch.float64 else t
