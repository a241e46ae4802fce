"""mpcasm_qp_solve_soft (``engine.solve_qp(soft=...)``): the solve to tolerance with soft limits, against
tests/soft_restatement.py instance by instance -- status, iteration count, final rho and the iterate -- with
test_gpu_qp_solve.py's ``assert_matches`` (soft_cases.assert_matches: the same checks on every instance, none left
out; the residuals' absolute slack and rho's bound derived per instance, see there), its TOL scaled by cond(K) and
its MARGIN; against the hard entry bit for bit where every row is hard; and against the slack QP solved on the CPU."""
import numpy as np
import pytest

import osqp_restatement as rs
import soft_cases as sc
import soft_restatement as ss
from mpcasm import problems
from test_gpu_qp_solve import to_dev

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (5, 9), (36, 76), (12, 257), (65, 70)]
SHAPE_IDS = ["one lane", "tiny", "biped", "second trip of the rows", "more unknowns than lanes"]
FIELDS = ("x", "y", "z", "status", "iters", "res", "rho")


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def same_bits(torch, a, b, what=""):
    """Two solutions, field by field, bit for bit (NaN where NaN)."""
    for name, u, v in zip(FIELDS, a, b):
        assert torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u,
                           v.view(torch.int64) if v.dtype == torch.float64 else v), (what, name)


@pytest.mark.parametrize("no,nc", SHAPES, ids=SHAPE_IDS)
def test_a_mixed_batch_against_the_restatement(gpu_api, torch_gpu, no, nc):
    """Solvable, contradicting-pair (kept hard: infeasible; soft: solved), dual-infeasible and indefinite instances
    in one launch, per-instance penalties mixing hard and soft rows, OSQP's defaults, adaptive rho moving.  The seeds
    (soft_cases.SEED_OFFSETS) exclude a dual-infeasible instance that changes rho away from the clips: that adaptive
    step is not covered here."""
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h, lin, quad = sc.mixed_batch(no, nc, sc.seed(no, nc))
    ref = sc.expected(P, q, G, h, lin, quad)
    sol = engine.solve_qp(*to_dev(torch, P, q, G, h), soft=tuple(to_dev(torch, lin, quad)))
    for b in range(P.shape[0]):
        sc.assert_matches(sol, ref[b], b, tol=sc.tolerance(P[b], G[b], ref[b]), P=P[b], G=G[b])
    got = sorted(set(int(s) for s in sol.status.cpu()))
    assert got == sorted({1, -4, -7} | ({-3} if nc >= 2 else set()))
    if nc >= 2:
        assert [ref[5].status, ref[6].status] == [rs.PRIMAL_INFEASIBLE, rs.SOLVED]
        assert (G[6] @ ref[6].x - h[6]).max() > 0.1         # (the soft pair is violated in the solution)


@pytest.mark.parametrize("iters", [1, 7, 40])
@pytest.mark.parametrize("no,nc", [(5, 9), (36, 76), (12, 257)], ids=["tiny", "biped", "second trip"])
def test_iterates_at_fixed_counts(gpu_api, torch_gpu, no, nc, iters):
    """Eps 0, rho fixed: the iterates after 1, 7 and 40 iterations are the restatement's (numpy arrays and scalars
    as penalties: the (nc,) pair for the batch, and one scalar pair for every row)."""
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h, lin, quad = sc.mixed_batch(no, nc, sc.seed(no, nc))
    P, q, G, h, lin, quad = (a[:7] for a in (P, q, G, h, lin, quad))      # (all but the indefinite one)
    kw = dict(eps_abs=0, eps_rel=0, eps_prim_inf=0, eps_dual_inf=0, adaptive_rho_interval=0, max_iter=iters)
    dev = to_dev(torch, P, q, G, h)
    for pen in ((lin, quad), (lin[0], quad[0]), (0.7, 0.25)):
        sol = engine.solve_qp(*dev, soft=pen, **kw)
        for b in range(P.shape[0]):
            lv, qv = (pen[0][b], pen[1][b]) if np.ndim(pen[0]) == 2 else pen
            ref = sc.solve(P[b], q[b], G[b], h[b], lv, qv, **kw)
            assert ref.status == rs.MAX_ITER and ref.iters == iters
            sc.assert_matches(sol, ref, b, "after %d" % iters, tol=sc.tolerance(P[b], G[b], ref), P=P[b], G=G[b])


@pytest.mark.parametrize("no,nc", [(36, 76), (65, 70), (7, 0)], ids=["biped", "more unknowns than lanes", "free"])
def test_all_rows_hard_is_the_hard_entry_bit_for_bit(gpu_api, torch_gpu, no, nc):
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h = sc.mixed_batch(no, nc, sc.seed(no, nc))[:4]
    dev = to_dev(torch, P, q, G, h)
    kh, ks = (torch.full(tuple(dev[0].shape), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    hard = engine.solve_qp(*dev, kinv=kh)
    for pen in ((np.inf, 0.0), (np.full((P.shape[0], nc), np.inf), np.full((P.shape[0], nc), 3.0))):
        soft = engine.solve_qp(*dev, kinv=ks.fill_(7.0), soft=pen)
        same_bits(torch, soft, hard, "all hard")
        assert torch.equal(ks.view(torch.int64), kh.view(torch.int64))
    assert len(set(hard.status.tolist())) >= (4 if nc else 3)


def test_stride_zero_is_the_vectors_repeated(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h, lin, quad = sc.mixed_batch(36, 76, sc.seed(36, 76))
    dev = to_dev(torch, P, q, G, h)
    B = P.shape[0]
    one = engine.solve_qp(*dev, soft=(lin[0], quad[0]))
    each = engine.solve_qp(*dev, soft=(np.tile(lin[0], (B, 1)), np.tile(quad[0], (B, 1))))
    same_bits(torch, one, each, "stride")
    assert int((one.status == rs.SOLVED).sum()) >= 5


@pytest.mark.parametrize("no,nc", [(5, 9), (36, 76)], ids=["tiny", "biped"])
def test_soft_against_hard_and_the_slack_qp(gpu_api, torch_gpu, no, nc):
    """Contradicting-pair instances: PRIMAL_INFEASIBLE hard, SOLVED with every row soft at lin = 1e4 (OSQP's
    defaults).  Then both the device and the slack QP on the CPU to ABSOLUTE residuals of 1e-9 (eps_rel = 0: a
    relative one would scale with |q| = lin = 1e4 in the slack QP): x, and y on G's rows, agree to 1e-6 relative,
    the bound test_qp_soft_cpu.py holds the restatement to in the same comparison (the device is within 1e-10
    cond(K) of the restatement; the two restatements were seen 2e-9 apart)."""
    torch = torch_gpu
    from mpcasm import engine

    # (seeds at which both instances are soft_cases.well_posed at lin = 1e4 -- asserted below.  What they exclude: a
    # solve whose rho is sent to the clip 1e6 by the cold start's first, rounding-level dual residual and leaves it
    # again on a primal residual that is rounding: five of the first six seeds at (5, 9); soft_cases.solve has the
    # figures)
    rng = np.random.default_rng(1000 * no + nc + {(5, 9): 5}.get((no, nc), 0))
    qps = [rs.primal_infeasible_qp(rng, no, nc) for _ in range(2)]
    P, q, G, h = (np.stack(a) for a in zip(*qps))
    dev = to_dev(torch, P, q, G, h)
    hard = engine.solve_qp(*dev)
    soft = engine.solve_qp(*dev, soft=(1e4, 0.0))
    assert hard.status.tolist() == [rs.PRIMAL_INFEASIBLE] * 2 and soft.status.tolist() == [rs.SOLVED] * 2
    for b in range(2):
        assert rs.solve(P[b], q[b], G[b], h[b]).margin > sc.MARGIN
        ref = sc.solve(P[b], q[b], G[b], h[b], 1e4, 0.0)
        assert sc.well_posed(ref) and ref.rho_changes >= 2, (b, ref.margin, ref.rho_amp)
        sc.assert_matches(soft, ref, b, "lin 1e4", tol=sc.tolerance(P[b], G[b], ref), P=P[b], G=G[b])
    tight = dict(eps_abs=1e-9, eps_rel=0.0, max_iter=100000)
    sol = engine.solve_qp(*dev, soft=(1e4, 0.0), **tight)
    assert sol.status.tolist() == [rs.SOLVED] * 2
    for b in range(2):
        slack = rs.solve(*ss.slack_qp(P[b], q[b], G[b], h[b], 1e4, 0.0), **tight)
        assert slack.status == rs.SOLVED
        x, y = sol.x[b].cpu().numpy(), sol.y[b].cpu().numpy()
        ex = np.abs(x - slack.x[:no]).max() / np.abs(slack.x[:no]).max()
        ey = np.abs(y - slack.y[:nc]).max() / np.abs(slack.y[:nc]).max()
        print("soft against the slack QP (%d, %d)[%d]: x %.2e, y %.2e relative" % (no, nc, b, ex, ey))
        assert ex <= 1e-6 and ey <= 1e-6, (b, ex, ey)


@pytest.mark.parametrize("seed", [5009, 5011])
def test_the_refactor_at_the_clip_of_rho(gpu_api, torch_gpu, seed):
    """A contradicting pair at lin = 1e4 whose first adaptive step lands far beyond the clip (the cold start's dual
    residual at the first check is rounding, so rho' is ~1e13: both arithmetics take 1e6 itself): K formed, factored
    and inverted again at rho = 1e6, 75 iterations there, stopped before the next step (which would rest on a primal
    residual that rho = 1e6 has driven to rounding: soft_cases.solve).  Status, iterations, rho and iterate the
    restatement's, with the bounds of every other instance."""
    torch = torch_gpu
    from mpcasm import engine

    rng = np.random.default_rng(seed)
    rs.primal_infeasible_qp(rng, 5, 9)
    P, q, G, h = (a[None] for a in rs.primal_infeasible_qp(rng, 5, 9))
    kw = dict(max_iter=175)
    ref = sc.solve(P[0], q[0], G[0], h[0], 1e4, 0.0, **kw)
    assert ref.rho_path == (0.1, rs.RHO_MAX) and ref.status == rs.MAX_ITER and sc.well_posed(ref)
    sol = engine.solve_qp(*to_dev(torch, P, q, G, h), soft=(1e4, 0.0), **kw)
    assert float(sol.rho[0]) == rs.RHO_MAX
    sc.assert_matches(sol, ref, 0, "at the clip", tol=sc.tolerance(P[0], G[0], ref), P=P[0], G=G[0])


def test_bad_penalties_are_that_instances_alone(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h, lin, quad = sc.mixed_batch(36, 76, sc.seed(36, 76))
    P, q, G, h, lin, quad = (np.concatenate([a[:5], a[:3]]) for a in (P, q, G, h, lin, quad))
    lin[5, 75], lin[6, 0], quad[7, 40] = -1.0, np.nan, np.inf          # (the last row, the first, one in between)
    lin[7, 40] = 1.0
    dev = to_dev(torch, P, q, G, h)
    kinv = torch.zeros(tuple(dev[0].shape), dtype=torch.float64, device="cuda")
    sol = engine.solve_qp(*dev, soft=(lin, quad), kinv=kinv)
    assert sol.status.tolist()[5:] == [rs.NON_CVX] * 3 and sol.iters.tolist()[5:] == [0] * 3
    for t in (sol.x, sol.y, sol.z, sol.res, kinv):
        assert bool(t[5:].isnan().all()) and not bool(t[:5].isnan().any())
    good = engine.solve_qp(*(t[:5].contiguous() for t in dev), soft=(lin[:5], quad[:5]))
    same_bits(torch, [t[:5] for t in sol], good, "beside bad penalties")
    assert good.status.tolist() == [rs.SOLVED] * 5


def biped_fleet(api, B, seed, scale):
    form = problems.biped(api, problems.BipedConfig(step_samples=8))
    form.update(step_times=np.array([6, 14]), step_count=0)
    return form, np.random.default_rng(seed).normal(0, scale, [B, form.given_len])


def test_reuse_across_a_change_of_rho(gpu_api, torch_gpu):
    """Disturbed bipeds (some of them infeasible hard), every row soft.  One launch whose adaptive step fires: the
    restatement's number of changes and final rho.  Then a second solve from the first's outputs -- x, y, z warm,
    rho and K^-1 handed back (``kinv_valid``), so a K^-1 that was refreshed when rho moved -- stops at its first
    check; factoring again instead gives the same bits."""
    torch = torch_gpu
    from mpcasm import engine

    B = 16
    form, given = biped_fleet(gpu_api, B, 29, 0.02)     # (the first seed from 11 on with all 16 well posed)
    P, q, G, h = engine.Assembler(form, batch=B).assemble(given)
    pen = (1e3, 0.0)
    kinv = torch.empty(tuple(P.shape), dtype=torch.float64, device="cuda")
    rho = torch.full((B,), engine.OSQP_RHO, dtype=torch.float64, device="cuda")
    first = engine.solve_qp(P, q, G, h, rho=rho, kinv=kinv, soft=pen)
    Pn, qn, Gn, hn = (t.cpu().numpy() for t in (P, q, G, h))
    moved = 0
    for b in range(B):
        ref = sc.solve(Pn[b], qn[b], Gn[b], hn[b], *pen)
        assert sc.well_posed(ref), (b, ref.margin, ref.rho_amp)
        sc.assert_matches(first, ref, b, "adaptive", tol=sc.tolerance(Pn[b], Gn[b], ref), P=Pn[b], G=Gn[b])
        moved += ref.rho_changes > 0
    assert moved == B and first.status.tolist() == [rs.SOLVED] * B
    runs = []
    for valid in (True, False):
        start = [t.clone() for t in (first.x, first.y, first.z)]
        k = kinv.clone()
        runs.append(engine.solve_qp(P, q, G, h, *start, rho=rho.clone(), kinv=k, kinv_valid=valid, soft=pen) + (k,))
    kept, fresh = runs
    for a, b in zip(kept, fresh):
        assert torch.equal(a, b)
    assert kept[3].tolist() == [rs.SOLVED] * B and kept[4].tolist() == [25] * B      # (status, iters)


def test_a_tick_captured_in_one_graph(gpu_api, torch_gpu):
    """assemble and solve_qp(soft=) captured in one graph, the penalties device tensors at stride 0: replays under
    set_sync_debug_mode("error") give the eager results."""
    torch = torch_gpu
    from mpcasm import engine

    B = 64
    form, given = biped_fleet(gpu_api, B, 9, 0.02)
    asm = engine.Assembler(form, batch=B)
    pen = asm.soft_rows({k: (1e3, 0.5) for k in range(len(asm.plan.limit_rows))})
    assert pen[0].is_cuda and tuple(pen[0].shape) == (asm.nc,)
    gbuf = torch.as_tensor(given, device="cuda")
    engine.solve_qp(*asm.assemble(gbuf), soft=pen)          # (once as it is: kernels loaded, buffers there)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = engine.solve_qp(*asm.assemble(gbuf), soft=pen)
    rng = np.random.default_rng(10)
    for _ in range(3):
        new = torch.as_tensor(rng.normal(0, 0.02, given.shape), device="cuda")
        gbuf.copy_(new)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            graph.replay()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured]
        eager = engine.solve_qp(*asm.assemble(new), soft=pen)
        for a, b in zip(replayed, eager):
            assert torch.equal(a, b)
        assert bool((eager.status == rs.SOLVED).all())


def test_what_the_soft_entry_refuses(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import capi, engine

    rng = np.random.default_rng(2)
    P, q, G, h = (np.stack(a) for a in zip(*[rs.random_qp(rng, 6, 4) for _ in range(3)]))
    dev = to_dev(torch, P, q, G, h)
    for pen in ((np.ones(3), np.zeros(3)), (np.ones((2, 4)), np.zeros((2, 4))), (np.ones(4), np.zeros((3, 4))), 1.0,
                (1.0,)):
        with pytest.raises(ValueError):
            engine.solve_qp(*dev, soft=pen)
    with pytest.raises(ValueError, match="polish"):
        engine.solve_qp(*dev, soft=(1.0, 0.0), polish=True)
    with pytest.raises(capi.MpcasmError) as err:
        engine.solve_qp(*dev, soft=(1.0, 0.0), max_iter=-1)
    assert err.value.status == capi.ERR_ARG
    # (36, 391): the hard entry's LDS fits, the soft entry's two vectors more do not -- said so, nothing launched
    big = to_dev(torch, *(np.stack(a) for a in zip(*[rs.random_qp(rng, 36, 391) for _ in range(2)])))
    assert engine.qp_solve_lds_bytes(36, 391) < engine.qp_solve_soft_lds_bytes(36, 390)
    engine.solve_qp(*big, max_iter=25)
    with pytest.raises(capi.MpcasmError) as err:
        engine.solve_qp(*big, soft=(1.0, 0.0))
    assert err.value.status == capi.ERR_LIMIT
