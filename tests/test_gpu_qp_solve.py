"""mpcasm_qp_solve (K5's solve mode): OSQP's ADMM with its stopping rules, infeasibility certificates and
adaptive rho, every instance of a batch on its own, against tests/osqp_restatement.py instance by instance:
status, iteration count, final rho and the iterate.  Every instance used here is one whose decisions lie
far (more than 1e-6 relative) from a tie, so that sums rounded in another order cannot flip them; the
tests assert that of the restatement's record rather than trust it."""
import numpy as np
import pytest

import osqp_restatement as rs
import solver_reference as sr
from helpers import assert_close
from mpcasm import problems
from oracle import admm_oracle as ao

pytestmark = pytest.mark.gpu
TOL = 1e-10
MARGIN = 1e-6
SHAPES = [(36, 76), (5, 3), (70, 10), (64, 65), (33, 200), (7, 0)]
SHAPE_IDS = ["biped", "tiny", "wide", "edge", "tall", "free"]


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def to_dev(torch, *arrays):
    return [torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in arrays]


def mixed_batch(no, nc, seed):
    """Solvable instances, then one primal-infeasible (where there are two rows to contradict each other),
    one dual-infeasible and one with an indefinite P, in one batch of one shape."""
    rng = np.random.default_rng(seed)
    qps = [rs.random_qp(rng, no, nc) for _ in range(5)]
    if nc >= 2:
        qps.append(rs.primal_infeasible_qp(rng, no, nc))
    qps.append(rs.dual_infeasible_qp(rng, no, nc))
    P, q, G, h = rs.random_qp(rng, no, nc)
    qps.append((-50.0 * np.eye(no), q, G, h))
    return [np.stack(a) for a in zip(*qps)]


def expected(P, q, G, h, **kw):
    out = [rs.solve(P[b], q[b], G[b], h[b], **kw) for b in range(P.shape[0])]
    for b, s in enumerate(out):
        assert s.margin > MARGIN, "instance %d decides within %.1e of a tie: pick another" % (b, s.margin)
    return out


def assert_matches(sol, ref, b, what="", tol=TOL):
    assert int(sol.status[b]) == ref.status, (what, b, int(sol.status[b]), ref.status)
    assert int(sol.iters[b]) == ref.iters, (what, b, int(sol.iters[b]), ref.iters)
    assert np.isclose(float(sol.rho[b]), ref.rho, rtol=1e-9, atol=0), (what, b, float(sol.rho[b]), ref.rho)
    if ref.status == rs.NON_CVX:
        for t in (sol.x, sol.y, sol.z, sol.res):
            assert bool(t[b].isnan().all())
        return
    assert_close(sol.x[b].cpu().numpy(), ref.x, tol, "%s x[%d]" % (what, b))
    # (y moves by rho times z-sized terms: where every limit lets go -- a dual-infeasible instance running off
    # along a direction all rows fall along -- y is rounding around 0, measured against rho |z|)
    ydev = sol.y[b].cpu().numpy()
    yscale = max(np.abs(ref.y).max(initial=0.0), ref.rho * np.abs(ref.z).max(initial=0.0))
    assert np.abs(ydev - ref.y).max(initial=0.0) <= tol * yscale, "%s y[%d]" % (what, b)
    assert_close(sol.z[b].cpu().numpy(), ref.z, tol, "%s z[%d]" % (what, b))
    assert np.allclose(sol.res[b].cpu().numpy(), ref.res, rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("no,nc", SHAPES, ids=SHAPE_IDS)
def test_a_mixed_batch_against_the_restatement(gpu_api, torch_gpu, no, nc):
    """Solvable, primal-infeasible, dual-infeasible and indefinite instances in the same launch, OSQP's
    defaults: every instance's status, iterations, final rho and iterate are the restatement's."""
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h = mixed_batch(no, nc, no * 1000 + nc)
    ref = expected(P, q, G, h)
    sol = engine.solve_qp(*to_dev(torch, P, q, G, h))
    for b in range(P.shape[0]):
        # (the kernel applies an explicit K^-1, the restatement solves with K: they differ by rounding times
        # K's condition -- 1e-10 everywhere but for the dual-infeasible instance without rows, whose K is
        # P + sigma I with P singular: cond ~ 1e7)
        K = P[b] + ao.SIGMA * np.eye(no) + ref[b].rho * G[b].T @ G[b]
        assert_matches(sol, ref[b], b, tol=max(TOL, 1e-14 * np.linalg.cond(K)) if ref[b].status != rs.NON_CVX else TOL)
    got = sorted(set(int(s) for s in sol.status.cpu()))
    assert got == sorted({1, -4, -7} | ({-3} if nc >= 2 else set()))


def early_exit_batch():
    """Three instances of one shape that stop at 25, at about a hundred and at over a thousand iterations
    (eps 1e-5, rho fixed per instance): q = 0 (x = 0 is the solution from the start), a random QP at
    rho = 1, the same QP at rho = 3e-3."""
    rng = np.random.default_rng(4)
    P, q, G, h = rs.random_qp(rng, 12, 30)
    qps = [(P, np.zeros(12), G, h), (P, q, G, h), (P, q, G, h)]
    return [np.stack(a) for a in zip(*qps)] + [np.array([1.0, 1.0, 3e-3])]


EARLY = dict(eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=0)


def test_every_instance_stops_on_its_own(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h, rho = early_exit_batch()
    ref = [rs.solve(P[b], q[b], G[b], h[b], rho=rho[b], **EARLY) for b in range(3)]
    assert [s.margin > MARGIN for s in ref] == [True] * 3
    assert [s.status for s in ref] == [rs.SOLVED] * 3
    assert ref[0].iters == 25 and 50 <= ref[1].iters <= 250 and ref[2].iters > 1000
    sol = engine.solve_qp(*to_dev(torch, P, q, G, h), rho=torch.as_tensor(rho, device="cuda"), **EARLY)
    for b in range(3):
        assert_matches(sol, ref[b], b, "early")
        # (its iterate is the plain iteration's after ITS count, not after the slowest instance's)
        xo, yo, zo, _ = ao.admm(P[b], q[b], G[b], h[b], iters=ref[b].iters, rho=rho[b])
        assert_close(sol.x[b].cpu().numpy(), xo, TOL, "x"), assert_close(sol.y[b].cpu().numpy(), yo, TOL, "y")
    assert len(set(sol.iters.tolist())) == 3


def biped_fleet(api, B, seed=8, scale=0.001):
    form = problems.biped(api, problems.BipedConfig(step_samples=8))
    form.update(step_times=np.array([6, 14]), step_count=0)
    rng = np.random.default_rng(seed)
    return form, rng.normal(0, scale, [B, form.given_len])


def host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def test_adaptive_rho_and_the_inverse_it_leaves(gpu_api, torch_gpu):
    """Bipeds from rho = 0.1 (OSQP's default): the step moves, to where the restatement moves it, and the
    K^-1 written back is the inverse for the final rho."""
    torch = torch_gpu
    from mpcasm import engine

    form, given = biped_fleet(gpu_api, 16, seed=11)
    P, q, G, h = engine.Assembler(form, batch=16).assemble(given)
    kinv = torch.full(tuple(P.shape), float("nan"), dtype=torch.float64, device="cuda")
    sol = engine.solve_qp(P, q, G, h, kinv=kinv)
    Pn, qn, Gn, hn = host(P, q, G, h)
    ref = expected(Pn, qn, Gn, hn)
    for b in range(16):
        assert_matches(sol, ref[b], b, "adaptive")
    moved = [b for b in range(16) if ref[b].rho_changes]
    assert moved and all(float(sol.rho[b]) != engine.OSQP_RHO for b in moved)
    for b in (moved[0], moved[-1], 0):
        r = float(sol.rho[b])
        Kref = np.linalg.inv(Pn[b] + engine.OSQP_SIGMA * np.eye(Pn.shape[1]) + r * Gn[b].T @ Gn[b])
        assert_close(kinv[b].cpu().numpy(), Kref, 1e-9, "K^-1 for the final rho")
        # (and within the forward bound no u kappa2 |X*|_2 of the long-double inverse, whatever rho came out)
        sr.assert_inverse(kinv[b].cpu().numpy(), Pn[b], Gn[b], r, engine.OSQP_SIGMA, "K^-1 for the final rho")


def test_a_fleet_from_the_assembly_to_solutions(gpu_api, torch_gpu):
    """4 096 walkers, mpcasm_assemble then mpcasm_qp_solve with OSQP's defaults: every one solved and
    meeting its own stopping inequalities (recomputed here with torch; the slack 1e-9 relative allows for
    sums rounded in another order), 64 sampled ones the restatement's."""
    torch = torch_gpu
    from mpcasm import engine

    B = 4096
    form, given = biped_fleet(gpu_api, B)
    P, q, G, h = engine.Assembler(form, batch=B).assemble(given)
    sol = engine.solve_qp(P, q, G, h)
    status = sol.status.cpu().numpy()
    bad = np.flatnonzero(status != rs.SOLVED)
    assert bad.size == 0, "%d of %d not solved (statuses %s, iterations %s)" % (
        bad.size, B, np.unique(status[bad]).tolist(), sol.iters[bad[:8].tolist()].tolist())
    x, y, z = sol.x, sol.y, sol.z
    inf = lambda t: t.abs().amax(dim=1)
    Gx = torch.einsum("brc,bc->br", G, x)
    Px = torch.einsum("bij,bj->bi", P, x)
    Gty = torch.einsum("brc,br->bc", G, y)
    rp, rd = inf(Gx - z), inf(Px + q + Gty)
    tp = 1e-3 + 1e-3 * torch.maximum(inf(Gx), inf(z))
    td = 1e-3 + 1e-3 * torch.maximum(torch.maximum(inf(Px), inf(Gty)), inf(q))
    assert bool((rp <= tp * (1 + 1e-9)).all()) and bool((rd <= td * (1 + 1e-9)).all())
    assert torch.allclose(sol.res[:, 0], rp, rtol=1e-9, atol=1e-15)
    assert int(sol.iters.min()) >= 25 and int(sol.iters.max()) < 4000
    # 64 walkers against the restatement on the same matrices (those far from a tie)
    rng = np.random.default_rng(1)
    checked = 0
    for b in rng.choice(B, 80, replace=False):
        Pn, qn, Gn, hn = host(P[b], q[b], G[b], h[b])
        ref = rs.solve(Pn, qn, Gn, hn)
        if ref.margin <= MARGIN:
            continue
        assert_matches(sol, ref, b, "fleet")
        checked += 1
        if checked == 64:
            break
    assert checked == 64


def test_the_next_tick_reuses_the_inverse_and_the_step(gpu_api, torch_gpu):
    """A tick, then the next with a new `given` (P and G unchanged) warm from the last iterate: handing the
    K^-1 and rho the first call left back in gives, bit for bit, what factoring again gives."""
    torch = torch_gpu
    from mpcasm import engine

    B = 256
    form, given = biped_fleet(gpu_api, B, seed=5)
    asm = engine.Assembler(form, batch=B)
    P, q, G, h = asm.assemble(given)
    P1 = P.clone()
    kinv = torch.empty(tuple(P.shape), dtype=torch.float64, device="cuda")
    rho = torch.full((B,), engine.OSQP_RHO, dtype=torch.float64, device="cuda")
    first = engine.solve_qp(P, q, G, h, rho=rho, kinv=kinv)
    assert first.rho.data_ptr() == rho.data_ptr() and bool((rho != engine.OSQP_RHO).any())
    given2 = given + np.random.default_rng(6).normal(0, 0.0005, given.shape)
    P, q, G, h = asm.assemble(given2)
    assert torch.equal(P, P1)
    runs = []
    for valid in (True, False):
        start = [t.clone() for t in (first.x, first.y, first.z)]
        k = kinv.clone()
        runs.append(engine.solve_qp(P, q, G, h, *start, rho=rho.clone(), kinv=k, kinv_valid=valid) + (k,))
    kept, fresh = runs
    for a, b in zip(kept, fresh):
        assert torch.equal(a, b)
    assert bool((kept[3] == rs.SOLVED).all())


def test_a_tick_captured_in_one_graph(gpu_api, torch_gpu):
    """assemble and solve_qp captured in one graph on one stream, nothing read back in between: replays
    for three new `given` give the eager results."""
    torch = torch_gpu
    from mpcasm import engine

    B = 64
    form, given = biped_fleet(gpu_api, B, seed=9)
    asm = engine.Assembler(form, batch=B)
    gbuf = torch.as_tensor(given, device="cuda")
    engine.solve_qp(*asm.assemble(gbuf))          # (once as it is: kernels loaded, buffers there)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = engine.solve_qp(*asm.assemble(gbuf))
    rng = np.random.default_rng(10)
    for _ in range(3):
        new = rng.normal(0, 0.001, given.shape)
        gbuf.copy_(torch.as_tensor(new, device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured]
        eager = engine.solve_qp(*asm.assemble(torch.as_tensor(new, device="cuda")))
        for a, b in zip(replayed, eager):
            assert torch.equal(a, b)
        assert bool((eager.status == rs.SOLVED).all())


def test_what_the_solve_refuses_and_its_edges(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import capi, engine

    rng = np.random.default_rng(2)
    P, q, G, h = (np.stack(a) for a in zip(*[rs.random_qp(rng, 6, 4) for _ in range(3)]))
    dP, dq, dG, dh = to_dev(torch, P, q, G, h)
    for kw in (dict(eps_abs=-1e-3), dict(eps_rel=float("inf")), dict(eps_prim_inf=float("nan")),
               dict(eps_dual_inf=-1.0), dict(max_iter=-1), dict(check_every=0), dict(adaptive_rho_interval=-25),
               dict(adaptive_rho_interval=30), dict(sigma=0.0), dict(alpha=2.0)):
        with pytest.raises(capi.MpcasmError) as err:
            engine.solve_qp(dP, dq, dG, dh, **kw)
        assert err.value.status == -1, kw
    with pytest.raises(ValueError):
        engine.solve_qp(dP, dq, dG, dh, rho=torch.ones(2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        engine.solve_qp(dP, dq, dG, dh, kinv_valid=True)
    # C3's QP (96 unknowns, 196 limits) does not fit in LDS: said so, nothing launched
    big = to_dev(torch, *(np.stack(a) for a in zip(*[rs.random_qp(rng, 96, 196) for _ in range(2)])))
    with pytest.raises(capi.MpcasmError) as err:
        engine.solve_qp(*big)
    assert err.value.status == capi.ERR_LIMIT
    with pytest.raises(capi.MpcasmError) as err:
        engine.qp_solve_lds_bytes(96, 196)
    assert err.value.status == capi.ERR_LIMIT
    # the biped's instance takes what mpcasm_admm's does: four per CU (160 KiB / 4 = 40 960 B)
    assert engine.qp_solve_lds_bytes(36, 76) == 40320 <= 160 * 1024 // 4
    # rho <= 0: checked on the device, that instance alone not convex
    sol = engine.solve_qp(dP, dq, dG, dh, rho=torch.tensor([1.0, 0.0, -1.0], dtype=torch.float64, device="cuda"))
    assert sol.status.tolist()[1:] == [rs.NON_CVX] * 2 and sol.iters.tolist()[1:] == [0, 0]
    assert sol.status.tolist()[0] == rs.SOLVED and bool(sol.x[1:].isnan().all())
    # no iteration at all; all four eps 0; a check after every iteration
    sol = engine.solve_qp(dP, dq, dG, dh, max_iter=0)
    assert sol.status.tolist() == [rs.MAX_ITER] * 3 and sol.iters.tolist() == [0] * 3
    assert not bool(sol.x.any())
    zero = dict(eps_abs=0, eps_rel=0, eps_prim_inf=0, eps_dual_inf=0)
    sol = engine.solve_qp(dP, dq, dG, dh, max_iter=60, **zero)
    assert sol.iters.tolist() == [60] * 3 and sol.status.tolist() == [rs.MAX_ITER] * 3
    for kw in (dict(check_every=1, adaptive_rho_interval=0), dict(check_every=1, adaptive_rho_interval=7)):
        ref = expected(P, q, G, h, **kw)
        sol = engine.solve_qp(dP, dq, dG, dh, **kw)
        for b in range(3):
            assert_matches(sol, ref[b], b, str(kw))
