"""mpcasm_qp_solve_wide: the solve to tolerance for QPs whose matrices do not fit on chip (G read in place,
K^-1 in LDS or in d_kinv), against tests/osqp_restatement.py instance by instance as tests/test_gpu_qp_solve.py
holds mpcasm_qp_solve: status, iteration count, final rho and the iterate, on instances whose decisions lie
more than 1e-6 from a tie (asserted on the restatement's record)."""
import numpy as np
import pytest

import osqp_restatement as rs
import solver_reference as sr
from helpers import assert_close
from mpcasm import problems
from oracle import admm_oracle as ao
from test_gpu_qp_solve import MARGIN, SHAPE_IDS, SHAPES, TOL, expected, host, mixed_batch, to_dev

pytestmark = pytest.mark.gpu
WIDE_SHAPES = [(96, 196), (200, 404), (130, 0), (65, 300), (1, 1)]
WIDE_IDS = ["c3", "c5", "free130", "mid", "one"]


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def assert_matches(sol, ref, b, what="", tol=TOL, P=None, G=None):
    """tests/test_gpu_qp_solve.py's check with two bounds scaled to the instance.  rho is computed from the
    iterate's residuals, which are differences of iterates and carry a larger relative error than the iterate:
    rtol max(1e-9, 10 tol) (tol > 1e-10 only where K's condition makes it so -- assembled C3 instances after
    two or three changes of rho: 1.3e-8 and 1.4e-8 measured against tol 1.2e-8).  The residuals of an instance
    that runs off (dual infeasible, |x| ~ 1e6) are rounding of |P| |x|- and |z|-sized terms, summed here in
    another order: absolute slack 1e-13 of that size (1e-12 at least)."""
    assert int(sol.status[b]) == ref.status, (what, b, int(sol.status[b]), ref.status)
    assert int(sol.iters[b]) == ref.iters, (what, b, int(sol.iters[b]), ref.iters)
    assert np.isclose(float(sol.rho[b]), ref.rho, rtol=max(1e-9, 10 * tol), atol=0), (what, b, float(sol.rho[b]), ref.rho)
    if ref.status == rs.NON_CVX:
        for t in (sol.x, sol.y, sol.z, sol.res):
            assert bool(t[b].isnan().all())
        return
    assert_close(sol.x[b].cpu().numpy(), ref.x, tol, "%s x[%d]" % (what, b))
    ydev = sol.y[b].cpu().numpy()
    yscale = max(np.abs(ref.y).max(initial=0.0), ref.rho * np.abs(ref.z).max(initial=0.0))
    assert np.abs(ydev - ref.y).max(initial=0.0) <= tol * yscale, "%s y[%d]" % (what, b)
    assert_close(sol.z[b].cpu().numpy(), ref.z, tol, "%s z[%d]" % (what, b))
    size = np.abs(ref.z).max(initial=0.0)
    for M in (P, G):
        if M is not None and M.size:
            size = max(size, np.abs(M).sum(axis=1).max() * np.abs(ref.x).max())
    slack = max(1e-12, 1e-13 * size)
    assert np.allclose(sol.res[b].cpu().numpy(), ref.res, rtol=1e-6, atol=slack), (what, b, sol.res[b], ref.res)


def tol_for(P, G, ref, b):
    """assert_matches' bound for instance b: rounding times K's condition (the kernel applies an explicit
    K^-1, the restatement solves with K)."""
    if ref[b].status == rs.NON_CVX:
        return TOL
    K = P[b] + ao.SIGMA * np.eye(P.shape[1]) + ref[b].rho * G[b].T @ G[b]
    return max(TOL, 1e-14 * np.linalg.cond(K))


def check_mixed(torch, no, nc, seed=None):
    from mpcasm import engine

    P, q, G, h = mixed_batch(no, nc, no * 1000 + nc if seed is None else seed)
    ref = expected(P, q, G, h)
    sol = engine.solve_qp_wide(*to_dev(torch, P, q, G, h))
    for b in range(P.shape[0]):
        assert_matches(sol, ref[b], b, "wide %dx%d" % (no, nc), tol=tol_for(P, G, ref, b), P=P[b], G=G[b])
    got = sorted(set(int(s) for s in sol.status.cpu()))
    assert got == sorted({1, -4, -7} | ({-3} if nc >= 2 else set()))


@pytest.mark.parametrize("no,nc", WIDE_SHAPES, ids=WIDE_IDS)
def test_a_wide_mixed_batch_against_the_restatement(gpu_api, torch_gpu, no, nc):
    """Solvable, primal-infeasible, dual-infeasible and indefinite instances of shapes the LDS path refuses
    (and two it takes), OSQP's defaults.  (1 x 1 with seed 1: the default seed's second instance changes rho
    on a primal residual 6e-11 of its scale, rounding that picks the new rho.)"""
    check_mixed(torch_gpu, no, nc, seed=1 if (no, nc) == (1, 1) else None)


def test_the_largest_shape(gpu_api, torch_gpu):
    """C4's shape, 384 unknowns and 1 536 limits: two solvable instances and a primal-infeasible one."""
    torch = torch_gpu
    from mpcasm import engine

    rng = np.random.default_rng(384)
    qps = [rs.random_qp(rng, 384, 1536) for _ in range(2)] + [rs.primal_infeasible_qp(rng, 384, 1536)]
    P, q, G, h = (np.stack(a) for a in zip(*qps))
    ref = expected(P, q, G, h)
    assert [s.status for s in ref] == [rs.SOLVED, rs.SOLVED, rs.PRIMAL_INFEASIBLE]
    sol = engine.solve_qp_wide(*to_dev(torch, P, q, G, h))
    for b in range(3):
        assert_matches(sol, ref[b], b, "c4 shape", tol=tol_for(P, G, ref, b), P=P[b], G=G[b])


@pytest.mark.parametrize("no,nc", SHAPES, ids=SHAPE_IDS)
def test_both_paths_where_both_apply(gpu_api, torch_gpu, no, nc):
    """The LDS path's six shapes through the wide path: the same restatement checks."""
    check_mixed(torch_gpu, no, nc)


@pytest.mark.parametrize("kw", [dict(check_every=1, adaptive_rho_interval=0),
                                dict(check_every=1, adaptive_rho_interval=7),
                                dict(max_iter=0),
                                dict(max_iter=60, eps_abs=0, eps_rel=0, eps_prim_inf=0, eps_dual_inf=0)],
                         ids=["every1", "every1_rho7", "none", "eps0"])
def test_adaptive_rho_and_early_exit(gpu_api, torch_gpu, kw):
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h = mixed_batch(96, 196, 17)
    ref = expected(P, q, G, h, **kw)
    sol = engine.solve_qp_wide(*to_dev(torch, P, q, G, h), **kw)
    for b in range(P.shape[0]):
        assert_matches(sol, ref[b], b, str(kw), tol=tol_for(P, G, ref, b), P=P[b], G=G[b])
    if kw.get("max_iter") == 0:
        assert sol.iters.tolist() == [0] * P.shape[0]
    if "adaptive_rho_interval" in kw and kw["adaptive_rho_interval"] == 7:
        assert any(s.rho_changes for s in ref)


def c3_batch(api, B, seed=31):
    from mpcasm import engine

    form = problems.lipm3d(api, N=32)
    rng = np.random.default_rng(seed)
    asm = engine.Assembler(form, batch=B)
    given = rng.normal(0, 0.02, [B, form.given_len])
    given[:, 6] += 0.85   # (CoM_z inside the height band 0.75 .. 0.95: most instances solvable)
    return form, asm, given


def sampled_matches(sol, P, q, G, h, B, count=16, seed=1):
    rng = np.random.default_rng(seed)
    checked = 0
    for b in rng.choice(B, 4 * count, replace=False):
        Pn, qn, Gn, hn = host(P[b], q[b], G[b], h[b])
        ref = rs.solve(Pn, qn, Gn, hn)
        if ref.margin <= MARGIN:
            continue
        # (assembled C3: K's condition times 1e-13, not 1e-14 -- an instance's iterate carries the rounding of
        # every K^-1 along its path of rho; 5.0e-9 measured where 1e-14 cond(K) gives 4.2e-9)
        K = Pn + ao.SIGMA * np.eye(Pn.shape[0]) + ref.rho * Gn.T @ Gn
        assert_matches(sol, ref, b, "c3", tol=max(TOL, 1e-13 * np.linalg.cond(K)), P=Pn, G=Gn)
        checked += 1
        if checked == count:
            break
    assert checked == count


def test_assembled_c3(gpu_api, torch_gpu):
    """4 096 assembled C3 QPs: every solved one meets OSQP's bounds recomputed from P, q, G, h; 16 sampled
    ones are the restatement's."""
    torch = torch_gpu
    from mpcasm import engine

    B = 4096
    form, asm, given = c3_batch(gpu_api, B)
    P, q, G, h = (t.clone() for t in asm.assemble(given))
    sol = engine.solve_qp_wide(P, q, G, h)
    solved = sol.status == rs.SOLVED
    assert int(solved.sum()) > 0
    x, y, z = sol.x, sol.y, sol.z
    inf = lambda t: t.abs().amax(dim=1)
    Gx = torch.einsum("brc,bc->br", G, x)
    Px = torch.einsum("bij,bj->bi", P, x)
    Gty = torch.einsum("brc,br->bc", G, y)
    rp, rd = inf(Gx - z), inf(Px + q + Gty)
    tp = 1e-3 + 1e-3 * torch.maximum(inf(Gx), inf(z))
    td = 1e-3 + 1e-3 * torch.maximum(torch.maximum(inf(Px), inf(Gty)), inf(q))
    assert bool((rp <= tp * (1 + 1e-9))[solved].all()) and bool((rd <= td * (1 + 1e-9))[solved].all())
    assert torch.allclose(sol.res[solved, 0], rp[solved], rtol=1e-9, atol=1e-15)
    sampled_matches(sol, P, q, G, h, B)


@pytest.mark.parametrize("home", ["lds", "global"])
def test_kinv_on_and_off_chip(gpu_api, torch_gpu, monkeypatch, home):
    """K^-1 forced into LDS and into d_kinv: the 96 x 196 mixed batch and 16 sampled C3 instances each the
    restatement's."""
    torch = torch_gpu
    from mpcasm import engine

    monkeypatch.setenv("MPCASM_QP_WIDE_KINV", home)
    assert engine.qp_solve_wide_info(96, 196)[1] == (home == "lds")
    check_mixed(torch, 96, 196)
    B = 512
    form, asm, given = c3_batch(gpu_api, B, seed=41)
    P, q, G, h = (t.clone() for t in asm.assemble(given))
    kinv = torch.full((B, 96, 96), float("nan"), dtype=torch.float64, device="cuda")
    sol = engine.solve_qp_wide(P, q, G, h, kinv=kinv)
    sampled_matches(sol, P, q, G, h, B)
    # K^-1 left behind is the inverse for the final rho, in either home
    Pn, Gn = host(P[0], G[0])
    r = float(sol.rho[0])
    Kref = np.linalg.inv(Pn + engine.OSQP_SIGMA * np.eye(96) + r * Gn.T @ Gn)
    assert_close(kinv[0].cpu().numpy(), Kref, 1e-9, "K^-1 for the final rho")
    # (and within the forward bound no u kappa2 |X*|_2 of the long-double inverse, whatever rho came out)
    sr.assert_inverse(kinv[0].cpu().numpy(), Pn, Gn, r, engine.OSQP_SIGMA, "K^-1 for the final rho")


@pytest.mark.parametrize("home", [None, "global"])
def test_the_next_tick_reuses_the_inverse(gpu_api, torch_gpu, monkeypatch, home):
    """The next tick on the same P, G with kinv and rho passed back is bit-identical to a fresh factorisation
    from the same rho; two identical calls are bit-identical."""
    torch = torch_gpu
    from mpcasm import engine

    if home is not None:
        monkeypatch.setenv("MPCASM_QP_WIDE_KINV", home)
    B = 256
    form, asm, given = c3_batch(gpu_api, B, seed=5)
    P, q, G, h = (t.clone() for t in asm.assemble(given))
    kinv = torch.empty((B, 96, 96), dtype=torch.float64, device="cuda")
    rho = torch.full((B,), engine.OSQP_RHO, dtype=torch.float64, device="cuda")
    first = engine.solve_qp_wide(P, q, G, h, rho=rho, kinv=kinv)
    assert bool((rho != engine.OSQP_RHO).any())
    P2, q2, G2, h2 = asm.assemble(given + np.random.default_rng(6).normal(0, 0.01, given.shape))
    assert torch.equal(P2, P) and torch.equal(G2, G)
    runs = []
    for valid in (True, False, True):
        start = [t.clone() for t in (first.x, first.y, first.z)]
        k = kinv.clone()
        runs.append(engine.solve_qp_wide(P2, q2, G2, h2, *start, rho=rho.clone(), kinv=k, kinv_valid=valid) + (k,))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    assert bool((runs[0][3] == rs.SOLVED).any())


def test_a_c3_tick_captured_in_one_graph(gpu_api, torch_gpu):
    """assemble + solve_qp_wide of C3 in one graph: replays on new `given` equal the eager calls bit for bit;
    sixteen calls read nothing back."""
    torch = torch_gpu
    from mpcasm import engine

    B = 256
    form, asm, given = c3_batch(gpu_api, B, seed=9)
    gbuf = torch.as_tensor(given, device="cuda")
    engine.solve_qp_wide(*asm.assemble(gbuf))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = engine.solve_qp_wide(*asm.assemble(gbuf))
    rng = np.random.default_rng(10)
    for _ in range(2):
        new = given + rng.normal(0, 0.01, given.shape)
        gbuf.copy_(torch.as_tensor(new, device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured]
        eager = engine.solve_qp_wide(*asm.assemble(torch.as_tensor(new, device="cuda")))
        for a, b in zip(replayed, eager):
            assert torch.equal(a, b)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(16):
            engine.solve_qp_wide(*asm.assemble(gbuf))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_what_the_wide_solve_refuses(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import capi, engine

    rng = np.random.default_rng(2)
    P, q, G, h = (np.stack(a) for a in zip(*[rs.random_qp(rng, 200, 404) for _ in range(2)]))
    dP, dq, dG, dh = to_dev(torch, P, q, G, h)
    x = torch.full((2, 200), 7.0, dtype=torch.float64, device="cuda")
    y, z = (torch.full((2, 404), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    for kw in (dict(eps_abs=-1e-3), dict(eps_rel=float("inf")), dict(eps_prim_inf=float("nan")),
               dict(eps_dual_inf=-1.0), dict(max_iter=-1), dict(check_every=0), dict(adaptive_rho_interval=-25),
               dict(adaptive_rho_interval=30), dict(sigma=0.0), dict(alpha=2.0), dict(alpha=0.0)):
        with pytest.raises(capi.MpcasmError) as err:
            engine.solve_qp_wide(dP, dq, dG, dh, x, y, z, **kw)
        assert err.value.status == -1, kw
    for bad in (torch.empty((2, 200, 199), dtype=torch.float64, device="cuda"),
                torch.empty((2, 200, 200), dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError):
            engine.solve_qp_wide(dP, dq, dG, dh, x, y, z, kinv=bad)
    # past the limit: 513 unknowns, and 2 710 limits at 512
    for no, nc in ((513, 4), (512, 2710)):
        with pytest.raises(capi.MpcasmError) as err:
            engine.qp_solve_wide_info(no, nc)
        assert err.value.status == capi.ERR_LIMIT
        big = [torch.zeros(s, dtype=torch.float64, device="cuda") for s in
               ((1, no, no), (1, no), (1, nc, no), (1, nc))]
        with pytest.raises(capi.MpcasmError) as err:
            engine.solve_qp_wide(*big)
        assert err.value.status == capi.ERR_LIMIT
    # K^-1 off chip and no workspace: refused at the C entry
    rc = capi.load().mpcasm_qp_solve_wide(200, 404, dP.data_ptr(), dq.data_ptr(), dG.data_ptr(), dh.data_ptr(),
                                          x.data_ptr(), y.data_ptr(), z.data_ptr(), 1,
                                          torch.ones(2, dtype=torch.float64, device="cuda").data_ptr(),
                                          1e-6, 1.6, 1e-3, 1e-3, 1e-4, 1e-4, 100, 25, 100,
                                          torch.empty(2, dtype=torch.int32, device="cuda").data_ptr(),
                                          torch.empty(2, dtype=torch.int32, device="cuda").data_ptr(),
                                          None, 2, None, 0, None)
    assert rc == -1
    torch.cuda.synchronize()
    # nothing launched: the warm start is as it was
    assert bool((x == 7.0).all()) and bool((y == 7.0).all()) and bool((z == 7.0).all())
    # rho <= 0: that instance alone not convex
    sol = engine.solve_qp_wide(dP, dq, dG, dh, rho=torch.tensor([1.0, 0.0], dtype=torch.float64, device="cuda"))
    assert sol.status.tolist() == [rs.SOLVED, rs.NON_CVX] and sol.iters.tolist()[1] == 0
    assert bool(sol.x[1].isnan().all())
