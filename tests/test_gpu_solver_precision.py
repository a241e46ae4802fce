"""The three solver kernels -- mpcasm_admm, mpcasm_qp_solve (csrc/admm.hip) and mpcasm_qp_solve_wide
(csrc/admm_wide.hip, K^-1 on chip and in d_kinv) -- against tests/solver_reference.py: the explicit inverse,
one step, 65 steps and the residuals each against the same computation in long double, on QPs whose K has a
prescribed condition (1e1, 1e5, 1e9) at rho = 1e-6, 0.1 and 1e6, at the shapes where the kernels take another
path.  A-priori bounds where rounding-error analysis gives one (the inverse, one step, the residuals), else
the plain fp64 restatement as the yardstick: the kernel may err 8 times as much as a correct implementation
in another order of summation, about three times the spread seen between two such orderings (0.35 to 2.6).
tests/test_solver_reference_cpu.py holds the reference and the bounds themselves to account.

Every test prints one report line ``solver-precision: ...`` with the worst of its instances (pytest -s);
profiles/solver_precision.txt keeps those of one full run."""
import numpy as np
import pytest

import solver_reference as sr
from helpers import LD, U64
from test_gpu_qp_solve_wide import check_mixed

pytestmark = pytest.mark.gpu
ZERO = dict(eps_abs=0, eps_rel=0, eps_prim_inf=0, eps_dual_inf=0, adaptive_rho_interval=0)
YARD = 8.0
CASE_ENTRIES = [(c, e) for c in sr.cases() for e in sr.entries(c[0], c[1])]
IDS = ["%s-%s" % (sr.case_id(c), e) for c, e in CASE_ENTRIES]


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def report(what, c, entry, text):
    print("solver-precision: %-7s %-24s %-11s %s" % (what, c if isinstance(c, str) else sr.case_id(c), entry, text))


def choose(monkeypatch, entry, no, nc):
    """The entry's home for K^-1 set and confirmed; the shape confirmed to fit where the entry keeps it."""
    from mpcasm import engine

    if entry in ("admm", "solve"):
        assert engine.qp_solve_lds_bytes(no, nc) == 8 * sr.lds_doubles(no, nc) <= sr.LDS_LIMIT
        return
    home = entry.split("-")[1]
    # what the kernel does by default, before the override: K^-1 on chip up to 129 unknowns, not beyond
    monkeypatch.delenv("MPCASM_QP_WIDE_KINV", raising=False)
    assert engine.qp_solve_wide_info(no, nc)[1] == (8 * sr.wide_doubles(no, nc, True) <= sr.LDS_LIMIT)
    monkeypatch.setenv("MPCASM_QP_WIDE_KINV", home)
    lds, on = engine.qp_solve_wide_info(no, nc)
    assert on == (home == "lds") and lds == 8 * sr.wide_doubles(no, nc, on)


def test_where_the_inverse_lives_at_the_edges(gpu_api, monkeypatch):
    from mpcasm import engine

    monkeypatch.delenv("MPCASM_QP_WIDE_KINV", raising=False)
    assert engine.qp_solve_wide_info(129, 4)[1] is True
    assert engine.qp_solve_wide_info(257, 3)[1] is False and engine.qp_solve_wide_info(512, 8)[1] is False
    assert engine.qp_solve_lds_bytes(96, 1) <= sr.LDS_LIMIT


def run(torch, entry, qp, rho, iters, start=None, kinv=None):
    """``iters`` plain iterations of ``entry`` on the stacked QPs ``qp`` (numpy), cold or from ``start``
    (device tensors, updated in place): ``x, y, z, res`` on the device.  On a cold start every result buffer
    holds NaN before the call."""
    from mpcasm import capi, engine

    P, q, G, h = (torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in qp)
    B, no, nc = P.shape[0], P.shape[1], G.shape[1]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    if entry == "admm":
        if start is not None:
            return engine.admm(P, q, G, h, *start, iters=iters, rho=rho, sigma=sr.SIGMA, alpha=sr.ALPHA, kinv=kinv)
        x, y, z, res = nan(B, no), nan(B, nc), nan(B, nc), nan(B, 2)
        rc = capi.load().mpcasm_admm(no, nc, P.data_ptr(), q.data_ptr(), G.data_ptr(), h.data_ptr(), x.data_ptr(),
                                     y.data_ptr(), z.data_ptr(), res.data_ptr(), float(rho), sr.SIGMA, sr.ALPHA,
                                     int(iters), 0, B, kinv.data_ptr() if kinv is not None else None, 0, None)
        capi.check(rc, "mpcasm_admm")
        return x, y, z, res
    solve = engine.solve_qp if entry == "solve" else engine.solve_qp_wide
    # (one check, at the last iteration: with all eps 0 an instance still stops at a check whose two norms
    # round to exactly 0 -- one unknown does that, after 25 iterations)
    kw = dict(rho=rho, max_iter=iters, check_every=max(iters, 1), sigma=sr.SIGMA, alpha=sr.ALPHA, kinv=kinv, **ZERO)
    if start is not None:
        sol = solve(P, q, G, h, *start, **kw)
    else:
        ints = lambda: torch.full((B,), -99, dtype=torch.int32, device="cuda")
        sol = solve(P, q, G, h, out=(nan(B, no), nan(B, nc), nan(B, nc), ints(), ints(), nan(B, 2)), **kw)
    assert sol.iters.tolist() == [iters] * B
    assert set(sol.status.tolist()) <= {engine.QP_MAX_ITER, engine.QP_SOLVED}      # (SOLVED: both norms came out 0)
    assert sol.rho.tolist() == [rho] * B
    return sol.x, sol.y, sol.z, sol.res


def host(*tensors):
    out = [t.cpu().numpy() for t in tensors]
    for a in out:
        assert np.isfinite(a).all(), "a result holds NaN or inf"
    return out


def stacked(cs):
    return cs.P, cs.q, cs.G, cs.h


@pytest.mark.parametrize("c,entry", CASE_ENTRIES, ids=IDS)
def test_the_inverse(gpu_api, torch_gpu, monkeypatch, c, entry):
    """(a) K^-1 as the kernel leaves it after no iteration at all: exactly symmetric, within the forward bound
    of X*, and within 8 times the restatement's error."""
    torch = torch_gpu
    cs = sr.case(*c)
    choose(monkeypatch, entry, cs.no, cs.nc)
    kinv = torch.full((sr.INSTANCES, cs.no, cs.no), float("nan"), dtype=torch.float64, device="cuda")
    x, y, z, res = run(torch, entry, stacked(cs), cs.rho, 0, kinv=kinv)
    assert torch.equal(kinv, kinv.transpose(1, 2))
    (X,) = host(kinv)
    assert not np.any(host(x)[0])                       # (no iteration: the cold start comes back)
    fails, units, share, ratio = [], 0.0, 0.0, 0.0
    for b in range(sr.INSTANCES):
        err, bound = sr.err_inf(X[b], cs.X[b]), sr.inverse_bound(cs.no, cs.kappa[b], cs.X[b])
        yard = max(sr.err_inf(cs.X64[b], cs.X[b]), U64 * float(np.abs(cs.X[b]).max()))
        units = max(units, err / (U64 * cs.kappa[b] * sr.norm2(cs.X[b])))
        share, ratio = max(share, err / bound), max(ratio, err / yard)
        if err > bound:
            fails.append("instance %d: |X - X*| %.3e > bound %.3e" % (b, err, bound))
        if err > YARD * yard:
            fails.append("instance %d: |X - X*| %.3e > %g x the restatement's %.3e" % (b, err, YARD, yard))
    report("inverse", c, entry, "kappa2 %.1e  err %.3f u kappa2 |X*|_2 = %.4f of the bound, %.2f x the restatement's"
           % (max(cs.kappa), units, share, ratio))
    assert not fails, fails


@pytest.mark.parametrize("c,entry", CASE_ENTRIES, ids=IDS)
def test_one_step_from_a_warm_start(gpu_api, torch_gpu, monkeypatch, c, entry):
    """(b) one iteration from random x, y >= 0, z <= h with active and inactive rows, against the long-double
    step that applies X*:  |dx| <= 2 e,  |dz| <= 2 |G|_2 e + 8 u Mz,  |dy| <= rho (2 |G|_2 e + 8 u Mz)."""
    torch = torch_gpu
    cs = sr.case(*c)
    choose(monkeypatch, entry, cs.no, cs.nc)
    start = [torch.as_tensor(a.copy(), device="cuda") for a in (cs.x0, cs.y0, cs.z0)]
    x, y, z = host(*run(torch, entry, stacked(cs), cs.rho, 1, start=start)[:3])
    fails, share = [], [0.0, 0.0, 0.0]
    for b in range(sr.INSTANCES):
        xs, ys, zs, rs, zrs = cs.ref_step(b)
        bounds = sr.step_bounds(cs.G[b], cs.h[b], cs.y0[b], cs.rho, cs.kappa[b], cs.X[b], rs, zrs)
        errs = (sr.err_inf(x[b], xs), sr.err_inf(y[b], ys), sr.err_inf(z[b], zs))
        share = [max(w, sr.ratio(e, bd)) for w, e, bd in zip(share, errs, bounds)]
        fails += ["instance %d: |d%s| %.3e > %.3e" % (b, n, e, bd) for n, e, bd in zip("xyz", errs, bounds) if e > bd]
    report("step", c, entry, "kappa2 %.1e  of the bounds: |dx| %.2e |dy| %.2e |dz| %.2e" % (max(cs.kappa), *share))
    assert not fails, fails


def against_the_yardstick(cs, b, stage, got, what):
    """(c) for one instance after ``stage`` (0: 40 steps, 1: 25 more): failures, the worst ratio to the
    restatement's error and ``|dx| / |x*|``."""
    ref, rest = cs.iterates(b, LD)[stage], cs.iterates(b, np.float64)[stage]
    fails, worst = [], 0.0
    for name, g, r, r64 in zip("xyz", got, ref, rest):
        floor = U64 * float(np.abs(r).max(initial=LD(0)))
        err, yard = sr.err_inf(g, r), max(sr.err_inf(r64, r), floor)
        worst = max(worst, sr.ratio(err, yard))
        if err > YARD * yard:
            fails.append("instance %d, %s: %s off by %.3e > %g x the restatement's %.3e" % (b, what, name, err, YARD, yard))
    return fails, worst, sr.ratio(sr.err_inf(got[0], ref[0]), float(np.abs(ref[0]).max()))


def res_failures(qp, x, y, z, res, b, what):
    """(d) the kernel's res against the long-double norms of the very iterate it returned: failures and the
    larger share of a bound."""
    no, nc = qp[0].shape[0], qp[2].shape[0]
    rp, rd, Mp, Md = sr.residuals(*qp[:3], x, y, z)
    bp, bd = sr.res_bounds(no, nc, Mp, Md)
    ep, ed = abs(float(LD(res[0]) - rp)), abs(float(LD(res[1]) - rd))
    fails = ["instance %d, %s: res_%s %.3e off by %.3e > %.3e" % (b, what, n, r, e, bd_)
             for n, r, e, bd_ in (("p", res[0], ep, bp), ("d", res[1], ed, bd)) if e > bd_]
    return fails, max(sr.ratio(ep, bp), sr.ratio(ed, bd))


@pytest.mark.parametrize("c,entry", CASE_ENTRIES, ids=IDS)
def test_forty_steps_and_twenty_five_more(gpu_api, torch_gpu, monkeypatch, c, entry):
    """(c) 40 steps from the cold start, then 25 from the kernel's own state: each of x, y, z within 8 times
    the restatement's error against the long-double iterate; (d) res of either against long double."""
    torch = torch_gpu
    cs = sr.case(*c)
    choose(monkeypatch, entry, cs.no, cs.nc)
    fails, text = [], []
    state = run(torch, entry, stacked(cs), cs.rho, 40)
    for stage, what in enumerate(("40", "65")):
        if stage:
            state = run(torch, entry, stacked(cs), cs.rho, 25, start=list(state[:3]))
        x, y, z, res = host(*state)
        yard, rel, units, share = 0.0, 0.0, 0.0, 0.0
        for b in range(sr.INSTANCES):
            f, w, r = against_the_yardstick(cs, b, stage, (x[b], y[b], z[b]), what)
            g, s = res_failures(cs.qp(b), x[b], y[b], z[b], res[b], b, what)
            fails += f + g
            yard, rel, units, share = max(yard, w), max(rel, r), max(units, r / (U64 * cs.kappa[b])), max(share, s)
        text.append("after %s: %.2f x the restatement's, |dx|/|x*| %.1e = %.3f u kappa2, res at %.4f of its bound"
                    % (what, yard, rel, units, share))
    report("iterate", c, entry, "kappa2 %.1e  " % max(cs.kappa) + "; ".join(text))
    assert not fails, fails


@pytest.mark.parametrize("c,entry", [ce for ce in CASE_ENTRIES if ce[0][2] == sr.TARGETS[0] and ce[0][:2] not in sr.SLOW],
                         ids=[i for i, ce in zip(IDS, CASE_ENTRIES) if ce[0][2] == sr.TARGETS[0] and ce[0][:2] not in sr.SLOW])
def test_the_residuals_at_a_converged_iterate(gpu_api, torch_gpu, monkeypatch, c, entry):
    """(d) where res is a difference of nearly equal sums: warm runs on the well-conditioned cases until
    res < 1e-10, then res against the long-double norms of the returned iterate."""
    torch = torch_gpu
    cs = sr.case(*c)
    choose(monkeypatch, entry, cs.no, cs.nc)
    state = run(torch, entry, stacked(cs), cs.rho, sr.CONVERGE_ITERS)
    for _ in range(sr.CONVERGE_ROUNDS - 1):
        if float(state[3].max()) < sr.CONVERGED:
            break
        state = run(torch, entry, stacked(cs), cs.rho, sr.CONVERGE_ITERS, start=list(state[:3]))
    x, y, z, res = host(*state)
    assert res.max() < sr.CONVERGED, res
    fails, share = [], 0.0
    for b in range(sr.INSTANCES):
        f, s = res_failures(cs.qp(b), x[b], y[b], z[b], res[b], b, "converged")
        fails, share = fails + f, max(share, s)
    report("res", c, entry, "converged: res up to %.1e %.1e, off by %.4f of its bound at the most"
           % (res[:, 0].max(), res[:, 1].max(), share))
    assert not fails, fails


@pytest.mark.parametrize("no,nc,entry", [(64, 2, "solve"), (64, 2, "wide-lds"), (64, 2, "wide-global"),
                                         (129, 4, "wide-lds"), (129, 4, "wide-global")])
def test_honest_verdicts_past_the_reach_of_the_method(gpu_api, torch_gpu, monkeypatch, no, nc, entry):
    """(e) P of rank no - 3 at rho = 1e6, kappa2 >= 1e13: the explicit inverse keeps few digits or none.  The
    real solve, OSQP's defaults, 400 iterations: whatever the status, an instance called SOLVED meets OSQP's two
    inequalities recomputed in long double from P, q, G, h and the returned iterate (slack: (d)'s, on the norm
    and on its scale), and none holds a NaN unless it is called NON_CVX."""
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h, kappas = sr.deficient_case(no, nc)
    assert min(kappas) >= 1e13, kappas
    choose(monkeypatch, entry, no, nc)
    solve = engine.solve_qp if entry == "solve" else engine.solve_qp_wide
    sol = solve(*(torch.as_tensor(a, device="cuda") for a in (P, q, G, h)), rho=1e6, max_iter=400)
    status = sol.status.tolist()
    x, y, z, res = (t.cpu().numpy() for t in (sol.x, sol.y, sol.z, sol.res))
    worst = [0.0, 0.0]
    for b in range(sr.INSTANCES):
        if status[b] == engine.QP_NON_CVX:
            continue
        assert all(np.isfinite(a[b]).all() for a in (x, y, z, res)), "instance %d (status %d) holds a NaN" % (b, status[b])
        if status[b] != engine.QP_SOLVED:
            continue
        rp, rd, Mp, Md = sr.residuals(P[b], q[b], G[b], x[b], y[b], z[b])
        bp, bd = sr.res_bounds(no, nc, Mp, Md)
        c = lambda a: np.asarray(a, dtype=np.float64).astype(LD)
        top = lambda v: float(np.abs(v).max(initial=LD(0)))
        sp = max(top(c(G[b]) @ c(x[b])), top(c(z[b])))
        sd = max(top(c(P[b]) @ c(x[b])), top(c(G[b]).T @ c(y[b])), top(c(q[b])))
        worst = [max(worst[0], float(rp) / (1e-3 + 1e-3 * sp)), max(worst[1], float(rd) / (1e-3 + 1e-3 * sd))]
        assert float(rp) <= 1e-3 + 1e-3 * sp + (1 + 1e-3) * bp, "instance %d called SOLVED: r_p* %.3e" % (b, float(rp))
        assert float(rd) <= 1e-3 + 1e-3 * sd + (1 + 1e-3) * bd, "instance %d called SOLVED: r_d* %.3e" % (b, float(rd))
    report("verdict", "%dx%d-deficient" % (no, nc), entry,
           "kappa2 %.1e  status %s iters %s rho %s; the SOLVED ones at r_p* %.2e, r_d* %.2e of their eps"
           % (min(kappas), status, sol.iters.tolist(), ["%.3g" % r for r in sol.rho.tolist()], *worst))


@pytest.mark.parametrize("no,nc", [(128, 9), (129, 4), (256, 17), (257, 3)])
def test_the_restatement_checks_at_the_new_wide_edges(gpu_api, torch_gpu, no, nc):
    """(f) tests/test_gpu_qp_solve_wide.py's mixed batch at the sizes where the columns per lane change (128 |
    129, 256 | 257) and where K^-1 leaves the chip (129 | 130).  (257 x 3 with seed 5: the default seed's
    primal-infeasible instance picks its new rho from a dual residual 2e-10 of rounding size -- the restatement's
    own rho moves by 7e-4 when the unknowns are merely permuted; with seed 5 it moves by 6e-11.)"""
    check_mixed(torch_gpu, no, nc, seed=5 if (no, nc) == (257, 3) else None)
