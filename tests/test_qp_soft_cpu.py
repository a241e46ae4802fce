"""CPU: soft limits in the QP solvers -- the restatement the device tests hold the kernels to
(tests/soft_restatement.py) against the hard restatement and against the slack QP, the verdicts with and without
the masked certificate, ``plan.soft_rows``, the two host-only info entries and the refusals of the C entries that
need no device."""
import ctypes

import numpy as np
import pytest

import osqp_restatement as rs
import soft_restatement as ss
from mpcasm import capi, engine, problems
from mpcasm.plan import compile_plan, soft_rows

MARGIN = 1e-6
LIMIT = 156 * 1024
SHAPES = [(5, 9), (36, 76)]


@pytest.mark.parametrize("no,nc", SHAPES)
@pytest.mark.parametrize("make", [rs.random_qp, rs.primal_infeasible_qp, rs.dual_infeasible_qp])
def test_all_rows_hard_is_the_hard_restatement_exactly(make, no, nc):
    qp = make(np.random.default_rng(no * 100 + nc), no, nc)
    hard = rs.solve(*qp)
    soft = ss.solve(*qp, np.inf, 0.0)
    assert (soft.status, soft.iters, soft.rho, soft.margin, soft.rho_changes, soft.res) == \
        (hard.status, hard.iters, hard.rho, hard.margin, hard.rho_changes, hard.res)
    for a, b in zip(soft[:3], hard[:3]):
        assert np.array_equal(a, b)
    assert hard.status == {rs.random_qp: rs.SOLVED, rs.primal_infeasible_qp: rs.PRIMAL_INFEASIBLE,
                           rs.dual_infeasible_qp: rs.DUAL_INFEASIBLE}[make]


@pytest.mark.parametrize("no,nc", SHAPES)
def test_soft_rows_against_the_slack_qp(no, nc):
    """A QP whose limits cannot all hold (the contradicting pair), every row soft but one: x, and y on G's rows,
    are the slack QP's as the hard restatement solves it."""
    rng = np.random.default_rng(no + nc)
    P, q, G, h = rs.primal_infeasible_qp(rng, no, nc)
    lin, quad = rng.uniform(0.5, 2.0, nc), rng.uniform(0.0, 1.0, nc)
    quad[::3] = 0.0
    lin[nc - 1] = np.inf                       # (one row kept hard)
    kw = dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=200000)
    soft = ss.solve(P, q, G, h, lin, quad, **kw)
    slack = rs.solve(*ss.slack_qp(P, q, G, h, lin, quad), **kw)
    assert soft.status == rs.SOLVED and slack.status == rs.SOLVED
    assert (G @ soft.x - h).max() > 0.5        # (a soft row is violated: the penalty is at work)
    assert np.abs(soft.x - slack.x[:no]).max() <= 1e-6 * np.abs(slack.x[:no]).max()
    assert np.abs(soft.y - slack.y[:nc]).max() <= 1e-6 * np.abs(slack.y[:nc]).max()


@pytest.mark.parametrize("no,nc", [(5, 9), (36, 76), (65, 70)])
def test_the_verdicts_with_and_without_the_mask(no, nc):
    P, q, G, h = rs.primal_infeasible_qp(np.random.default_rng(7 * no + nc), no, nc)
    hard = rs.solve(P, q, G, h)
    assert hard.status == rs.PRIMAL_INFEASIBLE and hard.margin > MARGIN
    masked = ss.solve(P, q, G, h, 1e4, 0.0)
    assert masked.status == rs.SOLVED and masked.margin > MARGIN
    # without the mask y's climb towards lin reads as a certificate: the wrong verdict, at the hard solve's check
    unmasked = ss.solve(P, q, G, h, 1e4, 0.0, mask=False)
    assert unmasked.status == rs.PRIMAL_INFEASIBLE and unmasked.iters == hard.iters
    # the contradicting pair kept hard among soft rows: still a certificate, on the hard rows alone
    lin = np.full(nc, 1e4)
    lin[:2] = np.inf
    pair = ss.solve(P, q, G, h, lin, 0.0)
    assert pair.status == rs.PRIMAL_INFEASIBLE and pair.margin > MARGIN


def test_a_penalty_no_multiplier_reaches_changes_nothing():
    P, q, G, h = rs.random_qp(np.random.default_rng(3), 36, 76)
    hard = rs.solve(P, q, G, h)
    soft = ss.solve(P, q, G, h, 10.0 * max(hard.y.max(), 1.0), 0.0)
    assert hard.status == rs.SOLVED and soft.iters == hard.iters
    assert np.allclose(soft.x, hard.x, rtol=0, atol=1e-12) and np.allclose(soft.y, hard.y, rtol=0, atol=1e-12)


@pytest.mark.parametrize("lin,quad", [(-1.0, 0.0), (np.nan, 0.0), (1.0, np.inf), (1.0, -1.0), (1.0, np.nan)])
def test_bad_penalties_in_the_restatement(lin, quad):
    P, q, G, h = rs.random_qp(np.random.default_rng(5), 5, 9)
    lv, qv = np.full(9, 1.0), np.zeros(9)
    lv[4], qv[4] = lin, quad
    sol = ss.solve(P, q, G, h, lv, qv)
    assert sol.status == rs.NON_CVX and sol.iters == 0 and np.isnan(sol.x).all()


# ---- plan.soft_rows ----------------------------------------------------------------------------------------------
def plans(cpu_api):
    return [compile_plan(problems.biped(cpu_api, problems.BipedConfig(step_samples=8))),
            compile_plan(problems.lipm_ltv(cpu_api, N=12), ltv=["LIP"])]


def test_soft_rows_rows_and_defaults(cpu_api):
    for plan in plans(cpu_api):
        assert len(plan.limit_rows) >= 2
        lin, quad = soft_rows(plan, {})
        assert lin.shape == quad.shape == (plan.nc,) and lin.dtype == quad.dtype == np.float64
        assert np.isinf(lin).all() and (lin > 0).all() and (quad == 0).all()
        last = len(plan.limit_rows) - 1
        r0, n0 = plan.limit_rows[0]
        r1, n1 = plan.limit_rows[last]
        per_row = np.arange(1.0, n1 + 1.0)
        lin, quad = soft_rows(plan, {0: (1e3, 0.5), last: (per_row, np.zeros(n1))})
        assert (lin[r0:r0 + n0] == 1e3).all() and (quad[r0:r0 + n0] == 0.5).all()
        assert np.array_equal(lin[r1:r1 + n1], per_row) and (quad[r1:r1 + n1] == 0).all()
        named = np.zeros(plan.nc, dtype=bool)
        named[r0:r0 + n0] = named[r1:r1 + n1] = True
        assert np.isinf(lin[~named]).all() and (quad[~named] == 0).all()
        assert soft_rows(plan, {0: (np.inf, 0.0)})[0][r0] == np.inf      # (a rule may name a row hard)


def test_soft_rows_refusals(cpu_api):
    for plan in plans(cpu_api):
        n0 = plan.limit_rows[0][1]
        for rules in ({len(plan.limit_rows): (1.0, 0.0)}, {-1: (1.0, 0.0)}, {"0": (1.0, 0.0)}, {0: 1.0},
                      {0: (np.ones(n0 + 1), 0.0)}, {0: (1.0, np.zeros(n0 + 1))}, {0: (np.ones((n0, 1)), 0.0)},
                      {0: (-1.0, 0.0)}, {0: (np.nan, 0.0)}, {0: (1.0, -1.0)}, {0: (1.0, np.nan)},
                      {0: (1.0, np.inf)}):
            with pytest.raises(ValueError):
                soft_rows(plan, rules)


# ---- the host-only entries ------------------------------------------------------------------------------------------
def narrow_doubles(no, nc, soft):
    m = max(nc, no)
    total = (no + m) * (no | 1) + 8 * no + 4 * nc + 4 * m + (2 * nc if soft else 0)
    return total + (total & 1)


def wide_doubles(no, nc, on_chip, soft):
    n = (5 if soft else 3) * nc + 23 * no + 64 + (no * (no | 1) if on_chip else 0)
    return n + (n & 1)


@pytest.mark.parametrize("no,nc", [(1, 1), (5, 9), (36, 76), (12, 257), (65, 70), (7, 0)])
def test_the_narrow_entrys_lds(no, nc):
    assert engine.qp_solve_soft_lds_bytes(no, nc) == 8 * narrow_doubles(no, nc, True)
    assert engine.qp_solve_lds_bytes(no, nc) == 8 * narrow_doubles(no, nc, False)


def test_the_narrow_entrys_limit_at_the_edge():
    no = 36
    nc = max(n for n in range(no, 1000) if 8 * narrow_doubles(no, n, True) <= LIMIT)
    assert engine.qp_solve_soft_lds_bytes(no, nc) <= LIMIT
    with pytest.raises(capi.MpcasmError) as err:
        engine.qp_solve_soft_lds_bytes(no, nc + 1)
    assert err.value.status == capi.ERR_LIMIT
    assert 8 * narrow_doubles(no, nc + 1, False) <= LIMIT      # (the hard entry still takes it)
    engine.qp_solve_lds_bytes(no, nc + 1)


@pytest.mark.parametrize("no,nc", [(36, 76), (96, 196), (65, 70), (129, 140), (257, 260), (200, 404), (384, 1536),
                                   (512, 1625), (7, 0)])
def test_the_wide_entrys_info(monkeypatch, no, nc):
    monkeypatch.delenv("MPCASM_QP_WIDE_KINV", raising=False)
    lds, on = engine.qp_solve_wide_soft_info(no, nc)
    assert on == (no <= 512 and 8 * wide_doubles(no, nc, True, True) <= LIMIT)
    assert lds == 8 * wide_doubles(no, nc, on, True) <= LIMIT
    monkeypatch.setenv("MPCASM_QP_WIDE_KINV", "global")
    assert engine.qp_solve_wide_soft_info(no, nc) == (8 * wide_doubles(no, nc, False, True), False)


@pytest.mark.parametrize("no,nc", [(513, 1), (512, 1626), (1, 3977)])
def test_the_wide_entrys_limit_just_past_the_edge(monkeypatch, no, nc):
    monkeypatch.delenv("MPCASM_QP_WIDE_KINV", raising=False)
    assert no > 512 or (8 * wide_doubles(no, nc, False, True) > LIMIT >= 8 * wide_doubles(no, nc - 1, False, True))
    with pytest.raises(capi.MpcasmError) as err:
        engine.qp_solve_wide_soft_info(no, nc)
    assert err.value.status == capi.ERR_LIMIT
    engine.qp_solve_wide_soft_info(no - 1 if no == 513 else no, nc - 1 if no != 513 else nc)


# ---- refusals that need no device ----------------------------------------------------------------------------------
def call(entry, no=4, nc=3, batch=2, stride=3, lin=True, quad=True, max_iter=10):
    """``entry`` on host buffers standing in for device memory: every case here is refused before any device call."""
    buf = lambda n: ctypes.cast((ctypes.c_double * max(n, 1))(), ctypes.c_void_p)
    ints = lambda n: ctypes.cast((ctypes.c_int32 * max(n, 1))(), ctypes.c_void_p)
    P, q, G, h = buf(batch * no * no), buf(batch * no), buf(batch * nc * no), buf(batch * nc)
    x, y, z, rho, res = buf(batch * no), buf(batch * nc), buf(batch * nc), buf(batch), buf(2 * batch)
    keep = [P, q, G, h, x, y, z, rho, res]
    return getattr(capi.load(), entry)(no, nc, P, q, G, h, x, y, z, 0, rho, 1e-6, 1.6, 1e-3, 1e-3, 1e-4, 1e-4,
                                       max_iter, 25, 100, ints(batch), ints(batch), res, batch, None, 0, None,
                                       buf(batch * nc) if lin else None, buf(batch * nc) if quad else None,
                                       stride), keep


@pytest.mark.parametrize("entry", ["mpcasm_qp_solve_soft", "mpcasm_qp_solve_wide_soft"])
def test_what_the_soft_entries_refuse_before_any_device_call(entry, monkeypatch):
    monkeypatch.delenv("MPCASM_QP_WIDE_KINV", raising=False)
    for stride in (1, 2, 4, -3, 6):
        assert call(entry, stride=stride)[0] == capi.ERR_ARG
    assert call(entry, lin=False)[0] == capi.ERR_ARG
    assert call(entry, quad=False)[0] == capi.ERR_ARG
    assert call(entry, max_iter=-1)[0] == capi.ERR_ARG                  # (what the hard twin refuses)
    assert call(entry, no=0)[0] == capi.ERR_ARG
    assert call(entry, batch=0)[0] == capi.OK                           # (nothing to do)
    assert call(entry, batch=0, stride=0)[0] == capi.OK
    assert call(entry, batch=0, stride=2)[0] == capi.ERR_ARG            # (decided before the batch is looked at)
    assert call(entry, nc=0, stride=0, lin=False, quad=False, batch=0)[0] == capi.OK
    # past the entry's size limit: MPCASM_ERR_LIMIT, nothing launched
    if entry == "mpcasm_qp_solve_wide_soft":
        assert call(entry, no=512, nc=1626, stride=1626, batch=0)[0] == capi.ERR_LIMIT
    else:   # (the narrow entries learn it from their launch, which asks before it touches the device)
        assert call(entry, no=36, nc=391, stride=391, batch=1)[0] == capi.ERR_LIMIT
        assert call(entry, no=36, nc=391, stride=0, batch=1)[0] == capi.ERR_LIMIT


def test_polish_with_soft_raises_before_the_device_is_asked_for():
    for solve in (engine.solve_qp, engine.solve_qp_wide):
        with pytest.raises(ValueError, match="polish"):
            solve(None, None, None, None, polish=True, soft=(1.0, 0.0))
