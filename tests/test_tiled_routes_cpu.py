"""CPU: what a plan runs on along the tiled path (csrc/tiled.hip, tiled_choose) as the library itself reports it --
mpcasm_tiled_route, the very function the launch decides with.  Every case of the family in tiled_cases.py is pinned
to its route, the family is held to reach EVERY selectable variant (the scan form's seven instantiations fused and
behind the pre-passes, the shared form's seven TG, both table pre-passes, the Toeplitz and the general form), and the
bound the GPU test applies (helpers.kappa) is shown to leave room for a correct fp64 computation in the fused
set-up's own order of association -- the table and the free response by doubling, plan_emulator.fused_setup -- on the
very kind of inputs that test uses: it stays within HALF of it."""
import ctypes

import numpy as np
import pytest

import plan_emulator
import tiled_cases as tc
from helpers import assert_componentwise, kappa, lti_tracking_problem, precise_reference
from mpcasm import capi, engine, problems
from mpcasm.plan import _H, compile_plan

IDS = [c.shape.name for c in tc.CASES]
FUSED = [c for c in tc.CASES if c.route != tc.LIMIT and c.route.form == tc.SCAN and c.route.fused]


_COMPILED = {}      # case name -> (A, B, form, plan): compiled once, shared by the tests, left unchanged


def _compiled(api, case, seed=11):
    name = case.shape.name
    if name not in _COMPILED:
        rng = np.random.default_rng(seed)
        A, B = tc.plants(rng, 1, case.shape)
        form, plan = tc.compile_case(api, rng, case, (A[0], B[0]))
        _COMPILED[name] = (A[0], B[0], form, plan)
    return (np.random.default_rng(seed + 1),) + _COMPILED[name]


def _route(plan, case, **kw):
    return engine.tiled_route(plan, case.batch, tc.src_stride(plan, case), path=case.path, **kw)


def _pinned(r):
    """What a case pins of a TiledRoute (the LDS figure apart)."""
    return tc.Route(r.form, r.fused, r.kp, r.cb, r.rows_in_lds, r.whole_lines, r.whole_lds, r.tables, r.tg, r.sym, None)


@pytest.mark.parametrize("case", tc.CASES, ids=IDS)
def test_every_case_takes_its_route(cpu_api, case):
    _, _, _, form, plan = _compiled(cpu_api, case)
    shape, it = case.shape, plan.itab
    assert plan.no >= 128 and it[_H["T_OK"]] == 1 and plan.resident["ok"] == 0
    assert (it[_H["T_SCAN"]], it[_H["T_SCAN_NBLK"]], it[_H["T_SCAN_FUSED"]]) == (case.K, case.nblk, case.fused)
    assert it[_H["T_TOEPLITZ"]] == (0 if shape.kind == "shared" else 1)
    if case.route == tc.LIMIT:
        with pytest.raises(capi.MpcasmError) as refusal:
            _route(plan, case)
        assert refusal.value.status == capi.ERR_LIMIT
        return
    r = _route(plan, case)
    assert _pinned(r) == case.route._replace(lds=None), r
    assert r.whole_lds == (r.lds > 64 * 1024) and r.lds <= 156 * 1024
    if case.route.lds is not None:
        assert r.lds == case.route.lds
    if r.form == tc.SCAN:
        # the instantiation is the first of the list that holds the plan's terms and column blocks
        first = next((kp, cb) for kp, cb in tc.SCAN_INSTANTIATIONS if case.K <= kp and case.nblk <= cb)
        assert (r.kp, r.cb) == first
        assert r.whole_lines == (plan.no % 16 == 0 and shape.N % 16 == 0)
        assert r.rows_in_lds == (r.lds + (0 if r.rows_in_lds else 16 * plan.nc) <= 80 * 1024 - 8 * 33)      # (NSTREAM pointers of static LDS)
    else:
        assert (r.kp, r.cb, r.fused, r.rows_in_lds, r.whole_lines) == (0, 0, 0, 0, 0)
        assert (r.lds > 0) == (r.form == tc.TOEPLITZ)
    # one half at a time: the same route (the shared form's TG belongs to P)
    cost, limits = _route(plan, case, want=capi.WANT_COST), _route(plan, case, want=capi.WANT_CONSTRAINTS)
    assert cost == r and limits == r._replace(tg=0)


def test_the_family_reaches_every_selectable_variant(cpu_api):
    reached, tight, tables, facts = set(), set(), set(), {}
    for case in tc.CASES:
        if case.route == tc.LIMIT:
            continue
        _, _, _, form, plan = _compiled(cpu_api, case)
        r = _route(plan, case)
        reached.add(tc.variant_of(r))
        if r.tables:
            tables.add(r.tables)
            reached.add(("tables", r.tables))
        if r.form == tc.SCAN:
            if case.K == r.kp or case.nblk == r.cb:
                tight.add((r.kp, r.cb))
            for key, value in (("fused", r.fused), ("rows_in_lds", r.rows_in_lds), ("whole_lines", r.whole_lines),
                               ("whole_lds", r.whole_lds), ("n > 16", int(case.shape.n > 16)),
                               ("K < n", int(case.K < case.shape.n)),
                               ("other unknowns", int(plan.itab[_H["T_SCAN_NOTHER"]] > 0)),
                               ("rows of G behind the rest", int(plan.itab[_H["T_SCAN_NGREST"]] > 0)),
                               ("chunks", (plan.no + 127) // 128)):
                facts.setdefault(key, set()).add(value)
            # n > 16 on both set-ups, and with the rows of G through the scalar cache on both
            if case.shape.n > 16:
                facts.setdefault("n > 16, fused", set()).add(r.fused)
            if not r.rows_in_lds:
                facts.setdefault("rows not in LDS, fused", set()).add(r.fused)
    assert len(tc.SELECTABLE) == 14 + 7 + 4 + 2 and set(tc.UNREACHABLE) <= tc.SELECTABLE
    missing = tc.SELECTABLE - set(tc.UNREACHABLE) - reached
    assert not missing, "no case reaches %s" % sorted(missing, key=str)
    assert reached <= tc.SELECTABLE, "not in the written list: %s" % sorted(reached - tc.SELECTABLE, key=str)
    assert not reached & set(tc.UNREACHABLE), "reached after all: take it off the list of exceptions"
    # every instantiation at its own limit at least once: K = KP or nblk = CB
    assert tight == set(tc.SCAN_INSTANTIATIONS), sorted(set(tc.SCAN_INSTANTIATIONS) - tight)
    for key in ("fused", "rows_in_lds", "whole_lines", "whole_lds", "n > 16", "K < n", "other unknowns",
                "rows of G behind the rest", "n > 16, fused", "rows not in LDS, fused"):
        assert facts[key] == {0, 1}, key
    assert {1, 2, 3, 4, 5} <= facts["chunks"]          # (5: 576 unknowns, the last chunk half used)


@pytest.mark.parametrize("case", FUSED, ids=[c.shape.name for c in FUSED])
def test_the_bound_has_room_for_the_doubling(cpu_api, case):
    """Not a measurement of the kernel: fp64 arithmetic in the fused set-up's own order (rounds of doubling, the
    n-term sums from t = 0) and the scan form's recurrences, on a plant and a formulation of the GPU test's kind,
    stays within half of kappa(N, n) of long double -- so a kernel beyond kappa is at fault, not the bound."""
    rng, A, B, form, plan = _compiled(cpu_api, case)
    shape = case.shape
    given = rng.normal(0, 0.3, form.given_len)
    mine = plan_emulator.run_scan(plan, given, ab=[(A, B)], fused=True, with_ref=False)
    ref = precise_reference(form, "plant", A, B, given)
    kap, worst = kappa(shape.N, shape.n), 0.0
    for key in "PqGh":
        worst = max(worst, assert_componentwise(mine[key], *ref[key], kap // 2, "%s %s" % (shape.name, key)))
    print("componentwise %-60s worst %8.3g u M   kappa %d" % ("fp64 doubling " + shape.name, worst, kap))


@pytest.mark.parametrize("name", ["fused-12-6-24", "fused-4-4-36", "fused-40-3-44-k8"])
def test_the_doubling_makes_the_recurrences_table(cpu_api, name):
    """plan_emulator.fused_setup against the pre-passes' recurrence X_d = A X_{d-1} (plan_emulator._tiled_streams)
    and d = Mg given through the column tables: the same table, the same d, a few roundings apart -- with a short
    last round (N = 24: 16 + 8; 36: 32 + 4; 44: 32 + 12)."""
    case = tc.BY_NAME[name]
    rng, A, B, form, plan = _compiled(cpu_api, case)
    n, m, N = case.shape.n, case.shape.m, case.shape.N
    given = rng.normal(0, 0.3, form.given_len)
    Tc, x, d = plan_emulator.fused_setup(plan, given, [(A, B)])
    ids = plan.lti[0]["ids"]
    tb = plan_emulator._tiled_streams(plan, [s.array for s in plan.sources], [(A, B)])[ids[0]]
    theirs = tb.reshape(n * m, 2 * N)[:, N:]
    assert not tb.reshape(n * m, 2 * N)[:, :N].any()
    scale = np.abs(theirs)
    assert (np.abs(Tc.reshape(n * m, N) - theirs) <= 64 * 2.0 ** -53 * N * scale).all()      # (free of cancellation)
    step, xs = np.array(given), []
    for _ in range(N):
        step = A @ step
        xs.append(step)
    assert np.allclose(x, np.stack(xs), rtol=1e-12, atol=0)
    ref = plan_emulator.run_tiled(plan, given, ab=[(A, B)])
    assert np.allclose(d, ref["d"], rtol=1e-12, atol=0)


def test_query_checks_its_arguments(cpu_api):
    case = tc.BY_NAME["fused-12-6-24"]
    _, _, _, _, plan = _compiled(cpu_api, case)
    lib = capi.load()
    itab, dtab = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab)
    strides = (ctypes.c_int64 * len(plan.sources))(*tc.src_stride(plan, case))
    out = (ctypes.c_int32 * 16)(*([7] * 16))
    args = (itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size)
    assert lib.mpcasm_tiled_route(*args, strides, 19, 3, 0, out) == 0
    assert list(out[:6]) == [tc.SCAN, 1, 12, 6, 1, 0] and list(out[11:]) == [0] * 5
    assert lib.mpcasm_tiled_route(*args, strides, 19, 3, 0, None) == -1
    assert lib.mpcasm_tiled_route(None, itab.size, dtab.ctypes.data, dtab.size, strides, 19, 3, 0, out) == -1
    assert lib.mpcasm_tiled_route(*args, None, 19, 3, 0, out) == -1                 # (the plan has sources)
    assert lib.mpcasm_tiled_route(*args, strides, 0, 3, 0, out) == -1               # (no instance)
    assert lib.mpcasm_tiled_route(*args, strides, 19, 0, 0, out) == -1              # (no half wanted)
    assert lib.mpcasm_tiled_route(*args, strides, 19, 4, 0, out) == -1
    assert lib.mpcasm_tiled_route(*args, strides, 19, 3, 5, out) == -1              # (no such path)
    assert lib.mpcasm_tiled_route(*args, strides, 19, 3, 2, out) == -1              # (path 2: the staged pipeline)
    bad = (ctypes.c_int64 * len(plan.sources))(*([-1] * len(plan.sources)))
    assert lib.mpcasm_tiled_route(*args, bad, 19, 3, 0, out) == -1
    assert lib.mpcasm_tiled_route(itab.ctypes.data, 4, dtab.ctypes.data, dtab.size, strides, 19, 3, 0, out) == -2
    # path -1 is the process-wide option
    assert lib.mpcasm_tiled_route(*args, strides, 19, 3, -1, out) == 0 and out[1] == 1
    # the refusal zeroes out
    over_case = tc.BY_NAME["refused-64-2-64-k4"]
    _, _, _, _, over = _compiled(cpu_api, over_case)
    itab, dtab = np.ascontiguousarray(over.itab), np.ascontiguousarray(over.dtab)
    strides = (ctypes.c_int64 * len(over.sources))(*tc.src_stride(over, over_case))
    out = (ctypes.c_int32 * 16)(*([7] * 16))
    assert lib.mpcasm_tiled_route(itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size, strides, 19, 3, 0,
                                  out) == capi.ERR_LIMIT
    assert list(out) == [0] * 16
    for path in (1, 3, 4):      # (no route without the tables of a system of 64 states and n (m + n) = 4224)
        with pytest.raises(capi.MpcasmError) as refusal:
            engine.tiled_route(over, 19, tc.src_stride(over, over_case), path=path)
        assert refusal.value.status == capi.ERR_LIMIT


def test_plans_of_other_kernels_are_refused(cpu_api):
    """MPCASM_ERR_ARG: a plan the persistent kernel takes first, a narrow plan, a plan compiled with ltv=."""
    rng = np.random.default_rng(3)
    on_chip = compile_plan(problems.random_lti(cpu_api, rng, nx=4, nu=8, N=16), lti=["plant"])
    assert on_chip.no == 128 and on_chip.resident["ok"] == 1
    narrow = compile_plan(lti_tracking_problem(cpu_api, rng, 3, 2, 8)[0])
    ltv = compile_plan(problems.lipm_ltv(cpu_api, N=80), ltv=["LIP"])
    assert ltv.no >= 128
    for plan in (on_chip, narrow, ltv):
        with pytest.raises(capi.MpcasmError) as refusal:
            engine.tiled_route(plan, 19, [1] * len(plan.sources))
        assert refusal.value.status == capi.ERR_ARG


def test_generated_tables_past_64_kb_of_lds_are_refused(cpu_api):
    """MPCASM_ERR_LIMIT before anything is launched: a generated group of 24 states and 24 inputs passes the limits
    of the groups (n (m + n) = 1152 <= 2048, n <= 64), but the per-system pre-pass that would make its horizon
    tables needs (n n + 2 n (m + n) + 16 n m) 8 = 96 768 bytes of dynamic LDS, and that kernel has never run with
    more than 64 KB.  N = 6 is the shortest horizon at which the plan is the tiled path's (144 unknowns)."""
    plan = compile_plan(problems.random_lti(cpu_api, np.random.default_rng(3), nx=24, nu=24, N=6), lti=["plant"])
    assert plan.no == 144 and plan.resident["ok"] == 0
    for path in (0, 1, 3, 4):
        with pytest.raises(capi.MpcasmError) as refusal:
            engine.tiled_route(plan, 19, [1] * len(plan.sources), path=path)
        assert refusal.value.status == capi.ERR_LIMIT


def test_the_shared_form_needs_every_source_shared(cpu_api):
    """One source of an instance's own, fewer than 8 instances: the general kernel."""
    case = tc.BY_NAME["shared-7"]
    _, _, _, _, plan = _compiled(cpu_api, case)
    n = len(plan.sources)
    assert engine.tiled_route(plan, 67).form == tc.SHARED
    assert engine.tiled_route(plan, 67, [0] * (n - 1) + [8]).form == tc.GENERAL
    assert engine.tiled_route(plan, 7).form == tc.GENERAL
    assert engine.tiled_route(plan, 16).tg == 8 and engine.tiled_route(plan, 15).form == tc.GENERAL   # (2 x 8 weights)
