"""CPU: the instantiation of the sweep kernel a plan runs on (csrc/sweep.hip, sweep_choose) as the library itself
reports it -- mpcasm_sweep_route, the very function the launch decides with.  Every case of the family in
sweep_cases.py is pinned to its route, the family is held to reach EVERY instantiation times every path of the
lines of G, and the bound the GPU test applies (helpers.kappa) is shown to leave room for a correct fp64
computation on the very kind of inputs that test uses: the emulator of the kernel's recursions (small cases) or the
fp64 oracle (wide ones) stays within HALF of it."""
import ctypes

import numpy as np
import pytest

import plan_emulator
import sweep_cases as sc
from helpers import assert_componentwise, kappa, lti_tracking_problem
from mpcasm import capi, engine
from mpcasm.plan import _H
from oracle import qp_oracle as orc

IDS = [c.shape.name for c in sc.CASES]


def _compiled(api, case, seed=11):
    rng = np.random.default_rng(seed)
    A, B = sc.plants(rng, 1, case.shape)
    form, plan = sc.compile_case(api, rng, case.shape, plant=(A[0, 0], B[0, 0]))
    return rng, A[0], B[0], form, plan


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_every_case_takes_its_route(cpu_api, case):
    _, _, _, form, plan = _compiled(cpu_api, case)
    assert plan.no == case.no and plan.itab[_H["SW_OK"]] == 1
    if case.route is sc.LIMIT:
        with pytest.raises(capi.MpcasmError) as refusal:
            engine.sweep_route(plan)
        assert refusal.value.status == capi.ERR_LIMIT
        return
    out = engine.sweep_route(plan)
    assert sc.Route(*out[:6]) == case.route, out
    assert 0 < out[6] <= 160 * 1024 and out[7] == (out[6] > 64 * 1024)
    facts = sc.table_facts(plan)
    assert facts["axes"] == case.shape.axes
    # what the line mode means in the plan's own tables
    if case.route.reg_lines:
        assert facts["fewest_lines"] >= case.route.reg_lines
    if sc.mode_of(case.route) == "per-limit" and plan.nc:
        assert facts["fewest_lines"] == 0 and facts["most_lines"] > case.route.lr


def test_the_family_reaches_every_selectable_variant(cpu_api):
    reached, deep, in_regs, axes, strides = set(), set(), set(), set(), set()
    for case in sc.CASES:
        if case.route is sc.LIMIT:
            continue
        _, _, _, form, plan = _compiled(cpu_api, case)
        r = sc.Route(*engine.sweep_route(plan)[:6])
        facts = sc.table_facts(plan)
        reached.add((r.cpt, r.specialised, r.pair, sc.mode_of(r)))
        if facts["most_lines"] > r.lr:
            deep.add((r.cpt, r.pair, sc.mode_of(r)))
        in_regs.add(facts["partial"] <= 8)
        axes.add(facts["axes"])
        strides |= set(facts["ksteps"])
    assert len(sc.SELECTABLE) == 18 and set(sc.UNREACHABLE) <= sc.SELECTABLE
    missing = sc.SELECTABLE - set(sc.UNREACHABLE) - reached
    assert not missing, "no case reaches %s" % sorted(missing)
    assert reached <= sc.SELECTABLE, "not in the written list: %s" % sorted(reached - sc.SELECTABLE)
    assert not reached & set(sc.UNREACHABLE), "reached after all: take it off the list of exceptions"
    # a step with more lines than LR for every CPT -- beside regular lines (the rest one by one) and, where no line
    # is regular, past the lines fetched at once, per limit and per line
    for cpt, pair in ((1, 0), (2, 1), (2, 0), (4, 0)):
        for mode in sc.MODES:
            assert (cpt, pair, mode) in deep, "no step with more than LR lines on CPT %d PAIR %d, %s" % (cpt, pair, mode)
    assert in_regs == {True, False}
    assert axes == {1, 2, 3, 4}
    assert {0, 2, 3} <= strides and min(strides) >= 0      # (a single step; strided; a descending one folded)


def test_the_table_facts_of_the_special_cases(cpu_api):
    facts = {name: sc.table_facts(_compiled(cpu_api, sc.BY_NAME[name])[4])
             for name in ("terms>8", "desc", "one-step", "pair-a3", "four-a4-n2", "one-4-4-63", "four-noreg", "lipm-33")}
    assert facts["terms>8"]["partial"] == 12 and set(facts["terms>8"]["ksteps"]) == {1, 2, 3}
    assert facts["desc"]["partial"] == 2 and facts["desc"]["ksteps"] == [2]
    assert facts["one-step"]["ksteps"] == [0]
    assert facts["pair-a3"]["terms"] == 12 and facts["pair-a3"]["partial"] == 0
    assert facts["four-a4-n2"]["terms"] == 16 and facts["four-a4-n2"]["partial"] == 8
    assert facts["one-4-4-63"]["most_lines"] == 10
    assert facts["four-noreg"]["most_lines"] == 3
    assert facts["lipm-33"]["most_lines"] == 8 and facts["lipm-33"]["fewest_lines"] == 4


def _fp64_oracle(form, name, N, A, B, given):
    dyn = form.dynamics[name]
    saved = list(dyn.matrices)
    try:
        S, U = orc.extend_matrices_ltv(N, A, B)
        dyn.matrices = list(U) + [S]
        dyn.update_definitions()
        PM = orc.preview_matrices(form)
        g = given.reshape(-1, 1)
        P, q = orc.qp_all_costs(form, PM, g)
        out = {"P": P, "q": q.ravel()}
        if orc.all_limits(form):
            G, h = orc.qp_all_constraints(form, PM, g)
            out.update(G=G, h=h.ravel())
        return out
    finally:
        dyn.matrices = saved
        dyn.update_definitions()


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.route is not sc.LIMIT],
                         ids=[c.shape.name for c in sc.CASES if c.route is not sc.LIMIT])
def test_the_bound_has_room_for_fp64(cpu_api, case):
    """Not a measurement of the kernel: fp64 arithmetic on a plant and a formulation of the GPU test's kind stays
    within half of kappa(N, n), so a kernel beyond kappa is at fault, not the bound."""
    rng, A, B, form, plan = _compiled(cpu_api, case)
    name, N, n = sc.dynamics_name(case.shape), case.shape.N, case.shape.n
    given = rng.normal(0, 0.3, form.given_len)
    if case.no <= 130:
        mine = plan_emulator.run_sweep(plan, given, A, B)
    else:
        mine = _fp64_oracle(form, name, N, A, B, given)
    # (the widest plan: q alone, P's long-double products take a minute)
    ref = sc.reference(form, name, A, B, given, want_P=case.no < 1024)
    worst = 0.0
    for key in "PqGh":
        if key in ref:
            worst = max(worst, assert_componentwise(mine[key], *ref[key], kappa(N, n) // 2, "%s %s" % (case.shape.name, key)))
    print("componentwise %-60s worst %8.3g u M   kappa %d" % ("fp64 " + case.shape.name, worst, kappa(N, n)))


def test_query_checks_its_arguments(cpu_api):
    _, _, _, _, plan = _compiled(cpu_api, sc.BY_NAME["desc"])
    lib = capi.load()
    itab, dtab = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab)
    out = (ctypes.c_int32 * 8)(*([7] * 8))
    args = (itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size)
    assert lib.mpcasm_sweep_route(*args, out) == 0 and out[0] == 2 and out[2] == 1
    assert lib.mpcasm_sweep_route(*args, None) == -1
    assert lib.mpcasm_sweep_route(None, itab.size, dtab.ctypes.data, dtab.size, out) == -1
    assert lib.mpcasm_sweep_route(itab.ctypes.data, 4, dtab.ctypes.data, dtab.size, out) == -2
    # the refusal zeroes out
    _, _, _, _, over = _compiled(cpu_api, sc.BY_NAME["over"])
    itab, dtab = np.ascontiguousarray(over.itab), np.ascontiguousarray(over.dtab)
    out = (ctypes.c_int32 * 8)(*([7] * 8))
    assert lib.mpcasm_sweep_route(itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size, out) == capi.ERR_LIMIT
    assert list(out) == [0] * 8
    # a plan of another kernel
    from mpcasm.plan import compile_plan

    form, _, _ = lti_tracking_problem(cpu_api, np.random.default_rng(3), 3, 2, 8)
    other = compile_plan(form)
    itab, dtab = np.ascontiguousarray(other.itab), np.ascontiguousarray(other.dtab)
    assert lib.mpcasm_sweep_route(itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size, out) == -1
    with pytest.raises(capi.MpcasmError):
        engine.sweep_route(other)
