"""CPU: what the staged pipeline launches for a plan (csrc/assemble.hip, staged_choose) as the library itself reports
it -- mpcasm_staged_route, the very function the launch decides with -- and which plans the per-instance fused kernel
takes (mpcasm_assemble_route).  Every case of the family in staged_cases.py is pinned to its route and to the facts of
its plan's tables (which branch of K4 a row takes, which blocks a term's masks leave empty: staged_cases.table_facts),
the family is held to reach EVERY selectable variant, and the bound the GPU test applies (helpers.kappa) is shown to
leave room for a correct fp64 computation on the very kind of inputs that test uses: the pipeline's own tables in
fp64 (plan_emulator.run), for the wide plans the fp64 oracle, stay within HALF of it."""
import ctypes

import numpy as np
import pytest

import plan_emulator
import staged_cases as sc
import sweep_cases
from helpers import assert_componentwise, kappa
from mpcasm import capi, engine
from mpcasm.plan import _H, FUSED_MAX_OPS
from oracle import qp_oracle as orc

IDS = [c.shape.name for c in sc.CASES]
_COMPILED = {}      # case name -> (plant, form, plan): compiled once, shared by the tests, left unchanged


def _compiled(api, case, seed=11):
    name = case.shape.name
    if name not in _COMPILED:
        rng = np.random.default_rng(seed)
        plant = sc.instance(sc.plants(rng, 1, case.shape), 0)
        _COMPILED[name] = (plant,) + sc.compile_case(api, rng, case, plant)
    return (np.random.default_rng(seed + 1),) + _COMPILED[name]


def _pinned(r, kernel, lds=None):
    return sc.Route(kernel, r.hessian, r.sym, r.nb, r.npairs, r.nbr, r.nbc, r.whole_lines, r.max_axes, lds)


def _branches(facts):
    """The branches of K4 the rows of a plan take, (branch, whole_lines): by the parity of no and each row's axes."""
    if facts["odd"]:
        return {("scalar", 0)}
    whole = int(facts["no"] % 16 == 0)
    return {("pairs", whole) if axes <= 2 else ("loop", 0) for axes in facts["axes"]}


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_every_case_takes_its_route(cpu_api, case):
    _, _, form, plan = _compiled(cpu_api, case)
    it, batch = plan.itab, case.batch
    facts = sc.table_facts(plan)
    assert {key: facts[key] for key in case.facts} == case.facts
    assert facts["nc_mod16"] != 0                       # (a last row block of fewer than 16 rows, every case)
    assert plan.no == case.facts["no"] and not plan.lti
    # the family's kernel: what mpcasm_assemble says for the case's path; the route below is what that launch runs
    kernel = engine.assemble_route(plan, batch, path=case.path)
    if case.route == sc.LIMIT:
        assert kernel.kernel == capi.KERNEL_STAGED      # (the refusal is the pipeline's own)
        with pytest.raises(capi.MpcasmError) as refusal:
            engine.staged_route(plan, batch)
        assert refusal.value.status == capi.ERR_LIMIT
        with pytest.raises(capi.MpcasmError) as refusal:
            engine.staged_route(plan, batch, want_cost=False)
        assert refusal.value.status == capi.ERR_LIMIT
        cost = engine.staged_route(plan, batch, want_constraints=False)     # (P, q alone: nothing to refuse)
        assert cost.hessian == capi.STAGED_BLOCK and cost.grid_k4 == 0
        return
    assert kernel.kernel == case.route.kernel, kernel
    if case.route.kernel == sc.FUSED:
        assert kernel.lds == case.route.lds and kernel.lds <= 80 * 1024
        assert engine.assemble_route(plan, batch, path=2).kernel == capi.KERNEL_STAGED
        nt = -(-plan.no // 16)
        assert nt * nt <= 36 and plan.no <= 128 and facts["axes"][-1] <= 4 and it[_H["FUSED_OK"]] == 1
    else:
        assert kernel.lds == 0
    r = engine.staged_route(plan, batch)
    assert _pinned(r, case.route.kernel, case.route.lds) == case.route, r
    assert r.max_axes == facts["axes"][-1]
    # the grids follow from the sizes: 16 rows of V, 4 blocks of 32 x 32, a block pair of 128 x 128, 64 columns of
    # q, 16 rows of G per workgroup -- K4's dealt to the XCDs in groups of eight instances
    up = lambda a, b: -(-a // b)
    assert r.grid_k2 == up(int(it[_H["RTOT"]]), 16) * batch
    if r.hessian == capi.STAGED_GEMM:
        assert (r.grid_k3, r.grid_gradient) == (r.npairs * batch, up(plan.no, 64) * batch)
        assert r.sym == (0 if facts["crossed"] else 1)
    else:
        assert (r.grid_k3, r.grid_gradient) == (up(r.nbr * r.nbc, 4) * batch, 0)
    assert r.grid_k4 == up(plan.nc, 16) * up(batch, 8) * 8
    # one half at a time
    cost, limits = engine.staged_route(plan, batch, want_constraints=False), engine.staged_route(plan, batch, want_cost=False)
    assert cost == r._replace(grid_k4=0, whole_lines=0)
    assert limits == r._replace(hessian=capi.STAGED_NONE, sym=0, nb=0, npairs=0, nbr=0, nbc=0, grid_k3=0, grid_gradient=0)
    # the masks are all ones beyond FUSED_MAX_OPS: the fused program is then not made
    assert not facts["all_ones"] or (it[_H["FUSED_OK"]] == 0 and it[_H["NOPS"]] == 0)


def test_the_family_reaches_every_selectable_variant(cpu_api):
    hessians, branches, parities, masks, fused, block = set(), set(), set(), set(), set(), set()
    for case in sc.CASES:
        _, _, form, plan = _compiled(cpu_api, case)
        facts = sc.table_facts(plan)
        if case.route == sc.LIMIT:
            continue
        r = engine.staged_route(plan, case.batch)
        if case.route.kernel == sc.FUSED:
            nt = -(-plan.no // 16)
            fused |= {("tiles", nt), ("odd", facts["odd"]), ("second q column", int(plan.no > 64)),
                      ("axes", facts["axes"][-1]), ("skip", int(facts["skip16"])), ("rows % 4", int(facts["rows_mod4"])),
                      ("halves", int(case.halves)), ("zero weight", int(case.zero_weight))}
            continue
        parities.add(facts["odd"])
        branches |= _branches(facts)
        if r.hessian == capi.STAGED_GEMM:
            hessians.add(("gemm", r.sym, min(r.nb, 3)))
            masks.add(("gemm", "all-ones" if facts["all_ones"] else "skip" if facts["skip128"] else "none"))
            block |= {("odd tail", facts["odd"]), ("short stage", int(facts["short_stage"])),
                      ("rows % 4", int(facts["rows_mod4"])), ("beyond tile 30", int(8 * (r.nb - 1) >= 30)),
                      ("second K4 trip", int(plan.no > 128 and not facts["odd"]))}
        else:
            hessians.add(("block", r.nbr, r.nbc))
            masks.add(("block", "skip" if facts["skip32"] else "none"))
    # every Hessian form x sym x (nb = 1, 2, >= 3); the block kernel from one block to 4 x 4, with q alone in a block
    # column of its own (nbc = nbr + 1) and inside the last one
    assert {("gemm", sym, nb) for sym in (0, 1) for nb in (1, 2, 3)} <= hessians
    assert {("block", 1, 1), ("block", 1, 2), ("block", 2, 2), ("block", 2, 3), ("block", 3, 4), ("block", 4, 4)} <= hessians
    # every branch of K4 x whole_lines (the scalar branch and the loop over axes write no whole lines)
    assert branches == {("scalar", 0), ("pairs", 0), ("pairs", 1), ("loop", 0)}
    assert parities == {0, 1}
    assert masks == {("gemm", "all-ones"), ("gemm", "skip"), ("gemm", "none"), ("block", "skip"), ("block", "none")}
    for key in ("odd tail", "short stage", "rows % 4", "beyond tile 30", "second K4 trip"):
        assert {(key, 0), (key, 1)} <= block, key
    # the fused kernel: one tile; all 36 tile slots; odd; the second q column; 3 and 4 axes; a tile skipped; rows % 4
    assert {("tiles", 1), ("tiles", 6), ("odd", 0), ("odd", 1), ("second q column", 0), ("second q column", 1),
            ("axes", 1), ("axes", 3), ("axes", 4), ("skip", 0), ("skip", 1), ("rows % 4", 0), ("rows % 4", 1),
            ("halves", 1), ("zero weight", 1)} <= fused
    # 3, 5 and 8 axes at even no on the pipeline; per-row arrows, centres and extremes; one staged and one fused case
    # with a weight of exactly 0, with halves, with parameters of their own
    axes = {sc.table_facts(_compiled(cpu_api, c)[3])["axes"][-1] for c in sc.CASES if c.route != sc.LIMIT
            and c.route.kernel == sc.STAGED}
    assert {1, 3, 5, 8} <= axes
    per_row = sc.table_facts(_compiled(cpu_api, sc.BY_NAME["per-row"])[3])
    assert per_row["per_row"] and per_row["per_row_center"] and per_row["per_row_extreme"]
    for kernel in (sc.STAGED, sc.FUSED):
        mine = [c for c in sc.GPU_CASES if c.route.kernel == kernel]
        assert any(c.zero_weight for c in mine) and any(c.halves for c in mine) and any(c.own_params for c in mine)
    assert all(c.batch % 8 and c.batch in (5, sc.WIDE_BATCH, sc.SMALL_BATCH) for c in sc.CASES)


def test_the_masks_of_the_two_plants(cpu_api):
    """A cost on a state of the first plant has no tile over the second plant's columns, and the other way round; a
    plan beyond FUSED_MAX_OPS has every bit set."""
    _, _, _, plan = _compiled(cpu_api, sc.BY_NAME["gemm-160-two-plants"])
    gt = np.asarray(plan.itab[plan.itab[_H["OFF_GTERM"]]:][:plan.itab[_H["NGTERM"]] * 10]).reshape(-1, 10)
    dense = gt[(gt[:, 6] & 4) == 0]
    first, second = 0xFF, 0x300                         # tiles 0 .. 7: columns 0 .. 127; tiles 8, 9: 128 .. 159
    assert {int(m) for m in dense[:, 7]} == {first, second} and (dense[:, 7] == dense[:, 8]).all()
    _, _, _, plan = _compiled(cpu_api, sc.BY_NAME["gemm-208-all-ones"])
    gt = np.asarray(plan.itab[plan.itab[_H["OFF_GTERM"]]:][:plan.itab[_H["NGTERM"]] * 10]).reshape(-1, 10)
    assert (gt[(gt[:, 6] & 4) == 0][:, 7:9] == 0x7FFFFFFF).all() and FUSED_MAX_OPS == 1 << 18


def _inputs(case, rng, form, plan):
    """given and the parameters of one instance, of the GPU test's kind."""
    given = rng.normal(0, 0.3, form.given_len)
    params = np.array(plan.params, dtype=float)
    if case.own_params:
        params = sweep_cases.perturb_params(plan, params[None].copy(), rng)[0]
    return given, params


@pytest.mark.parametrize("case", sc.GPU_CASES, ids=[c.shape.name for c in sc.GPU_CASES])
def test_the_bound_has_room_for_fp64(cpu_api, case):
    """Not a measurement of the kernel: fp64 arithmetic on plants and a formulation of the GPU test's kind -- through
    the pipeline's own tables (plan_emulator.run: the workspace rows, the terms' products, the rows of G) up to 100
    unknowns, by the fp64 oracle beyond -- stays within half of kappa(N, n) of long double, so a kernel beyond kappa
    is at fault, not the bound."""
    rng, plant, form, plan = _compiled(cpu_api, case)
    given, params = _inputs(case, rng, form, plan)
    with sweep_cases.instance_params(form, plan) as objects:
        objects.set(params)
        if plan.no <= 100:
            mine = plan_emulator.run(plan, given, params=params)
        else:
            G, h, P, q = orc.assemble(form, given.reshape(-1, 1))
            mine = {"G": G, "h": h.ravel(), "P": P, "q": q.ravel()}
        ref = sc.reference(form, plant, given)
    kap, worst = kappa(case.shape.N, case.shape.n), 0.0
    for key in "PqGh":
        worst = max(worst, assert_componentwise(mine[key], *ref[key], kap // 2, "%s %s" % (case.shape.name, key)))
    print("componentwise %-60s worst %8.3g u M   kappa %d" % ("fp64 " + case.shape.name, worst, kap))


def test_the_reference_over_two_plants_is_the_helpers(cpu_api):
    """staged_cases.reference with a second plant against helpers.precise_reference where the second plant is the
    formulation's own: the same numbers for the rows and columns of the first."""
    from helpers import precise_reference

    case = sc.BY_NAME["fused-two-plants"]
    rng, plant, form, plan = _compiled(cpu_api, case)
    given = rng.normal(0, 0.3, form.given_len)
    both = sc.reference(form, plant, given)
    one = precise_reference(form, "plant", *plant["plant"], given)
    cols = case.shape.m * case.shape.N
    for key in "PqGh":
        assert both[key][0].shape == one[key][0].shape
    # (the second plant's matrices are the fp64 ones in `one`, long double in `both`: the first plant's block agrees)
    assert np.array_equal(both["P"][0][:cols, :cols], one["P"][0][:cols, :cols])
    assert np.array_equal(both["P"][1][:cols, :cols], one["P"][1][:cols, :cols])


def test_query_checks_its_arguments(cpu_api):
    _, _, _, plan = _compiled(cpu_api, sc.BY_NAME["gemm-129"])
    lib = capi.load()
    itab, dtab = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab)
    out = (ctypes.c_int32 * 8)(*([7] * 8))
    args = (itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size)
    assert lib.mpcasm_staged_route(*args, 1, 1, 11, out) == 0
    assert list(out) == [capi.STAGED_GEMM, capi.STAGED_SYM | (1 << 8), 2, 3, 9 * 11, 3 * 11, 3 * 11, 6 * 16]
    assert lib.mpcasm_staged_route(*args, 1, 1, 11, None) == -1
    assert lib.mpcasm_staged_route(None, itab.size, dtab.ctypes.data, dtab.size, 1, 1, 11, out) == -1
    assert lib.mpcasm_staged_route(*args, 0, 0, 11, out) == -1              # (no half wanted)
    assert lib.mpcasm_staged_route(*args, 2, 1, 11, out) == -1
    assert lib.mpcasm_staged_route(*args, 1, -1, 11, out) == -1
    assert lib.mpcasm_staged_route(*args, 1, 1, 0, out) == -1               # (no instance)
    assert lib.mpcasm_staged_route(itab.ctypes.data, 4, dtab.ctypes.data, dtab.size, 1, 1, 11, out) == -2
    # the refusal zeroes out
    _, _, _, over = _compiled(cpu_api, sc.BY_NAME["axes-9"])
    itab, dtab = np.ascontiguousarray(over.itab), np.ascontiguousarray(over.dtab)
    out = (ctypes.c_int32 * 8)(*([7] * 8))
    assert lib.mpcasm_staged_route(itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size, 1, 1, 70, out) == capi.ERR_LIMIT
    assert list(out) == [0] * 8


def test_plans_the_pipeline_cannot_run_are_refused(cpu_api):
    """MPCASM_ERR_ARG: a plan compiled with lti= (its horizon matrices exist on chip only), one compiled with ltv=."""
    from helpers import lti_tracking_problem
    from mpcasm import problems
    from mpcasm.plan import compile_plan

    rng = np.random.default_rng(3)
    lti = compile_plan(lti_tracking_problem(cpu_api, rng, 3, 2, 8)[0], lti=["plant"])
    ltv = compile_plan(problems.lipm_ltv(cpu_api, N=16), ltv=["LIP"])
    for plan in (lti, ltv):
        with pytest.raises(capi.MpcasmError) as refusal:
            engine.staged_route(plan, 19)
        assert refusal.value.status == capi.ERR_ARG
