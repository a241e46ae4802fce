"""CPU: what a plan selects inside the persistent kernel (csrc/resident.hip), read from its RS_* words as the launch
reads them.  Every case of the family in persistent_cases.py compiles to a plan the kernel takes (RS_OK) with the
variant tuple its entry pins and an LDS footprint within the kernel's limit (mpcasm_resident_lds_bytes); the family
is held to reach EVERY value of every axis (all five launch_jc instantiations with the horizon tables made on chip
and fetched from memory, the four modes of G, both workspaces, ...) by enumeration; and the bound the GPU test
applies is shown to leave room for a correct fp64 computation of the resident program
(plan_emulator.run_resident) on the very kind of inputs that test uses: it stays within HALF of it."""
import ctypes

import numpy as np
import pytest

import persistent_cases as pc
import plan_emulator
import sweep_cases as sc
from helpers import assert_componentwise
from mpcasm import capi, engine
from mpcasm.plan import _H, LM_WORDS, RS_AXMAX, RS_DIAG_MAX

RESIDENT_LDS_LIMIT = 156 * 1024          # csrc/plan_dev.h
IDS = [c.name for c in pc.CASES]
_COMPILED = {}      # case name -> (rng, plants, form, given, plan): compiled once, shared by the tests, left unchanged


def _compiled(api, case):
    if case.name not in _COMPILED:
        rng, plants, form, given = pc.inputs(api, case, 1)
        _COMPILED[case.name] = (rng, plants, form, given, pc.compile_case(form, case))
    return _COMPILED[case.name]


def _most_axes(plan):
    """The most axes of a limit of the plan (the launch's max_axes)."""
    it = plan.itab
    lims = np.asarray(it[it[_H["OFF_LIMIT"]]:it[_H["OFF_LIMIT"]] + it[_H["NLIMIT"]] * LM_WORDS]).reshape(-1, LM_WORDS)
    return int(lims[:, 2].max())


@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_every_case_selects_its_variant(cpu_api, case):
    _, _, form, _, plan = _compiled(cpu_api, case)
    it = plan.itab
    assert it[_H["RS_OK"]] == 1 and plan.resident["ok"]
    assert pc.variant_of(plan) == case.variant
    assert (it[_H["RS_NLTI"]] == 0) == ("lti" not in case.kw)
    assert [(g["name"], g["n"], g["m"], g["N"]) for g in plan.lti] \
        == ([(name, n, m, case.N) for name, n, m in case.systems] if "lti" in case.kw else [])
    direct, in_lds = engine.resident_lds_bytes(plan)
    assert 0 < direct <= RESIDENT_LDS_LIMIT
    assert (0 < in_lds <= RESIDENT_LDS_LIMIT) == case.p_in_lds
    assert (plan.csc is not None) == ("csc" in case.kw) == (case.variant.g_mode == 3)
    assert it[_H["RS_NCHUNK"]] <= 32


def test_the_family_reaches_every_axis_value(cpu_api):
    reached = set()
    for case in pc.CASES:
        _, _, _, _, plan = _compiled(cpu_api, case)
        v = pc.variant_of(plan)
        reached |= {("jc", v.jc_inst, v.gen), ("g_mode", v.g_mode), ("unit", v.unit, v.gen), ("nlti", v.nlti)}
        if v.compact:
            reached.add(("compact", v.g_mode))
        if v.gfix and v.g_mode == 2:
            reached.add(("gfix", v.compact))
        if v.sym == 0 and case.p_in_lds:
            reached.add(("sym 0, P in LDS",))
        if v.g_mode in (2, 3):
            reached.add(("gsingle", v.g_mode, v.gsingle))
        if v.nzblk and v.nsplit:
            reached.add(("nzblk and nsplit",))
    required = set(pc.REQUIRED)
    assert len(required) == len(pc.REQUIRED) == 10 + 4 + 2 + 2 + 1 + 4 + 4 + 4 + 1
    assert set(pc.UNREACHABLE) <= required
    missing = required - set(pc.UNREACHABLE) - reached
    assert not missing, "no case reaches %s" % sorted(missing, key=str)
    assert not reached & set(pc.UNREACHABLE), "reached after all: take it off the list of exceptions"
    for combination in sorted(required, key=str):
        print("%-40s %s" % (combination, pc.UNREACHABLE.get(combination, "reached")))
    # the sizes the kernel's tables take: the most axes a row record holds, the most image chunks of a plan here
    assert max(_most_axes(_compiled(cpu_api, c)[4]) for c in pc.CASES) == RS_AXMAX
    assert max(int(_compiled(cpu_api, c)[4].itab[_H["RS_NCHUNK"]]) for c in pc.CASES) == 32


def test_a_column_carries_two_diagonal_costs_and_no_third(cpu_api):
    case = pc.BY_NAME["diagonal-3-2-6"]
    _, _, _, _, plan = _compiled(cpu_api, case)
    it, no, nparams = plan.itab, plan.no, int(plan.itab[_H["NPARAMS"]])
    dpar = np.asarray(it[it[_H["OFF_RS_DPAR"]]:it[_H["OFF_RS_DPAR"]] + 2 * RS_DIAG_MAX * no]).reshape(no, 2 * RS_DIAG_MAX)
    both = (dpar[:, 0] != nparams) & (dpar[:, 2] != nparams)
    assert both.sum() == case.N and (dpar[:, 0] != nparams).all()         # (u0: two terms; the other input: one)
    for name, make in pc.REFUSED.items():
        third = case._replace(name=name, make=make)
        _, _, form, _ = pc.inputs(cpu_api, third, 1)
        refused = pc.compile_case(form, third)
        assert refused.itab[_H["RS_OK"]] == 0 and not refused.resident["ok"]


@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_the_bound_has_room_for_the_resident_program(cpu_api, case):
    """Not a measurement of the kernel: fp64 arithmetic in the resident program's own order (the image, the compose
    ops, the packs of 4x4 blocks, the pieces of G) on a plant, a given and parameters of the GPU test's kind stays
    within half of the case's kappa of long double -- so a kernel beyond kappa is at fault, not the bound."""
    rng, plants, form, given, plan = _compiled(cpu_api, case)
    params = pc.params_of(plan, case, 1)[0]
    mine = plan_emulator.run_resident(plan, given[0], params=params,
                                      sources=pc.emulator_sources(plan, case, plants, 0))
    with sc.instance_params(form, plan) as objects:
        objects.set(params)
        ref = pc.reference(form, case, plants, 0, given[0])
    if plan.csc:
        ref = pc.csc_reference(ref, plan.csc)
        mine = dict(mine, P=mine["P_data"], G=mine["G_data"])
    kap, worst = pc.kappa_of(case), 0.0
    for key in "PqGh":
        worst = max(worst, assert_componentwise(mine[key], *ref[key], kap // 2, "%s %s" % (case.name, key)))
    print("componentwise %-60s worst %8.3g u M   kappa %d" % ("fp64 resident program " + case.name, worst, kap))


FETCH = [c for c in pc.CASES if c.fetch_runs]


@pytest.mark.parametrize("case", FETCH, ids=[c.name for c in FETCH])
def test_the_limit_of_runs_leaves_chunks_of_both_kinds(cpu_api, case):
    """The two builds of the per-plan kernel the GPU test adds for these cases: at a limit of 0 runs every chunk
    stays on the table, at persistent_cases.fetch_limit some are fetched by arithmetic and some are not -- and
    that kernel compiles (mpcasm_jit_check, no device needed)."""
    from test_fetch_segments_cpu import fetch_segments

    _, _, _, _, plan = _compiled(cpu_api, case)
    assert "lti" in case.kw and len(FETCH) == 2
    limit = pc.fetch_limit(plan, fetch_segments)
    assert not any(fetch_segments(plan, 0).values())
    kinds = {bool(runs) for runs in fetch_segments(plan, limit).values()}
    assert kinds == {False, True}
    lib = capi.load()
    log = ctypes.create_string_buffer(1 << 16)
    assert lib.mpcasm_set_option(capi.OPT_JIT_FETCH_RUNS, limit) == 0
    try:
        rc = lib.mpcasm_jit_check(plan.itab.ctypes.data, plan.itab.size, plan.dtab.ctypes.data, plan.dtab.size,
                                  log, len(log))
    finally:
        assert lib.mpcasm_set_option(capi.OPT_JIT_FETCH_RUNS, 8) == 0
    assert rc == 0, log.value.decode()
