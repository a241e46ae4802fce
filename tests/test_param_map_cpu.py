"""CPU: the host side of the fleet's commands -- the biped's command rules compiled to the records of a parameter
map, the restated map (tests/param_map_restatement.py) against the plan's own parameters on every place of the
step cycle, what the rule compiler refuses, and the library's entry as far as it answers without a device."""
import ctypes

import numpy as np
import pytest

import param_map_restatement as pm
from mpcasm import capi, problems
from mpcasm.engine import check_param_map_sign, param_map_records
from mpcasm.plan import compile_plan
from mpcasm.walkers import COMMAND_COLUMNS, biped_command_rules, stepping_area_facets

SLOTS = {34: [8, 10, 16, 17, 21, 22, 26, 27, 31, 32],
         36: [8, 10, 16, 17, 18, 19, 23, 24, 25, 26, 30, 31, 32, 33, 37, 38, 39, 40]}


def config(commands=None):
    conf = problems.BipedConfig(step_samples=8)
    if commands is not None:
        conf.target_vel = np.array([commands[0], commands[1], 0.0])
        conf.stepping_center = np.array([commands[2], commands[3]])
    return conf


def default_commands(conf):
    return np.array([conf.target_vel[0], conf.target_vel[1], conf.stepping_center[0], conf.stepping_center[1]])


def form_at(api, conf, step_times, step_count):
    form = problems.biped(api, conf)
    form.update(step_times=np.array(step_times), step_count=int(step_count))
    return form


def commanded_slots(form, plan):
    """The elements the commands reach, from the plan's own slots: both aims and the centres of every facet."""
    keys = [("cost", "track vel_x", "aim"), ("cost", "track vel_y", "aim")]
    keys += [("limit", k, "center") for k in stepping_area_facets(form)]
    out = []
    for key in keys:
        start, rows, cols = plan.param_slots[key]
        out.extend(range(start, start + rows * cols))
    return sorted(out)


def places_of_the_cycle(conf, phase):
    """``(step times, step count)`` at each of the 16 places of the step cycle of a walker ``phase`` ticks ahead."""
    clock = problems.StepClock(conf.step_samples, conf.num_steps)
    for _ in range(phase):
        clock.tick()
    out = []
    for _ in range(2 * conf.step_samples):
        out.append((np.array(clock.step_times), int(clock.step_count)))
        clock.tick()
    return out


# ---- 1. the record sets -------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase, width", [(0, 34), (7, 36)])
def test_the_biped_rules_compile_to_the_commanded_slots(cpu_api, phase, width):
    conf = config()
    form = form_at(cpu_api, conf, [7 - phase, 15 - phase], 0)
    plan = compile_plan(form)
    assert plan.no == width
    recs, coef = param_map_records(plan, biped_command_rules(form), COMMAND_COLUMNS)
    assert recs.dtype == np.int32 and recs.shape == (len(SLOTS[width]), 4)
    assert coef.dtype == np.float64 and coef.shape == (len(SLOTS[width]), 2)
    assert sorted(recs[:, 0].tolist()) == commanded_slots(form, plan) == SLOTS[width]
    assert set(recs[:, 1].tolist()) == {0, 1, 2, 3} and not recs[:, 3].any()
    signed = recs[:, 2] == pm.SIGNED
    assert set(recs[:, 2].tolist()) == {0, pm.SIGNED} and (recs[signed, 1] == 3).all() and (recs[~signed, 1] != 3).all()
    assert set(np.abs(coef[:, 1]).tolist()) == {1.0} and (coef[~signed, 1] == 1.0).all() and not coef[:, 0].any()


# ---- 2. / 3. the restated map against the plan's own parameters -----------------------------------------------
def check_cycle(api, commands, phases):
    """On every place of the cycle of the walkers ``phases``: a template row (the default configuration's
    parameters at that structure, the commanded elements spoiled) with the map applied equals the parameters of a
    form configured with ``commands``, bit for bit, and differs from the template in the commanded slots only."""
    conf_t, conf_c = config(), config(commands)
    cmd = default_commands(conf_t) if commands is None else np.asarray(commands, dtype=np.float64)
    parities, widths, places = set(), set(), 0
    for phase in phases:
        for times, count in places_of_the_cycle(conf_t, phase):
            form = form_at(api, conf_c, times, count)
            plan = compile_plan(form)
            want = plan.current_params()
            template_form = form_at(api, conf_t, times, 0)
            tplan = compile_plan(template_form)
            assert tplan.param_slots == plan.param_slots
            recs, coef = param_map_records(tplan, biped_command_rules(template_form), COMMAND_COLUMNS)
            slots = commanded_slots(template_form, tplan)
            template = tplan.current_params().copy()
            other = np.setdiff1d(np.arange(template.size), slots)
            assert np.array_equal(template[other].view(np.int64), want[other].view(np.int64))
            template[slots] = np.nan
            sign = np.array([(-1.0) ** (count + 1)])
            got = pm.apply_map(template[None, :], recs, coef, cmd[None, :], sign=sign)[0]
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), (phase, times, count)
            parities.add(count % 2)
            widths.add(plan.no)
            places += 1
    return parities, widths, places


def test_default_commands_give_the_plans_own_parameters(cpu_api):
    parities, widths, places = check_cycle(cpu_api, None, range(8))
    assert parities == {0, 1} and widths == {34, 36} and places == 8 * 16


def test_changed_commands_give_the_parameters_of_a_form_configured_so(cpu_api):
    parities, widths, places = check_cycle(cpu_api, (0.3, 0.1, 0.05, 0.30), (0, 5))
    assert parities == {0, 1} and widths == {34, 36} and places == 2 * 16


def test_the_itab_does_not_depend_on_the_commands(cpu_api):
    for times in ([7, 15], [0, 8]):
        a = compile_plan(form_at(cpu_api, config(), times, 1))
        b = compile_plan(form_at(cpu_api, config((0.3, 0.1, 0.05, 0.30)), times, 1))
        assert np.array_equal(a.itab, b.itab)


# ---- 4. refusals -----------------------------------------------------------------------------------------------
def test_the_rule_compiler_refuses(cpu_api):
    form = form_at(cpu_api, config(), [0, 8], 0)
    plan = compile_plan(form)
    facet = ("limit", stepping_area_facets(form)[0], "center")
    aim = ("cost", "track vel_x", "aim")
    with pytest.raises(KeyError):
        param_map_records(plan, {("cost", "no such cost", "aim"): ["vel_x"]}, COMMAND_COLUMNS)
    with pytest.raises(KeyError):
        param_map_records(plan, {aim: ["heading"]}, COMMAND_COLUMNS)
    with pytest.raises(ValueError):
        param_map_records(plan, {facet: ["step_x", "step_y"]}, COMMAND_COLUMNS)          # 2 x 2 elements
    with pytest.raises(ValueError):
        param_map_records(plan, {facet: [["step_x"], ["step_y"], [None], [None]]}, COMMAND_COLUMNS)
    for bad in (dict(c1=float("nan")), dict(c0=float("inf"))):
        with pytest.raises(ValueError):
            param_map_records(plan, {aim: [dict(column="vel_x", **bad)]}, COMMAND_COLUMNS)
    start, rows, cols = plan.param_slots[facet]
    assert (rows, cols) == (2, 2)
    # two entries on one element: a slot named twice cannot happen in a dict, two columns of one name can
    with pytest.raises(ValueError):
        param_map_records(plan, {aim: ["vel_x"]}, ("vel_x", "vel_x"))
    plan.param_slots[("cost", "alias", "aim")] = plan.param_slots[aim]
    try:
        with pytest.raises(ValueError):
            param_map_records(plan, {aim: ["vel_x"], ("cost", "alias", "aim"): ["vel_y"]}, COMMAND_COLUMNS)
    finally:
        del plan.param_slots[("cost", "alias", "aim")]
    # kept elements, constants and coefficients come through as written
    recs, coef = param_map_records(
        plan, {facet: [[None, dict(column="step_y", c0=0.5, c1=-2.0, signed=True)], ["step_x", None]]},
        COMMAND_COLUMNS)
    assert recs.tolist() == [[start + 1, 3, pm.SIGNED | pm.CONST, 0], [start + 2, 2, 0, 0]]
    assert coef.tolist() == [[0.5, -2.0], [0.0, 1.0]]
    # a signed map applied without a sign
    with pytest.raises(ValueError):
        check_param_map_sign(recs, None)
    check_param_map_sign(recs, np.ones(3))
    check_param_map_sign(recs[1:], None)
    empty = param_map_records(plan, {}, COMMAND_COLUMNS)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 2)


def test_the_restated_rule():
    params = np.arange(12, dtype=np.float64).reshape(3, 4)
    recs = [[0, 1, 0, 0], [3, 0, pm.SIGNED | pm.CONST, 0], [4, 0, 0, 0], [1, 2, 0, 0], [2, 0, 4, 0]]
    coef = [[9.0, 2.0], [0.5, -1.0], [0, 1], [0, 1], [0, 1]]
    cmd = np.array([[1.0, 10.0], [2.0, 20.0], [3.0, 30.0], [4.0, 40.0]])
    out = pm.apply_map(params, recs, coef, cmd, index=[3, 0], sign=[-1.0, 1.0, 1.0], count=2)
    assert out.tolist() == [[80.0, 1.0, 2.0, 4.5], [20.0, 5.0, 6.0, -0.5], [8.0, 9.0, 10.0, 11.0]]
    shared = pm.apply_map(params, recs, coef, cmd[1])
    assert shared[:, 0].tolist() == [40.0] * 3 and shared[:, 3].tolist() == [3.0, 7.0, 11.0]   # (no sign: kept)


# ---- 5. the library, as far as it answers without a device ---------------------------------------------------
def test_the_entry_decides_its_arguments_without_a_device():
    lib = capi.load()
    one = ctypes.c_void_p(16)      # (never dereferenced: every call below is decided on the host)

    def call(params=one, n_params=82, recs=one, coef=one, nrecs=18, cmd=one, stride=4, ncmd=4, batch=0):
        return lib.mpcasm_params_map(params, n_params, recs, coef, nrecs, cmd, stride, ncmd, None, None, batch, None)

    assert call() == capi.OK                                                  # batch == 0
    assert call(nrecs=0, batch=5, recs=None, coef=None, cmd=None) == capi.OK  # nrecs == 0
    assert call(stride=0) == capi.OK and call(stride=9) == capi.OK
    for bad in (dict(params=None), dict(recs=None), dict(coef=None), dict(cmd=None), dict(n_params=0),
                dict(nrecs=-1), dict(ncmd=0), dict(batch=-1), dict(stride=-1), dict(stride=3)):
        assert call(**bad) == capi.ERR_ARG, bad
        if "batch" not in bad:                  # ... before any device call, with instances to serve as well
            assert call(batch=4, **bad) == capi.ERR_ARG, bad
    assert call(params=None, nrecs=0, recs=None, coef=None, cmd=None) == capi.ERR_ARG


def test_the_symbol_is_bound_and_the_version_stays():
    lib = capi.load()
    assert "mpcasm_params_map" in capi.SIGNATURES and hasattr(lib, "mpcasm_params_map")
    assert (capi.PMAP_SIGNED, capi.PMAP_CONST) == (pm.SIGNED, pm.CONST) == (1, 2)
    assert lib.mpcasm_abi_version() == 1004
