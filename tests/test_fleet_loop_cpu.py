"""CPU: the host side of the closed walking loop (WalkerFleet.step) -- the given map of the biped is the
reference's update_given_collector, record by record, in every structure bucket; the map's rules are
checked; and the fleet's index of rows is refused unless its entries are distinct and in range."""
import numpy as np
import pytest

from fleet_loop_reference import rest_given, update_given
from mpcasm import capi, problems
from mpcasm.engine import given_map_records
from mpcasm.plan import compile_plan
from mpcasm.walkers import biped_given_rules, checked_index, steps_in_preview
from oracle import qp_oracle as orc


def bucket_forms(api, conf):
    """One biped formulation per structure bucket (steps in the preview), as WalkerFleet builds them."""
    n, out = conf.step_samples, {}
    for phi in range(n):
        times = np.array([(i + 1) * n - 1 - phi for i in range(conf.num_steps)])
        p = int(steps_in_preview(times, conf.horizon_lenght).sum())
        if p not in out:
            form = problems.biped(api, conf)
            form.update(step_times=times, step_count=phi % 3)
            out[p] = form
    return out


def apply_records(rows, values, given, pv):
    """What mpcasm_next_given writes, restated: a row of the preview program, a constant, or the old value."""
    out = np.array(given, dtype=np.float64)
    named = rows >= 0
    out[named] = pv[rows[named]]
    const = rows == capi.GIVEN_CONST
    out[const] = values[const]
    return out


def preview_program(form, plan, given, optim):
    """The oracle's rows of every definition, laid out as the plan's preview program (plan.pm_rows)."""
    PM = orc.preview_matrices(form)
    pv = np.full(plan.pmrows, np.nan)
    for v, (r0, n) in plan.pm_rows.items():
        pv[r0:r0 + n] = orc.preview(PM, given.reshape(-1, 1), optim.reshape(-1, 1), v).ravel()
    return pv


@pytest.mark.parametrize("step_samples", [8, 12])
def test_the_biped_map_is_the_reference_update(cpu_api, step_samples):
    conf = problems.BipedConfig(step_samples=step_samples)
    forms = bucket_forms(cpu_api, conf)
    assert len(forms) == 2
    rng = np.random.default_rng(7)
    for p, form in forms.items():
        plan = compile_plan(form)
        assert plan.no == 2 * conf.horizon_lenght + 2 * p
        rows, values = given_map_records(plan, biped_given_rules(form))
        # every column is written: x0 and s0 from preview rows, the bias from constants
        assert (rows != capi.GIVEN_KEEP).all()
        assert (rows[rows >= 0] < plan.pmrows).all()
        assert sorted(rows[rows >= 0]) == sorted(
            [plan.pm_rows[s][0] for s in form.dynamics["LIP"].state_ID] +
            [plan.pm_rows[s][0] + 1 for s in form.dynamics["steps"].state_ID])
        for _ in range(5):
            given = rng.normal(0, 0.3, plan.ng)
            optim = rng.normal(0, 0.3, plan.no)
            pv = preview_program(form, plan, given, optim)
            assert not np.isnan(pv).any()
            mine = apply_records(rows, values, given, pv)
            ref = update_given(form, given, optim).ravel()
            assert np.array_equal(mine, ref), (p, np.abs(mine - ref).max())


def test_the_state_rows_sit_where_the_plan_lays_them_out(cpu_api):
    conf = problems.BipedConfig(step_samples=8)
    form = bucket_forms(cpu_api, conf)[2]
    plan = compile_plan(form)
    assert plan.no == 36
    assert plan.pm_rows["s_x"] == (6, 16) and plan.pm_rows["CoM_x"] == (82, 16)
    rows, _ = given_map_records(plan, biped_given_rules(form))
    assert rows[plan.given_ID["x0_x"][0]] == 82          # CoM_x, sample 0
    assert rows[plan.given_ID["s0_x"][0]] == 6 + 1       # s_x, sample 1


def test_rules_of_every_kind_and_what_they_refuse(cpu_api):
    conf = problems.BipedConfig(step_samples=8)
    form = bucket_forms(cpu_api, conf)[1]
    plan = compile_plan(form)
    gid = plan.given_ID
    rows, values = given_map_records(plan, {"x0_x": [("CoM_x", 3), None, ("DCM_x", 15)], "n_y": -0.5})
    assert rows[gid["x0_x"][0]] == plan.pm_rows["CoM_x"][0] + 3
    assert rows[gid["x0_x"][1]] == capi.GIVEN_KEEP
    assert rows[gid["x0_x"][2]] == plan.pm_rows["DCM_x"][0] + 15
    assert (rows[gid["n_y"].start:gid["n_y"].stop] == capi.GIVEN_CONST).all()
    assert (values[gid["n_y"].start:gid["n_y"].stop] == -0.5).all()
    keep = [c for c in range(plan.ng) if c not in gid["x0_x"] and c not in gid["n_y"]]
    assert (rows[keep] == capi.GIVEN_KEEP).all()
    with pytest.raises(KeyError):
        given_map_records(plan, {"x0_z": 0.0})
    with pytest.raises(KeyError):
        given_map_records(plan, {"x0_x": [("CoM_z", 0), None, None]})
    with pytest.raises(ValueError):
        given_map_records(plan, {"x0_x": [("CoM_x", 16), None, None]})
    with pytest.raises(ValueError):
        given_map_records(plan, {"x0_x": [("CoM_x", 0)]})
    with pytest.raises(ValueError):
        given_map_records(plan, {"n_x": float("nan")})


def test_the_start_at_rest_is_the_reference_start(cpu_api):
    conf = problems.BipedConfig(step_samples=8)
    form = problems.biped(cpu_api, conf)
    given = rest_given(form, conf)
    assert given[form.given_ID["x0_y"][0]] == given[form.given_ID["s0_y"][0]] == conf.strt_y
    assert np.count_nonzero(given) == 2


def test_an_index_of_rows_must_be_distinct_and_in_range():
    assert checked_index(np.array([3, 0, 2]), 4).dtype == np.int32
    assert checked_index(np.array([], dtype=np.int64), 0).size == 0
    for bad in ([0, 4], [-1, 2], [1, 1]):
        with pytest.raises(ValueError):
            checked_index(np.array(bad), 4)


def test_the_qp_bits_of_the_two_rules():
    from mpcasm import engine

    bits = lambda mask: {s for s in capi.QP_STATUS if mask & capi.qp_bit(s)}
    assert bits(engine.APPLY_SOLVED) == {capi.QP_SOLVED, capi.QP_MAX_ITER}
    assert bits(engine.APPLY_ALL) == set(capi.QP_STATUS) - {capi.QP_NON_CVX}
