"""CPU: the row table of the forward rollout of a plan compiled with ``ltv=`` (mpcasm.plan.rollout_rows,
``mpcasm_ltv_rollout_compile``; csrc/rollout.hip reads it) -- every preview row covered once, kinds, steps and
combinations against the formulation's own dense preview matrices; the arithmetic of the kernel, restated in numpy
on the table's very words (rollout_emulator.py), against extended precision under kappa_rollout; the refusals; and
the CPU restatement of the closed loop the GPU test teacher-forces (test_gpu_ltv_loop.py), with the statuses its
inputs were chosen for."""
import numpy as np
import pytest

import rollout_cases as rc
import rollout_emulator as emu
import sweep_cases as sc
from helpers import assert_componentwise
from mpcasm import capi, engine, problems
from mpcasm.plan import ROLL_GIVEN, ROLL_OPTIM, ROLL_STATE, compile_plan, rollout_rows, rollout_sizes

TABLES = [("lipm", N) for N in (1, 2, 33)] + [(name, None) for name in rc.TABLE_SHAPES]


def _compile(api, which, N, rng):
    """``form, plan, dynamics name, (n, m, N, axes)``."""
    if which == "lipm":
        form = problems.lipm_ltv(api, N=N)
        return form, compile_plan(form, ltv=["LIP"]), "LIP"
    shape = rc.shape_of(which)
    form, plan = sc.compile_case(api, rng, shape)
    return form, plan, sc.dynamics_name(shape)


def _nominal(form, name, m):
    """The pair the formulation's horizon matrices were extended from (tools.py:14-33)."""
    mats = form.dynamics[name].matrices
    return mats[m][0].T, np.stack([mats[j][0, 0, :] for j in range(m)], axis=1)


@pytest.mark.parametrize("which,N", TABLES, ids=["%s-%s" % t if t[1] else t[0] for t in TABLES])
def test_the_row_table_against_the_formulation(cpu_api, which, N):
    import preview_cases as pc

    rng = np.random.default_rng(11)
    form, plan, name = _compile(cpu_api, which, N, rng)
    recs, cvec = rollout_rows(plan)
    sw = plan.sweep
    n, m, N, axes = sw["n"], sw["m"], sw["N"], sw["axes"]
    ng, no = plan.ng, plan.no
    # every row of the preview program exactly once, in order; no run crosses a definition
    assert recs[0, 1] == 0 and np.array_equal(recs[1:, 1], np.cumsum(recs[:-1, 2])) and recs[:, 2].sum() == plan.pmrows
    starts = {r0: r0 + rows for r0, rows in plan.pm_rows.values()}
    for kind, row0, count, *_ in recs:
        owner = max(r0 for r0 in starts if r0 <= row0)
        assert row0 + count <= starts[owner]
    # a definition of N rows is ONE run
    for var, (r0, rows) in plan.pm_rows.items():
        assert sum(1 for r in recs if r0 <= r[1] < r0 + rows) == 1, var
    # kinds, steps, combinations: the row of the formulation's dense [Mg | Mo] the record stands for
    A, B = _nominal(form, name, m)
    M = pc.dense_matrix(form, plan)
    powers = [np.eye(n)]
    for _ in range(N):
        powers.append(A @ powers[-1])
    kinds = set()
    for kind, row0, count, axis, k0, kstep, cv, _ in recs:
        kinds.add(int(kind))
        for i in range(count):
            k, want = k0 + i * kstep, np.zeros(ng + no)
            if kind == ROLL_GIVEN:
                want[k] = 1.0
            elif kind == ROLL_OPTIM:
                want[ng + k] = 1.0
            else:
                assert kind == ROLL_STATE and 0 <= k < N and np.all(cvec[cv, n:] == 0)
                c, x0 = cvec[cv, :n], axes[axis, 0]
                want[x0:x0 + n] = c @ powers[k + 1]
                for j in range(m):
                    for l in range(k + 1):
                        want[ng + axes[axis, 1 + j] + l] = c @ powers[k - l] @ B[:, j]
            # (which row it is, not how well it is rounded: both sides are fp64 products of up to N matrices in
            # different orders, so elements that cancel differ in their last bits -- a wrong kind, step or c is
            # off by the size of the row itself)
            np.testing.assert_allclose(M[row0 + i], want, rtol=0, atol=1e-9 * np.abs(M[row0 + i]).max())
    assert kinds == {ROLL_GIVEN, ROLL_OPTIM, ROLL_STATE}
    # the device table: the header is the plan's sizes, the body the records and combinations as they are
    words = engine.rollout_table(plan)
    sizes, trecs, tcvec = emu.parse(words)
    assert [sizes[k] for k in ("n", "m", "N", "axes", "pmrows", "ng", "no")] == list(rollout_sizes(plan))
    assert np.array_equal(trecs, recs) and np.array_equal(tcvec, cvec)


@pytest.mark.parametrize("which,N", TABLES, ids=["%s-%s" % t if t[1] else t[0] for t in TABLES])
def test_the_emulated_rollout_against_extended_precision(cpu_api, which, N):
    rng = np.random.default_rng(23)
    form, plan, name = _compile(cpu_api, which, N, rng)
    sw = plan.sweep
    n, m, N = sw["n"], sw["m"], sw["N"]
    shape = sc.Shape(which, None, n, m, N, sw["axes"].shape[0], 0, False, False, 0, ())
    A, B = sc.plants(rng, 2, shape)
    words = engine.rollout_table(plan)
    kap, worst = rc.kappa_rollout(N, n, m), 0.0
    for b in range(2):
        given, optim = rng.normal(0, 0.3, plan.ng), rng.normal(0, 0.5, plan.no)
        rows = emu.rollout(words, sw["axes"], A[b], B[b], given, optim)
        ref = rc.reference_rows(form, name, A[b], B[b], given, optim, plan)
        worst = max(worst, assert_componentwise(rows, *ref, kap, "%s, instance %d" % (which, b)))
        # the copies are copies
        for kind, row0, count, axis, k0, kstep, cv, _ in emu.parse(words)[1]:
            src = {ROLL_GIVEN: given, ROLL_OPTIM: optim}.get(int(kind))
            if src is not None:
                assert np.array_equal(rows[row0:row0 + count], src[k0:k0 + count * kstep:kstep] if kstep
                                      else src[k0:k0 + 1])
        # ... and the next given is the first sample of every state
        x1 = rc.first_step(plan, A[b, 0], B[b, 0], given, optim)
        assert_componentwise(x1, *rc.next_given_reference(plan, ref), kap, "%s, x_1" % which)
    print("componentwise emulated rollout %-12s worst %8.3g u M   kappa %d" % (which, worst, kap))


def test_a_definition_outside_the_three_kinds_is_named(cpu_api):
    api = cpu_api
    rng = np.random.default_rng(5)
    shape = rc.shape_of("desc")
    for bad, combo in (("twice_u", {"u0_x": 2.0}), ("across", {"s0_x": 1.0, "s0_y": 1.0}),
                       ("mixed", {"s0_x": 1.0, "u0_x": 1.0})):
        form = sc.build(api, rng, shape)
        form.incorporate_definition(bad, api.LineCombo(combo))
        form.make_preview_matrices()
        plan = compile_plan(form, ltv=["plant"])      # (the sweep kernel does not mind: no cost or limit reads it)
        with pytest.raises(ValueError, match=bad):
            rollout_rows(plan)
    # a plan without a dynamics compiled as ltv has no rollout at all
    plain = compile_plan(sc.build(api, rng, shape))
    with pytest.raises(ValueError, match="preview_rows"):
        rollout_rows(plain)


def test_compile_refuses_another_plan_and_mismatched_sizes(cpu_api):
    """mpcasm_ltv_rollout_compile, host only: no device is touched."""
    rng = np.random.default_rng(7)
    shape = rc.shape_of("desc")
    form = sc.build(cpu_api, rng, shape)
    plan, plain = compile_plan(form, ltv=["plant"]), compile_plan(form)
    recs, cvec = rollout_rows(plan)
    sizes = rollout_sizes(plan)
    assert engine.rollout_table(plan, recs, cvec, sizes).size == 12 + recs.size + 2 * cvec.size

    def refused(*args):
        with pytest.raises(capi.MpcasmError) as err:
            engine.rollout_table(*args)
        return err.value.status

    assert refused(plain, recs, cvec, sizes) == capi.ERR_ARG                 # not a sweep plan
    for i in range(7):                                                        # sizes that are not the plan's
        other = sizes.copy()
        other[i] += 1
        assert refused(plan, recs, cvec, other) == capi.ERR_ARG, i
    bad = recs.copy()
    bad[-1, 2] -= 1                                                           # a row left out
    assert refused(plan, bad, cvec, sizes) == capi.ERR_ARG
    bad = recs.copy()
    bad[3, 1] += 1                                                            # rows out of order / twice
    assert refused(plan, bad, cvec, sizes) == capi.ERR_ARG
    state = int(np.flatnonzero(recs[:, 0] == ROLL_STATE)[0])
    for col, value in ((0, 7), (3, shape.axes), (4, shape.N), (5, 2), (6, len(cvec))):
        bad = recs.copy()
        bad[state, col] = value                                               # kind, axis, step, stride, c
        assert refused(plan, bad, cvec, sizes) == capi.ERR_ARG, col
    copy = int(np.flatnonzero(recs[:, 0] == ROLL_OPTIM)[0])
    bad = recs.copy()
    bad[copy, 4] = plan.no - 1                                                # a column behind the unknowns
    assert refused(plan, bad, cvec, sizes) == capi.ERR_ARG
    nan = cvec.copy()
    nan[0, 0] = np.nan
    assert refused(plan, recs, nan, sizes) == capi.ERR_ARG
    # the two-call protocol: a capacity too small is refused, nothing written
    import ctypes

    itab, dtab, words = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab), ctypes.c_int64()
    small = np.full(4, -1, dtype=np.int32)
    assert capi.load().mpcasm_ltv_rollout_compile(
        itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size, sizes.ctypes.data, recs.ctypes.data, len(recs),
        cvec.ctypes.data, len(cvec), small.ctypes.data, small.size, ctypes.byref(words)) == capi.ERR_ARG
    assert (small == -1).all() and words.value == 12 + recs.size + 2 * cvec.size


def _shared_bytes(table_words):
    """The shared part of a workgroup's LDS (roll_lds): the table's body behind its 12-word header, in doubles
    rounded up to even, then RO_GROUP_MAX = 8 ints of rowof."""
    doubles = (table_words - 12 + 1) // 2
    return 8 * (doubles + (doubles & 1) + 4)


def _split(group, count):
    """The live instances of every workgroup of ``count`` instances in groups of ``group``."""
    return tuple(min(group, count - first) for first in range(0, count, group))


@pytest.mark.parametrize("name", rc.GPU_SHAPES)
def test_the_launch_geometry_of_the_gpu_shapes(cpu_api, name):
    """mpcasm_ltv_rollout_info, host only, on the compiled plan: the group, the LDS and the grid of rc.INFO."""
    form, plan = sc.compile_case(cpu_api, np.random.default_rng(31), rc.shape_of(name))
    words = engine.rollout_table(plan).size
    group, per, advance_group = rc.INFO[name]
    shared = _shared_bytes(words)
    assert shared == rc.INFO_SHARED.get(name, shared)
    assert engine.rollout_info(plan, True, 64) == (group, shared + group * per, -(-64 // group))
    for count in (1, 3):
        g = min(group, count)
        assert engine.rollout_info(plan, True, count, words) == (g, shared + g * per, -(-count // g)), count
    # the advance stages one step and no optim: 80 to 528 bytes an instance, so 8 of every shape share a workgroup
    g, lds, workgroups = engine.rollout_info(plan, False, 64)
    assert (g, workgroups) == (advance_group, 8) and (lds - shared) % g == 0 and 80 <= (lds - shared) // g <= 528
    for count in (1, 3):
        assert engine.rollout_info(plan, False, count)[::2] == (count, 1)


def test_the_geometry_cases_are_what_they_claim(cpu_api):
    """The premises of test_gpu_ltv_rollout_variants.py on the compiled plans: every split of rc.GEOMETRY and
    rc.ADVANCE is the entry's answer, the sixteen nm shapes compile with the sizes the cases rely on."""
    plans = {}

    def plan_of(name):
        if name not in plans:
            plans[name] = sc.compile_case(cpu_api, np.random.default_rng(31), rc.shape_of(name))[1]
        return plans[name]

    for name, batch, counts in rc.GEOMETRY:
        group = rc.INFO[name][0]
        assert max(counts) == batch
        for count, split in counts.items():
            assert split == _split(group, count), (name, count)
            assert engine.rollout_info(plan_of(name), True, count)[::2] == (max(split), len(split)), (name, count)
    seen = {split for _, _, counts in rc.GEOMETRY for split in counts.values()}
    assert any(len(s) > 1 and s[1] > 1 for s in seen)                     # a second workgroup of more than one
    assert any(s[0] == 8 for s in seen)                                   # a full workgroup of 8
    assert any(len(s) > 2 and s[0] > 2 and s[-1] < s[0] for s in seen)    # a partial one behind full ones, group > 2
    name, batch, rows, counts = rc.ADVANCE
    for count, split in counts.items():
        assert split == _split(8, count)
        assert engine.rollout_info(plan_of(name), False, count)[::2] == (8, len(split))
    # the start on an odd double: pmrows = 5 is odd (and no = 1, a plant of one double), 402 even
    assert plan_of("one-1-1-1").pmrows == 5 and plan_of("one-1-1-1").no == 1 and plan_of("lipm-33").pmrows == 402
    runs = {(name, batch, count) for name, batch, counts in rc.GEOMETRY for count in counts}
    assert set(rc.ODD_START) <= runs and rc.MISSING[:3] in runs             # (the aligned runs they are compared with)
    name, batch, count, rows, missing = rc.MISSING                          # the second workgroup's first instance, one
    assert missing == (8, 9, 16) and rc.GEOMETRY[0][2][count] == (8, 8, 1) and rows > batch     # inside it, the last
    # every roll_chain<NS, MS>: the sizes, a row table, groups of 8 and 3 at 11 instances, rows and advance
    sizes = set()
    for name in rc.NM_SHAPES:
        shape, plan = rc.shape_of(name), plan_of(name)
        sw = plan.sweep
        assert (sw["n"], sw["m"], sw["N"], sw["axes"].shape[0]) == (shape.n, shape.m, 5, 2)
        assert (plan.no, plan.ng) == (10 * shape.m, 2 * shape.n) and 42 <= plan.pmrows <= 108
        assert [int(sw["axes"][a, 1]) for a in range(2)] == [0, 5 * shape.m]       # (the second axis: ucol != 0)
        sizes.add((shape.n, shape.m))
        for rows in (True, False):
            assert engine.rollout_info(plan, rows, rc.NM_BATCH)[::2] == (8, 2)
    assert sizes == {(n, m) for n in range(1, 5) for m in range(1, 5)}
    assert {plan_of(n).pmrows for n in rc.NM_SHAPES} >= {42, 108}


def test_the_geometry_query_refuses_what_the_launch_refuses(cpu_api):
    import ctypes

    rng = np.random.default_rng(7)
    form = sc.build(cpu_api, rng, rc.shape_of("desc"))
    plan, plain = compile_plan(form, ltv=["plant"]), compile_plan(form)
    words = engine.rollout_table(plan).size

    def refused(*args):
        with pytest.raises(capi.MpcasmError) as err:
            engine.rollout_info(*args)
        return err.value.status

    assert refused(plain, True, 4, words) == capi.ERR_ARG                   # no dynamics compiled as ltv
    assert refused(plan, True, -1, words) == capi.ERR_ARG
    assert refused(plan, True, 4, 11) == capi.ERR_ARG                       # shorter than a table's header
    assert refused(plan, True, 4, 12 + 4096 + 1) == capi.ERR_ARG            # longer than any table
    assert engine.rollout_info(plan, True, 0, words) == (0, 0, 0)
    itab, dtab = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab)
    group, lds, groups = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
    out = (ctypes.byref(group), ctypes.byref(lds), ctypes.byref(groups))
    call = capi.load().mpcasm_ltv_rollout_info
    tables = (itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size)
    assert call(*tables, words, 2, 4, *out) == capi.ERR_ARG                 # rows_out: 0 or 1
    assert call(None, 0, None, 0, words, 1, 4, *out) == capi.ERR_ARG
    for i in range(3):
        assert call(*tables, words, 1, 4, *(None if j == i else o for j, o in enumerate(out))) == capi.ERR_ARG
    assert call(*tables, words, 1, 4, *out) == capi.OK and group.value >= 1


def test_the_restated_loop_exercises_both_branches(cpu_api):
    """The inputs of test_gpu_ltv_loop.py on the CPU: the oracle's assembly on the windowed per-step plant,
    osqp_restatement.solve, x_1 -- instance 1 primal infeasible (held) and the others solved, at every tick, no
    verdict near a tie."""
    form, A, B, given = rc.loop_inputs(cpu_api)
    plan = compile_plan(form, ltv=["LIP"])
    status, trail, margin = rc.restated_loop(cpu_api, plan, form, A, B, given)
    for b, want in rc.LOOP_STATUS.items():
        assert (status[:, b] == want).all(), (b, status[:, b])
    assert margin > 1e-6, margin
    held = [b for b, s in rc.LOOP_STATUS.items() if not rc.applies(s, "hold")]
    for b in range(rc.LOOP_BATCH):
        moved = [not np.array_equal(trail[t + 1, b], trail[t, b]) for t in range(rc.LOOP_TICKS)]
        assert all(moved) != (b in held) and any(moved) != (b in held)
    assert np.isfinite(trail).all()
