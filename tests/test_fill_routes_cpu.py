"""CPU: the kernel of the horizon fill a launch runs on (csrc/fill.hip, fill_choose) as the library itself reports
it -- mpcasm_fill_route, the very function launch_fill_su decides with.  Every case of the family in fill_cases.py
is pinned to its route, at both alignments of the outputs; the decision is held, shape by shape over a declared
grid, to a transcription of the conditions as they stood before fill_choose was split from the launch (the pin of
"no launch changed"); the family is held to reach everything that grid reaches; and the bound the GPU test applies
(helpers.kappa) is shown to leave room for a correct fp64 computation on the very inputs that test uses: the fp64
oracle stays within HALF of it."""
import ctypes
import os

import numpy as np
import pytest

import fill_cases as fc
from fill_cases import GENERIC, LTI, LTV, LTV_BLOCK, LTV_ROW, LTV_WAVE, PAD, QUAD, TINY, WHOLE
from helpers import assert_componentwise
from mpcasm import capi, engine

IDS = [c.name for c in fc.CASES]
LIMIT = fc.LIMIT
WAVE_ALL = 99        # fill_ltv_wave_kernel<true> of the earlier launch: see test_no_launch_changed...


def test_the_tuning_variable_is_unset():
    """MPCASM_FILL_MIN_WAVES is read once per process by the route and the launch alike; the pinned routes are
    those of its default."""
    assert "MPCASM_FILL_MIN_WAVES" not in os.environ


def test_constants_are_the_library_s():
    assert (QUAD, TINY, LTI, LTV_ROW, LTV_BLOCK, LTV_WAVE, LTV) == (
        capi.FILL_QUAD, capi.FILL_TINY, capi.FILL_LTI, capi.FILL_LTV_ROW, capi.FILL_LTV_BLOCK, capi.FILL_LTV_WAVE,
        capi.FILL_LTV)
    assert (GENERIC, PAD, WHOLE) == (capi.FILL_GENERIC, capi.FILL_PAD, capi.FILL_WHOLE_LINES)


def _route(batch, N, n, m, ltv, aligned, out=(ctypes.c_int32 * 8)()):
    rc = capi.load().mpcasm_fill_route(batch, N, n, m, ltv, aligned, out)
    if rc == capi.ERR_LIMIT:
        assert list(out) == [0] * 8
        return LIMIT
    assert rc == 0, rc
    return tuple(out)


def expected_grid(case, route):
    if route.kernel == QUAD:
        return -(-case.batch // route.spw)
    if route.kernel == TINY:
        return -(-case.batch // (4 * route.spw))
    if route.arg == 64 or route.kernel == LTV_WAVE:
        return -(-case.batch // 4)
    return case.batch


@pytest.mark.parametrize("case", fc.CASES, ids=IDS)
def test_every_case_takes_its_route(case):
    if case.route is LIMIT:
        for aligned in (True, False):
            with pytest.raises(capi.MpcasmError) as refusal:
                engine.fill_route(case.batch, case.N, case.n, case.m, case.ltv, aligned)
            assert refusal.value.status == capi.ERR_LIMIT
        return
    for aligned, route in ((True, case.route), (False, case.off8 or case.route)):
        out = engine.fill_route(case.batch, case.N, case.n, case.m, case.ltv, aligned)
        assert fc.Route(*out[:5]) == route, (aligned, out)
        assert out.grid == expected_grid(case, route)
        assert 0 < out.lds <= 160 * 1024 and out.whole_lds == (out.lds > 64 * 1024)
    # what is special about a shape is said by its name
    if case.name.endswith(("-N1", "-N2")):
        assert case.N == int(case.name[-1])
    if "-spw" in case.name:
        assert case.route.spw == int(case.name.split("-spw")[1]) and case.batch % case.route.spw != 0
    if "-lds" in case.name and "lds40" not in case.name:
        assert engine.fill_route(case.batch, case.N, case.n, case.m, case.ltv, True).whole_lds == 1


# --------------------------------------------------------------------------------------------------------------
# The decision as launch_fill_su took it before fill_choose existed, condition by condition (the LDS sizes are
# the *_lds_doubles of fill.hip): (kernel, arg, flags, spw, lshift, grid, LDS bytes, whole LDS).
# --------------------------------------------------------------------------------------------------------------
def _ev(x):
    return (x + 1) & ~1


GRANTED = 156 * 1024     # the dynamic LDS a workgroup is granted; the earlier launch tried up to the CU's 160 KB


def earlier_launch(batch, N, n, m, ltv, aligned, lds_max=GRANTED):

    def answer(kernel, arg, flags, spw, lshift, grid, lds):
        return (kernel, arg, flags, spw, lshift, grid, lds, int(lds > 64 * 1024))

    pairs = (N * n) % 2 == 0 and aligned
    if not ltv and n <= 4 and m + n <= 16 and pairs and (N * n * n) % 2 == 0:
        def quad(s):
            return (s * (N * n * n + m * 2 * N * n) + 64) * 8
        spw = 16 // (m + n)
        while spw > 1 and quad(spw) > 40 * 1024:
            spw -= 1
        while spw > 1 and (batch + spw - 1) // spw < 8192:
            spw -= 1
        if quad(spw) <= lds_max:
            lshift = 0
            while lshift < 6 and (1 << lshift) < (N * n) // 2:
                lshift += 1
            return answer(QUAD, n, WHOLE if (N * n) % 16 == 0 else 0, spw, lshift, (batch + spw - 1) // spw, quad(spw))
    if ltv and n <= 4 and n * m <= 64 and pairs:
        lq = 64 // n
        passes = (n + m * N + lq - 1) // lq
        row = (2 * _ev(passes * lq * n + 2) + _ev(N * n * n) + _ev(N * n * m)) * 8
        if row <= 64 * 1024:
            return answer(LTV_ROW, n, 0, 0, 0, batch, row)
    if not ltv:
        per = (_ev(m * N * n) + 2 * _ev(n * (m + n)) + _ev(n * n)) * 8
        xsz = n * (m + n)
        small = xsz <= 256 and per * 4 <= 48 * 1024
        spw = 64 // xsz if xsz <= 32 else 0
        while spw > 2 and (batch + 4 * spw - 1) // (4 * spw) < 512:
            spw -= 1
        tiny = (per + _ev(N * n * n) * 8) * 4 * (spw if spw > 0 else 1)
        if spw >= 2 and tiny <= 64 * 1024:
            return answer(TINY, 0, 0, spw, 0, (batch + 4 * spw - 1) // (4 * spw), tiny)
        if small:
            return answer(LTI, 64, 0, 0, 0, (batch + 3) // 4, per * 4)
        if per > lds_max:
            return LIMIT
        if xsz <= 1024:
            padded = per + m * N * n * 8
            if pairs and padded <= 78 * 1024:
                return answer(LTI, 256, PAD, 0, 0, batch, padded)
            return answer(LTI, 256, 0, 0, 0, batch, per)
        return answer(LTI, 256, GENERIC, 0, 0, batch, per)
    per = (2 * _ev(m * N * n) + 3 * _ev(n * n) + _ev(n * m)) * 8
    small = n <= 64 and per * 4 <= 64 * 1024 and N * n <= 1024
    step = _ev(n * n) + _ev(n * m)
    wper = (2 * _ev(m * N * n) + 2 * _ev(n * n) + 2 * step) * 8 * 4
    wall = (2 * _ev(m * N * n) + 2 * _ev(n * n) + N * step) * 8 * 4
    bper = (2 * _ev(m * N * n) + 2 * _ev(n * n) + N * step) * 8
    if n <= 256 and bper <= 20 * 1024:
        return answer(LTV_BLOCK, n if n in (2, 3, 4) else 0, 0, 0, 0, batch, bper)
    if n * n <= 128 and n * m <= 64 and wall <= 80 * 1024 and batch < 8192:
        return answer(WAVE_ALL, 0, 0, 0, 0, (batch + 3) // 4, wall)
    if n * n <= 128 and n * m <= 64 and wper <= 64 * 1024:
        return answer(LTV_WAVE, 0, 0, 0, 0, (batch + 3) // 4, wper)
    if small:
        return answer(LTV, 64, 0, 0, 0, (batch + 3) // 4, per * 4)
    if n > 256 or per > lds_max:
        return LIMIT
    return answer(LTV, 256, 0, 0, 0, batch, per)


# the declared grid.  Beyond four states and 32 lanes of recurrence the batch only sets the number of workgroups.
GRID_BATCH = (1, 3, 67, 6139, 8195, 10223, 16400, 33000, 50000, 57400, 65600)
GRID_BATCH_WIDE = (1, 3, 67)
GRID_STATES = tuple(range(1, 13)) + (16, 17, 20, 24, 25, 32, 33, 40, 48, 64, 65, 70, 128, 256, 257)
GRID_INPUTS = tuple(range(1, 17)) + (18, 20, 24, 30, 33)
GRID_HORIZON = tuple(range(1, 41)) + (48, 53, 54, 64, 66, 73, 85, 86, 100, 101, 128, 130, 170, 200, 212, 300, 400)


def grid():
    for ltv in (0, 1):
        for aligned in (1, 0):
            for n in GRID_STATES:
                for m in GRID_INPUTS:
                    by_batch = not ltv and (n <= 4 or n * (m + n) <= 32)
                    for batch in GRID_BATCH if by_batch else GRID_BATCH_WIDE:
                        for N in GRID_HORIZON:
                            yield batch, N, n, m, ltv, aligned


def signatures(answer, N, n):
    """What of an answer the family has to reach: the instantiation, with its dynamic LDS on either side of 64 KB;
    on the quad kernel every (NS, lshift), whole lines or not, every spw, the kinds of rows; on the tiny kernel
    spw = 2, a middle value (3 .. 8) and a large one (24 or more: 32 is the most any shape allows)."""
    kernel, arg, flags, spw, lshift, _, _, whole_lds = answer
    sigs = {("instantiation", kernel, arg, flags & (GENERIC | PAD)),
            ("whole-lds", kernel, 0 if kernel == QUAD else arg, flags & (GENERIC | PAD), whole_lds)}
    if kernel == QUAD:
        rl2 = N * n // 2
        R = 64 >> lshift
        sigs |= {("quad-lshift", arg, lshift), ("quad-whole-lines", flags & WHOLE), ("quad-spw", spw),
                 ("quad-rows", "long" if rl2 > 64 else "L64" if rl2 > 32 else
                  "short" if N < R else "tail" if N % R else "multiple")}
        if rl2 <= 64 and N // R >= 4:
            sigs.add(("quad-rows", "unrolled"))
    if kernel == TINY:
        sigs.add(("tiny-spw", "2" if spw == 2 else "middle" if spw <= 8 else "large" if spw >= 24 else "other"))
    sigs.discard(("tiny-spw", "other"))
    return sigs


INSTANTIATIONS = (
    {("instantiation", QUAD, ns, 0) for ns in (1, 2, 3, 4)} | {("instantiation", TINY, 0, 0)} |
    {("instantiation", LTI, 64, 0), ("instantiation", LTI, 256, PAD), ("instantiation", LTI, 256, 0),
     ("instantiation", LTI, 256, GENERIC)} |
    {("instantiation", LTV_ROW, ns, 0) for ns in (1, 2, 3, 4)} |
    {("instantiation", LTV_BLOCK, ns, 0) for ns in (0, 2, 3, 4)} |
    {("instantiation", LTV_WAVE, 0, 0), ("instantiation", LTV, 64, 0), ("instantiation", LTV, 256, 0)})


def test_no_launch_changed_and_the_family_reaches_what_the_grid_reaches():
    """One walk over the grid: fill_choose answers what the earlier launch did, shape by shape; the launch's
    branch for fill_ltv_wave_kernel<true> (every step's matrices in LDS, "ALL") is met by NO shape -- its
    condition, four times the block kernel's LDS within 80 KB, is the condition under which the block kernel in
    front of it has taken the launch -- which is why that instantiation is gone; every signature the grid meets is
    met by a case, and every instantiation is met by the grid."""
    met, limits, count, over_granted = set(), set(), 0, 0
    out = (ctypes.c_int32 * 8)()
    for shape in grid():
        count += 1
        was = earlier_launch(*shape)
        assert _route(*shape, out) == was, shape
        # the one difference from the launch as it was: what it sent off with more LDS than a workgroup is granted
        # (the runtime refused that launch) goes to the next kernel that takes the shape, or is refused
        before = earlier_launch(*shape, lds_max=160 * 1024)
        if before != was:
            assert before is not LIMIT and GRANTED < before[6] <= 160 * 1024, shape
            over_granted += 1
        if was is LIMIT:
            limits.add(shape[4])
        else:
            assert was[0] != WAVE_ALL, shape
            met |= signatures(was, shape[1], shape[2])
    assert count > 300000 and limits == {0, 1} and 0 < over_granted < count // 200
    assert {s for s in met if s[0] == "instantiation"} == INSTANTIATIONS
    reached = set()
    for case in fc.RUN:
        for aligned in (1, 0):
            reached |= signatures(earlier_launch(case.batch, case.N, case.n, case.m, case.ltv, aligned), case.N, case.n)
    missing = met - reached
    assert not missing, "no case reaches %s" % sorted(missing, key=str)
    assert reached <= met, "outside the grid: %s" % sorted(reached - met, key=str)


def test_the_axes_the_route_does_not_name():
    """Batches around a workgroup of four systems; ragged wavefronts of the tiny kernel; N = 1 and N = 2; the block
    kernel's <0> at n = 1 and n >= 5; the limit that lowers spw."""
    by_kernel = {}
    for c in fc.RUN:
        by_kernel.setdefault((c.route.kernel, c.route.arg), []).append(c)
    for key in ((LTI, 64), (LTV_WAVE, 0), (LTV, 64)):
        assert {1, 3, 4, 5, 67} <= {c.batch for c in by_kernel[key]}, key
    assert {c.n for c in by_kernel[(LTV_BLOCK, 0)]} >= {1, 5}
    for c in fc.RUN:
        if c.route.kernel == TINY and c.batch > 5:       # the last workgroup and its last wavefront partly filled
            per_block = 4 * c.route.spw
            assert 0 < c.batch % per_block < per_block - c.route.spw and (c.batch % per_block) % c.route.spw
    assert {64 % (c.n * (c.m + c.n)) != 0 for c in by_kernel[(TINY, 0)]} == {True, False}
    for ltv in (0, 1):
        assert {1, 2} <= {c.N for c in fc.RUN if c.ltv == ltv}
    assert max(c.m + c.n for c in fc.RUN if c.route.kernel == QUAD) == 16
    assert {c.m == 1 for c in fc.RUN if c.route.kernel == QUAD} == {True, False}
    # 40 KB: two systems of the shape would take more, and the batch alone would have allowed two
    c = fc.BY_NAME["quad4-N54-m4-lds40"]
    assert (2 * (c.N * c.n * c.n + 2 * c.m * c.N * c.n) + 64) * 8 > 40 * 1024 and 16 // (c.m + c.n) == 2
    assert (c.batch + 1) // 2 >= 8192 and c.route.spw == 1
    assert fc.BY_NAME["quad4-m12"].route.spw == 1 and fc.BY_NAME["quad1-spw8"].route.spw == 16 // 2


@pytest.mark.parametrize("case", fc.RUN, ids=[c.name for c in fc.RUN])
def test_the_bound_has_room_for_fp64(case):
    """Not a measurement of the kernel: the oracle's recurrence in fp64 on the GPU test's own inputs stays within
    half of kappa(N, n) of its run in long double, so a kernel beyond kappa is at fault, not the bound.  Every
    instance: those of a batch up to 67 one by one, a larger batch at once by the recurrence over the batch (and
    the instances the GPU test holds to the oracle itself one by one as well); where plants repeat, every plant."""
    A, B = fc.inputs(case)
    ref = fc.oracle(case)
    assert sorted(ref) == (list(range(case.batch)) if case.batch <= fc.SMALL_BATCH else fc.sample(case))
    worst = 0.0
    for b in ref:
        mine = fc.oracle_pair(case, A[b], B[b], dtype=float)
        for key in "SU":
            worst = max(worst, assert_componentwise(mine[key][0], *ref[b][key], fc.kappa(case) // 2,
                                                    "%s %s[%d]" % (case.name, key, b)))
    if case.batch > fc.SMALL_BATCH and case.name not in fc.DISTINCT:
        every = fc.batch_reference(case)
        for key, mine in zip("SU", fc.recurrence(A, B, case.N, dtype=float)):
            worst = max(worst, assert_componentwise(mine, *every[key], fc.kappa(case) // 2,
                                                    "%s %s (whole batch)" % (case.name, key)))
    print("componentwise %-24s fp64 oracle worst %8.3g u M   kappa %d" % (case.name, worst, fc.kappa(case)))


def test_the_batch_reference_is_the_oracle_s():
    """The recurrence vectorised over the batch (what the large batches are checked against) gives what the
    oracle gives, instance by instance, to the last bit of long double on most and within two units on all."""
    case = fc.BY_NAME["quad2-m2-spw4"]
    ref, per = fc.batch_reference(case), fc.oracle(case)
    for b in fc.sample(case):
        for key in "SU":
            for mine, theirs in zip(ref[key], per[b][key]):
                assert np.all(np.abs(mine[b] - theirs) <= 2 * np.finfo(fc.LD).eps * np.abs(theirs))
    assert not ref["U"][1][:, :, 0, 1:].any()      # above the diagonal: M = 0


def test_query_checks_its_arguments():
    lib = capi.load()
    out = (ctypes.c_int32 * 8)(*([7] * 8))
    assert lib.mpcasm_fill_route(8, 16, 3, 1, 0, 1, out) == 0 and out[0] == QUAD and out[1] == 3
    assert lib.mpcasm_fill_route(8, 16, 3, 1, 0, 1, None) == -1
    for bad in ((0, 16, 3, 1, 0, 1), (8, 0, 3, 1, 0, 1), (8, 16, 0, 1, 0, 1), (8, 16, 3, 0, 0, 1), (8, 16, 3, 1, 2, 1),
                (8, 16, 3, 1, 0, 2)):
        out = (ctypes.c_int32 * 8)(*([7] * 8))
        assert lib.mpcasm_fill_route(*bad, out) == -1 and list(out) == [0] * 8
    out = (ctypes.c_int32 * 8)(*([7] * 8))
    assert lib.mpcasm_fill_route(3, 1, 70, 33, 0, 1, out) == capi.ERR_LIMIT and list(out) == [0] * 8
