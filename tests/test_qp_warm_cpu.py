"""CPU: the host side of the loops' warm start -- the shift map on every place of the biped's step cycle, the
closed warm loop of one walker against the closed cold loop (both on the restatements), and the two entries of
the library as far as they answer without a device."""
import ctypes

import numpy as np
import pytest

import osqp_restatement as rs
import warm_restatement as wr
from fleet_loop_reference import host_loop
from mpcasm import capi, problems
from mpcasm.warm import horizon_of, limit_rows, shift_map


def forms_of_the_cycle(api, conf):
    """The biped as updated at each of the ``2 * step_samples + 1`` consecutive ticks of a walker from phase 0:
    ``(formulation, step count)`` per tick."""
    clock = problems.StepClock(conf.step_samples, conf.num_steps)
    out = []
    for _ in range(2 * conf.step_samples + 1):
        form = problems.biped(api, conf)
        form.update(step_times=np.array(clock.step_times), step_count=int(clock.step_count))
        out.append((form, clock.step_count))
        clock.tick()
    return out


def test_shift_map_on_every_place_of_the_biped_cycle(cpu_api):
    conf = problems.BipedConfig(step_samples=8)
    N = conf.horizon_lenght
    cycle = forms_of_the_cycle(cpu_api, conf)
    seen = set()
    for key in range(1, len(cycle)):
        (prev, c0), (new, c1) = cycle[key - 1], cycle[key]
        assert horizon_of(new) == N
        col, row = shift_map(prev, new, c1 != c0)
        assert col.dtype == row.dtype == np.int32
        assert col.shape == (new.optim_len,) and row.shape == (sum(limit_rows(new)),)
        assert col.min() >= -1 and col.max() < prev.optim_len
        assert row.min() >= -1 and row.max() < sum(limit_rows(prev))
        assert (col >= 0).any() and (row >= 0).any(), key
        for axis in ("_x", "_y"):           # the jerk: k -> k + 1, the last entry repeated
            jerk, old = new.optim_ID["CoM_dddot" + axis], prev.optim_ID["CoM_dddot" + axis]
            assert list(col[jerk.start:jerk.stop]) == [old.start + min(k + 1, N - 1) for k in range(N)]
        steps = {axis: list(col[new.optim_ID["Ds" + axis].start:new.optim_ID["Ds" + axis].stop])
                 for axis in ("_x", "_y")}
        change = (prev.optim_len, new.optim_len)
        seen.add(change)
        if change == (34, 36):              # a step enters the preview: the first is the old one, the second is new
            assert c1 == c0 and steps == {"_x": [16, -1], "_y": [33, -1]}
            # the stepping area's facets grew from 1 to 2 rows each: no counterpart; the 4 x 16 rows per sample
            # shifted inside their limit; the 4 terminal rows copied
            assert list(row[:8]) == [-1] * 8
            assert list(row[8:24]) == list(range(5, 20)) + [19]
            assert list(row[72:]) == [68, 69, 70, 71]
        elif change == (36, 34):            # the first step was taken: the one left was the second
            assert c1 == c0 + 1 and steps == {"_x": [17], "_y": [35]}
            assert list(row[:4]) == [-1] * 4
            assert list(row[4:20]) == list(range(9, 24)) + [23]
            assert list(row[68:]) == [72, 73, 74, 75]
        elif change == (36, 36):
            assert c1 == c0 and steps == {"_x": [16, 17], "_y": [34, 35]}
            assert list(row[:8]) == list(range(8))
        else:
            raise AssertionError(change)
    assert seen == {(34, 36), (36, 34), (36, 36)}


def test_shift_map_without_a_counterpart_gives_minus_one(cpu_api):
    conf = problems.BipedConfig(step_samples=8)
    (prev, _), (new, _) = forms_of_the_cycle(cpu_api, conf)[:2]
    import types
    renamed = types.SimpleNamespace(optim_ID={"other": range(0, 34)}, optim_len=34, optim_variables=["other"],
                                    domain={"other": 34})
    col, row = shift_map(renamed, new, False, prev_rows=[3], new_rows=limit_rows(new))
    assert (col == -1).all() and (row == -1).all()
    # the loop with one structure: every unknown and every row of a per-sample limit shifted, the rest copied
    ltv = problems.lipm_ltv(cpu_api, N=12)
    rows = [12, 12, 12, 12, 1, 1, 1, 1]
    col, row = shift_map(ltv, ltv, False, horizon=12, prev_rows=rows, new_rows=rows)
    assert list(col) == [min(k + 1, 11) for k in range(12)] + [12 + min(k + 1, 11) for k in range(12)]
    assert list(row[:12]) == list(range(1, 12)) + [11] and list(row[48:]) == [48, 49, 50, 51]


def test_the_closed_warm_loop_against_the_closed_cold_loop(cpu_api):
    """problems.biped, step_samples = 8, phases 0 and 3, 20 ticks from rest, both loops closed on their own
    solutions (the restatements).  Every tick that starts warm ends SOLVED, and over ticks 1-19 the warm loop
    takes at most half of the cold loop's iterations -- the condition; the ratio itself is what the run prints
    (measured: 1 450 against 6 875 iterations, 0.21 of cold, over both phases)."""
    conf = problems.BipedConfig(step_samples=8)
    total_warm = total_cold = 0
    for phase in (0, 3):
        form = problems.biped(cpu_api, conf)
        warm = wr.warm_loop(form, conf, phase, 20)
        _st, cold_iters, _tr, _m = host_loop(problems.biped(cpu_api, conf), conf, phase, 20)
        assert warm[0].warm == 0
        for t, tick in enumerate(warm):
            print("phase %d tick %2d  cold %4d  warm %4d  (%s, rho %.4g)"
                  % (phase, t, cold_iters[t], tick.sol.iters, "warm" if tick.warm else "cold", tick.start[3]))
            if tick.warm:
                assert tick.sol.status == rs.SOLVED, (phase, t, tick.sol.status)
            if t >= 1:
                assert tick.warm == int(warm[t - 1].sol.status == rs.SOLVED), (phase, t)
        total_warm += sum(tick.sol.iters for tick in warm[1:])
        total_cold += int(cold_iters[1:].sum())
    print("ticks 1-19, both phases: warm %d iterations, cold %d, ratio %.3f"
          % (total_warm, total_cold, total_warm / total_cold))
    assert 2 * total_warm <= total_cold, (total_warm, total_cold)


def test_the_restated_rule_mixes_warm_and_cold():
    rng = np.random.default_rng(2)
    B, no, nc, R = 6, 5, 3, 9
    G, h = rng.normal(size=(B, nc, no)), rng.normal(size=(B, nc))
    SX, SY = rng.normal(size=(R, 7)), rng.normal(size=(R, 4))
    SR = np.full(R, 0.3)
    SM = np.tile(np.array([[rs.SOLVED, 4]], dtype=np.int32), (R, 1))
    index = np.array([8, 1, 5, 2, 7, 0])
    SM[1, 1] = 3                  # another tag
    SM[5, 0] = rs.MAX_ITER        # a status outside the mask
    SR[2] = 0.0
    SX[7, 6] = np.nan             # gathered: cold
    SX[8, 5] = np.nan             # not gathered: stays warm
    col, row = np.array([1, 0, -1, 6, 9]), np.array([3, -5, 0])
    out = wr.warm_start(G, h, SX, SY, SR, SM, index, col, row, 4, wr.qp_bit(rs.SOLVED))
    assert [s.warm for s in out] == [1, 0, 0, 0, 0, 1]
    assert np.array_equal(out[0].x, [SX[8, 1], SX[8, 0], 0.0, SX[8, 6], 0.0])
    assert np.array_equal(out[0].y, [SY[8, 3], 0.0, SY[8, 0]]) and out[0].rho == 0.3
    assert np.array_equal(out[1].z, np.minimum(0.0, h[1])) and out[1].rho == wr.RHO_COLD
    assert np.all(np.abs(out[5].z.astype(wr.LD) - np.minimum(out[5].gx_ld, h[5])) <= 7 * 2.0 ** -53 * out[5].mag)


# ---- the library, as far as it answers without a device -----------------------------------------------------
def test_the_entries_decide_their_arguments_without_a_device():
    lib = capi.load()
    one = ctypes.c_void_p(16)      # (never dereferenced: every call below is decided on the host)
    store = lambda rows=4, sno=36, snc=76: [one, one, one, one, rows, sno, snc]

    def call_store(no, nc, count, y=one, **kw):
        return lib.mpcasm_qp_warm_store(no, nc, one, y, one, one, 3, *store(**kw), None, count, None)

    def call_start(no, nc, count, nulls=False, rho_cold=0.1, **kw):
        p = None if nulls else one
        return lib.mpcasm_qp_warm_start(no, nc, p, p, *store(**kw), None, one, p, 2, 2, rho_cold, one, p, p, one,
                                        one, count, None)

    assert call_store(36, 76, 0) == capi.OK and call_start(36, 76, 0) == capi.OK          # count = 0
    assert call_start(7, 0, 0, nulls=True) == capi.OK                                   # nc = 0 with the NULLs
    assert call_store(7, 0, 0, y=None) == capi.OK
    for bad in (dict(no=36, nc=76, count=-1), dict(no=0, nc=76, count=0), dict(no=36, nc=-1, count=0),
                dict(no=36, nc=76, count=0, sno=0), dict(no=36, nc=76, count=0, snc=-1),
                dict(no=513, nc=76, count=0, sno=513), dict(no=36, nc=2049, count=0, snc=2049),
                dict(no=36, nc=76, count=0, rows=-1)):
        assert call_store(**bad) == capi.ERR_ARG, bad
        assert call_start(**bad) == capi.ERR_ARG, bad
    assert call_store(36, 76, 0, sno=34) == capi.ERR_ARG        # the store is narrower than the launch
    assert call_start(36, 76, 0, sno=34) == capi.OK             # ... which a start may well be
    assert call_start(36, 76, 0, rho_cold=float("nan")) == capi.ERR_ARG
    # null operands, decided before any device call (count > 0, no device here or there)
    assert call_store(36, 76, 2, y=None) == capi.ERR_ARG
    assert call_start(36, 76, 2, nulls=True) == capi.ERR_ARG
    assert call_store(36, 76, 5, rows=4) == capi.ERR_ARG        # no index and fewer rows than instances


def test_the_header_symbols_are_bound_and_the_strings_unchanged():
    lib = capi.load()
    for name in ("mpcasm_qp_warm_store", "mpcasm_qp_warm_start"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.mpcasm_abi_version() == 1004
    assert lib.mpcasm_status_string(0) == b"ok"
    assert lib.mpcasm_status_string(-1) == lib.mpcasm_status_string(capi.ERR_ARG)
    assert lib.mpcasm_status_string(-2) == b"malformed plan tables"
    assert set(capi.STATUS) == {0, -1, -2, -3, -4, -5}
