"""CPU: the kernel family mpcasm_assemble runs a launch on, as the library itself reports it -- mpcasm_assemble_route,
the very function (csrc/dispatch.hip assemble_route) the launch, mpcasm_plan_prepare and mpcasm_tiled_route decide
with.  Plans of the existing families are crossed with MPCASM_OPT_PATH 0 .. 4, inputs aligned for the persistent
kernel's 16-byte loads or not, rows of `given` by index or not, and four batch sizes, and every combination is held
to a table written by hand from the order of the dispatch:

  1. a dynamics compiled as ltv: the sweep kernel, whatever the path;
  2. an instance fits a CU's LDS, the inputs are aligned, and the path is 0 -- or the plan was compiled with lti= or
     csc=, which no other kernel takes on chip: the persistent kernel;
  3. rows of `given` by index anywhere else: MPCASM_ERR_LIMIT;
  4. 128 unknowns or more, path != 2, no CSC: the tiled kernel;
  5. a plan with lti= or csc= that got here: MPCASM_ERR_LIMIT;
  6. the fused kernel's LDS is at most 80 KB and the path is 0 or 1: the fused kernel;
  7. the staged pipeline.

profiles/assemble_routes.txt holds what the launches themselves said, on the device, before assemble_route existed."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

import persistent_cases as pc
import sweep_cases as sc
import tiled_cases as tc
from mpcasm import capi, engine

R, F, S, T, W = capi.KERNEL_RESIDENT, capi.KERNEL_FUSED, capi.KERNEL_STAGED, capi.KERNEL_TILED, capi.KERNEL_SWEEP
L = "limit"                              # MPCASM_ERR_LIMIT
BATCHES = (1, 8, 4096, 65536)
PATHS = range(5)
RESIDENT_LDS_LIMIT = 156 * 1024          # csrc/plan_dev.h

# the family per path, for a launch that is (aligned, aligned and indexed, unaligned, unaligned and indexed); the
# batch does not enter (it picks the persistent kernel's hand-over of P, below)
ON_CHIP_ONLY = {path: (R, R, L, L) for path in PATHS}               # lti= or csc=: rules 2, then 3 and 5
ON_CHIP = {0: (R, R, F, L), 1: (F, L, F, L), 2: (S, L, S, L), 3: (S, L, S, L), 4: (S, L, S, L)}    # rules 2, 3, 6, 7
WIDE_LTI = {path: (L, L, L, L) if path == 2 else (T, L, T, L) for path in PATHS}                   # rules 3, 4, 5
WIDE = {path: (S, L, S, L) if path == 2 else (T, L, T, L) for path in PATHS}                       # rules 3, 4, 7
SWEEP = {path: (W, L, W, L) for path in PATHS}                                                     # rule 1

# family: the module of the case; p_direct: the persistent kernel's hand-over of P at the four batches -- straight
# to memory (1) while a launch writes less than 560e6 bytes, 8 (no^2 + no + nc no + nc) a piece, through LDS (0)
# beyond (mpcasm.h MPCASM_OPT_P_DIRECT; the clause for P costing a workgroup per CU needs a plan whose LDS crosses
# 80 KB with P and whose results are under 128 KB: none of these); a CSC plan reads P out of LDS at every size
Pinned = namedtuple("Pinned", "name family expect p_direct")
PINNED = [
    Pinned("lti-3-1-11", pc, ON_CHIP_ONLY, (1, 1, 1, 1)),         # the fewest unknowns: 7 392 bytes a piece
    Pinned("lipm3d-32", pc, ON_CHIP_ONLY, (1, 1, 0, 0)),          # more than 64 KB of LDS; 226 592 bytes a piece
    Pinned("biped16", pc, ON_CHIP_ONLY, (1, 1, 1, 0)),            # lti=, 16-byte image loads; 33 152 bytes a piece
    Pinned("biped16-mem", pc, ON_CHIP, (1, 1, 1, 0)),             # the same without lti=: the path decides
    Pinned("biped16-csc", pc, ON_CHIP_ONLY, (0, 0, 0, 0)),
    Pinned("fused-4-4-32", tc, WIDE_LTI, None),                   # 128 unknowns, lti=
    Pinned("refused-64-2-64-k4", tc, WIDE_LTI, None),             # the tiled path's own refusal comes after the route
    Pinned("shared-3", tc, WIDE, None),                           # 128 unknowns, S and U from memory
    Pinned("one-1-1-1", sc, SWEEP, None),                         # one unknown (and small enough for every kernel)
]
IDS = [p.name for p in PINNED]
_COMPILED = {}      # name -> (plan, source strides of a launch): compiled once, shared by the tests, left unchanged


def _compiled(api, pinned):
    if pinned.name not in _COMPILED:
        if pinned.family is pc:
            case = pc.BY_NAME[pinned.name]
            plan = pc.compile_case(pc.inputs(api, case, 1)[2], case)
            strides = [0] * len(plan.sources)
        elif pinned.family is tc:
            case, rng = tc.BY_NAME[pinned.name], np.random.default_rng(11)
            A, B = tc.plants(rng, 1, case.shape)
            plan = tc.compile_case(api, rng, case, (A[0], B[0]))[1]
            strides = tc.src_stride(plan, case)
        else:
            case, rng = sc.BY_NAME[pinned.name], np.random.default_rng(11)
            A, B = sc.plants(rng, 1, case.shape)
            plan = sc.compile_case(api, rng, case.shape, plant=(A[0, 0], B[0, 0]))[1]
            strides = [0] * len(plan.sources)
        _COMPILED[pinned.name] = (plan, strides)
    return _COMPILED[pinned.name]


def _route(plan, batch, path, aligned, indexed):
    try:
        return engine.assemble_route(plan, batch, path, aligned, indexed)
    except capi.MpcasmError as refusal:
        assert refusal.status == capi.ERR_LIMIT
        return L


def _table_args(plan):
    itab, dtab = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab)
    return itab, dtab, (itab.ctypes.data, itab.size, dtab.ctypes.data if dtab.size else None, dtab.size)


@pytest.mark.parametrize("pinned", PINNED, ids=IDS)
def test_every_combination_takes_its_route(cpu_api, pinned):
    plan, _ = _compiled(cpu_api, pinned)
    lds_direct, lds_with_p = engine.resident_lds_bytes(plan)
    for path in PATHS:
        for k, (aligned, indexed) in enumerate(((True, False), (True, True), (False, False), (False, True))):
            want = pinned.expect[path][k]
            for b, batch in enumerate(BATCHES):
                got = _route(plan, batch, path, aligned, indexed)
                where = (pinned.name, path, aligned, indexed, batch, got)
                assert (got if got == L else got.kernel) == want, where
                if want == R:
                    # the hand-over of P and the LDS that goes with it (mpcasm_resident_lds_bytes)
                    assert got.p_direct == pinned.p_direct[b], where
                    assert got.lds == (lds_direct if got.p_direct else lds_with_p), where
                    assert 0 < got.lds <= RESIDENT_LDS_LIMIT, where
                elif want == F:
                    assert 0 < got.lds <= 80 * 1024, where
                elif want != L:
                    assert got.lds == 0, where


def test_the_whole_lds_case_is_one(cpu_api):
    # (what "lipm3d-32" is pinned for: its persistent kernel needs the whole-LDS attribute at every batch)
    plan, _ = _compiled(cpu_api, PINNED[1])
    assert PINNED[1].name == "lipm3d-32" and min(engine.resident_lds_bytes(plan)) > 64 * 1024


@pytest.mark.parametrize("pinned", PINNED, ids=IDS)
def test_the_tiled_query_answers_where_the_route_is_tiled(cpu_api, pinned):
    """mpcasm_tiled_route: MPCASM_ERR_ARG exactly where an aligned launch does not take the tiled path; elsewhere its
    own answer -- the form, or the tiled path's refusal."""
    plan, strides = _compiled(cpu_api, pinned)
    itab, dtab, args = _table_args(plan)
    stride_arg = (ctypes.c_int64 * max(len(strides), 1))(*strides)
    out = (ctypes.c_int32 * 16)()
    for path in PATHS:
        for batch in BATCHES:
            rc = capi.load().mpcasm_tiled_route(*args, stride_arg, batch, 3, path, out)
            tiled = pinned.expect[path][0] == T
            assert (rc != capi.ERR_ARG) == tiled, (pinned.name, path, batch, rc)
            if tiled:
                assert rc == (capi.ERR_LIMIT if pinned.name.startswith("refused") else capi.OK), (pinned.name, path, rc)


def test_path_minus_one_is_the_process_wide_value(cpu_api):
    plan, _ = _compiled(cpu_api, PINNED[3])
    lib = capi.load()
    assert engine.assemble_route(plan, 8, -1).kernel == R
    try:
        for path in PATHS:
            capi.check(lib.mpcasm_set_option(capi.OPT_PATH, path), "mpcasm_set_option")
            assert engine.assemble_route(plan, 8, -1).kernel == ON_CHIP[path][0]
            assert engine.assemble_route(plan, 8, 0).kernel == R          # (a path of the call's own wins)
    finally:
        capi.check(lib.mpcasm_set_option(capi.OPT_PATH, 0), "mpcasm_set_option")


def test_query_checks_its_arguments(cpu_api):
    plan, _ = _compiled(cpu_api, PINNED[0])
    lib = capi.load()
    itab, dtab, args = _table_args(plan)
    out = (ctypes.c_int32 * 4)()
    assert lib.mpcasm_assemble_route(*args, 8, 0, 1, 0, out) == capi.OK and list(out) == [R, out[1], 1, 0]
    assert lib.mpcasm_assemble_route(*args, 8, 0, 1, 0, None) == capi.ERR_ARG
    assert lib.mpcasm_assemble_route(None, itab.size, dtab.ctypes.data, dtab.size, 8, 0, 1, 0, out) == capi.ERR_ARG
    assert lib.mpcasm_assemble_route(itab.ctypes.data, itab.size, None, dtab.size, 8, 0, 1, 0, out) == capi.ERR_ARG
    for batch, path, aligned, indexed in ((0, 0, 1, 0), (-1, 0, 1, 0), (8, 5, 1, 0), (8, -2, 1, 0), (8, 0, 2, 0),
                                          (8, 0, -1, 0), (8, 0, 1, 2), (8, 0, 1, -1)):
        assert lib.mpcasm_assemble_route(*args, batch, path, aligned, indexed, out) == capi.ERR_ARG, \
            (batch, path, aligned, indexed)
    assert lib.mpcasm_assemble_route(itab.ctypes.data, 4, dtab.ctypes.data, dtab.size, 8, 0, 1, 0, out) == -2
    # a refusal leaves nothing behind
    out[:] = [9, 9, 9, 9]
    assert lib.mpcasm_assemble_route(*args, 8, 0, 0, 0, out) == capi.ERR_LIMIT and list(out) == [0, 0, 0, 0]


def test_the_process_wide_options_keep_their_ranges():
    lib = capi.load()
    ranges = {capi.OPT_PATH: (4, 0), capi.OPT_P_DIRECT: (2, 0), capi.OPT_JIT: (2, 0), capi.OPT_RESIDENT_PER_CU: (16, 0),
              capi.OPT_JIT_FETCH_RUNS: (8, 8), capi.OPT_RESIDENT_GRID: (1 << 20, 0)}     # option: (greatest, default)
    try:
        for option, (greatest, _) in ranges.items():
            assert lib.mpcasm_set_option(option, -1) == capi.ERR_ARG
            assert lib.mpcasm_set_option(option, greatest + 1) == capi.ERR_ARG
            assert lib.mpcasm_set_option(option, greatest) == capi.OK and lib.mpcasm_set_option(option, 0) == capi.OK
        for value in (-5, 0, 1 << 30):
            assert lib.mpcasm_set_option(capi.OPT_PHASE_MASK, value) == capi.OK      # (any value)
        for option in (0, 8, -1):
            assert lib.mpcasm_set_option(option, 0) == capi.ERR_ARG
        assert lib.mpcasm_plan_set_option(None, capi.OPT_PATH, 0) == capi.ERR_ARG
    finally:
        for option, (_, default) in ranges.items():
            lib.mpcasm_set_option(option, default)
        lib.mpcasm_set_option(capi.OPT_PHASE_MASK, capi.PHASE_DEFAULT)
