"""The input fetch of the per-plan persistent kernel by arithmetic (CPU).

The kernel compiled for one plan does not read its fetch tables before it asks for the first
instance's inputs: ``jit.hip`` describes every 64-lane chunk of ``OFF_RS_ABMETA`` (the (A, B) of
the generated systems) and of ``OFF_RS_INMETA`` (the image) as at most 8 *runs* -- (first lane,
lanes, stream, first byte, bytes per lane step, period in lanes) -- and the kernel works a lane's
source out from its index.  A chunk with more runs stays on the table.  Here, for every plan the
persistent-kernel tests of the suite compile, the runs expanded over the lanes are compared with
the tables entry for entry (``mpcasm_fetch_segments`` hands out exactly what the generated header
holds), every chunk is either described or left to the table, and the kernel is compiled for the
plan (``mpcasm_jit_check``, no device needed).
"""
import ctypes

import numpy as np
import pytest

from mpcasm import capi, engine, problems
from mpcasm._tables import VALUES
from mpcasm.plan import _H, compile_plan

LIMIT = VALUES["FS_MAX"]                      # runs per chunk the kernel takes


def biped(api, samples, times, reduced=False):
    form = problems.biped(api, problems.BipedConfig(step_samples=samples), reduced=reduced)
    form.update(step_times=np.array(times), step_count=0)
    return form


PLANS = {
    "c2-36": lambda api: compile_plan(biped(api, 8, [6, 14]), lti=["LIP"]),
    "c2-34": lambda api: compile_plan(biped(api, 8, [7, 15]), lti=["LIP"]),
    "c2-36-reduced": lambda api: compile_plan(biped(api, 8, [6, 14], reduced=True), lti=["LIP"]),
    "c2-34-reduced": lambda api: compile_plan(biped(api, 8, [7, 15], reduced=True), lti=["LIP"]),
    # (a launch that picks its `given` rows through an index runs the plan of c2-36; its CSC form:)
    "c2-36-csc": lambda api: compile_plan(biped(api, 8, [6, 14]), lti=["LIP"], csc="upper"),
    "c3": lambda api: engine.plan_for_device(problems.lipm3d(api, N=32), lti=("LIP",)),
    "n24-on-chip": lambda api: engine.plan_for_device(biped(api, 12, [10, 22]), lti=("LIP",)),
    "n24-from-memory": lambda api: engine.plan_for_device(biped(api, 12, [10, 22])),
    "body_case": lambda api: compile_plan(problems.body_case(api)),
    "c2-36-no-lti": lambda api: compile_plan(biped(api, 8, [6, 14])),
}


def fetch_segments(plan, limit):
    """{(kind, chunk): [run, ...]} as the library describes the plan's fetch tables; kind 0: (A, B), 1: image."""
    lib = capi.load()
    it = plan.itab
    out = np.zeros(3 * 4096, dtype=np.int32)
    n = ctypes.c_int64(0)
    rc = lib.mpcasm_fetch_segments(it.ctypes.data, it.size, plan.dtab.ctypes.data, plan.dtab.size, limit,
                                   out.ctypes.data, out.size, ctypes.byref(n))
    assert rc == 0, rc
    words, at, chunks = out[:n.value], 0, {}
    while at < len(words):
        kind, chunk, runs = (int(w) for w in words[at:at + 3])
        assert (kind, chunk) not in chunks
        chunks[(kind, chunk)] = [tuple(int(w) for w in words[at + 3 + 6 * r:at + 9 + 6 * r]) for r in range(runs)]
        at += 3 + 6 * runs
    assert at == len(words)
    return chunks


def expand(runs):
    """(stream, byte offset) of the 64 lanes of a chunk from its runs, the way the kernel does it: the
    last run that starts at or before the lane."""
    entries = np.full((64, 2), -1, dtype=np.int64)
    covered = 0
    for first, lanes, stream, byte0, step, period in runs:
        assert first == covered and lanes >= 1 and period >= 1, runs      # ascending, no gap
        assert period >= lanes or period in (1, 2, 4), runs               # (the kernel masks the lane index)
        for lane in range(first, first + lanes):
            entries[lane] = stream, byte0 + ((lane - first) % period) * step
        covered = first + lanes
    assert covered == 64, runs
    return entries


def maximal_runs(entries):
    """Number of runs the library's greedy parse makes of a chunk, counted here from the table itself: at
    each lane the longest of a plain run (constant step) and a run of period 1, 2 or 4 lanes."""
    count, i, n = 0, 0, len(entries)
    while i < n:
        stream, byte0 = entries[i]
        step = entries[i + 1][1] - byte0 if i + 1 < n and entries[i + 1][0] == stream else 0
        best = 0
        for period in (0, 4, 2, 1):
            length = 0
            while (i + length < n and entries[i + length][0] == stream and entries[i + length][1]
                   == byte0 + (length % period if period else length) * (0 if period == 1 else step)):
                length += 1
            best = max(best, length)
        count, i = count + 1, i + best
    return count


def tables(plan):
    it = plan.itab
    ab = it[it[_H["OFF_RS_ABMETA"]]:][:it[_H["RS_AB"]] * 4].reshape(-1, 64, 2)
    image = it[it[_H["OFF_RS_INMETA"]]:][:it[_H["RS_NCHUNK"]] * 128].reshape(-1, 64, 2)
    return {0: ab, 1: image}


@pytest.mark.parametrize("name", list(PLANS))
def test_runs_expand_to_the_fetch_tables(cpu_api, name):
    plan = PLANS[name](cpu_api)
    it = plan.itab
    assert it[_H["RS_OK"]] == 1
    table = tables(plan)
    assert (it[_H["RS_NLTI"]] == 0) == (table[0].shape[0] == 0)
    for limit in (LIMIT, 3, 1, 0):
        chunks = fetch_segments(plan, limit)
        # every chunk of both tables is listed once: described by its runs, or left to the table
        assert sorted(chunks) == [(kind, k) for kind in (0, 1) for k in range(table[kind].shape[0])]
        for (kind, k), runs in chunks.items():
            assert len(runs) <= min(limit, LIMIT)
            if runs:
                assert np.array_equal(expand(runs), table[kind][k]), (name, kind, k, runs)
            else:
                # ... because it has more runs than the limit allows (or is an image chunk from 32 on, which
                # the kernel's mask of table chunks does not reach), not for nothing
                assert maximal_runs(table[kind][k]) > limit or (kind == 1 and k >= 32), (name, kind, k)
    described = {key: len(runs) for key, runs in fetch_segments(plan, LIMIT).items()}
    print(name, "runs per chunk:", described)
    if name == "c2-36":
        # the headline plan: its one chunk of (A, B) and both chunks of its image are fetched by arithmetic
        # (counted from the compiled plan before the kernel was written: 5, 6 and 2 maximal runs; the
        # padding behind B and the padding of the slot read the same constant and are one run here)
        assert sorted(described) == [(0, 0), (1, 0), (1, 1)]
        assert described[(0, 0)] == 4 and described[(1, 0)] == 6 and described[(1, 1)] == 2
    if name == "body_case":
        # the plan the GPU test runs with a limit of 3 runs: some chunks by arithmetic, some on the table
        counts = [len(r) for r in fetch_segments(plan, 3).values()]
        assert 0 in counts and max(counts) > 0


def test_a_chunk_of_many_runs_stays_on_the_table(cpu_api):
    """No plan of the suite has a chunk of more than 8 runs, so the default limit's table path is met here by
    a plan whose image is shuffled: the headline plan's first image chunk with every other 16-byte piece
    swapped has far more than 8 runs.  It is left to the table, the untouched chunks keep their runs, and the
    kernel with chunks of both kinds compiles."""
    lib = capi.load()
    plan = PLANS["c2-36"](cpu_api)
    it = plan.itab.copy()
    meta = it[it[_H["OFF_RS_INMETA"]]:][:128].reshape(64, 2)
    meta[0:32:2], meta[1:32:2] = meta[1:32:2].copy(), meta[0:32:2].copy()
    assert maximal_runs(meta) > LIMIT

    class Shuffled:
        itab, dtab = it, plan.dtab

    chunks = fetch_segments(Shuffled, LIMIT)
    assert chunks[(1, 0)] == [] and len(chunks[(1, 1)]) == 2 and len(chunks[(0, 0)]) == 4
    log = ctypes.create_string_buffer(1 << 16)
    rc = lib.mpcasm_jit_check(it.ctypes.data, it.size, plan.dtab.ctypes.data, plan.dtab.size, log, len(log))
    assert rc == 0, log.value.decode()


def test_the_kernel_compiles_with_chunks_of_both_kinds(cpu_api):
    """The build the GPU test runs for the reference's test_body problem: at most 3 runs per chunk."""
    lib = capi.load()
    plan = PLANS["body_case"](cpu_api)
    log = ctypes.create_string_buffer(1 << 16)
    assert lib.mpcasm_set_option(capi.OPT_JIT_FETCH_RUNS, 3) == 0
    try:
        rc = lib.mpcasm_jit_check(plan.itab.ctypes.data, plan.itab.size, plan.dtab.ctypes.data, plan.dtab.size,
                                  log, len(log))
    finally:
        assert lib.mpcasm_set_option(capi.OPT_JIT_FETCH_RUNS, LIMIT) == 0
    assert rc == 0, log.value.decode()
    assert lib.mpcasm_set_option(capi.OPT_JIT_FETCH_RUNS, LIMIT + 1) == -1
    assert lib.mpcasm_set_option(capi.OPT_JIT_FETCH_RUNS, -1) == -1


@pytest.mark.parametrize("name", list(PLANS))
def test_the_kernel_compiles_for_the_plan(cpu_api, name):
    lib = capi.load()
    plan = PLANS[name](cpu_api)
    log = ctypes.create_string_buffer(1 << 16)
    rc = lib.mpcasm_jit_check(plan.itab.ctypes.data, plan.itab.size, plan.dtab.ctypes.data, plan.dtab.size,
                              log, len(log))
    assert rc == 0, log.value.decode()
