"""CPU: the kernel f2 picks for a plan (csrc/preview.hip, launch_preview_or_goals) as the library itself
reports it -- mpcasm_preview_route, the very function the launches decide with.  Every case of the family
in preview_cases.py is pinned to its instantiation, and the family is held to reach EVERY instantiation the
dispatch can select: an instantiation added later without a case fails here."""
import numpy as np
import pytest

import preview_cases as pc
from mpcasm import capi, engine


def _routes(api, case, monkeypatch):
    rng = np.random.default_rng(11)
    form, plan = pc.compile_case(api, rng, case.shape)
    terms, ngoals = pc.goal_table(form, plan)
    strides = pc.source_strides(plan, case.shape.streams)
    monkeypatch.delenv("MPCASM_PREVIEW_NO_BLOCKS", raising=False)
    rows = engine.preview_route(plan, strides)
    dist = engine.preview_route(plan, strides, len(terms), ngoals)
    monkeypatch.setenv("MPCASM_PREVIEW_NO_BLOCKS", "1")
    no_blocks = engine.preview_route(plan, strides)
    no_blocks_dist = engine.preview_route(plan, strides, len(terms), ngoals)
    monkeypatch.delenv("MPCASM_PREVIEW_NO_BLOCKS")
    return plan, (len(terms), ngoals), rows, dist, no_blocks, no_blocks_dist


@pytest.mark.parametrize("case", pc.CASES, ids=[c.shape.name for c in pc.CASES])
def test_every_case_takes_its_route(cpu_api, monkeypatch, case):
    plan, (nterms, _), rows, dist, no_blocks, no_blocks_dist = _routes(cpu_api, case, monkeypatch)
    assert pc.route_key(rows) == case.rows, pc.route_id(pc.route_key(rows))
    assert pc.route_key(dist) == case.dist, pc.route_id(pc.route_key(dist))
    assert pc.route_key(no_blocks) == case.no_blocks, pc.route_id(pc.route_key(no_blocks))
    assert no_blocks_dist is None          # only the blocked kernel writes distances
    # the dynamic LDS of the launch, from the plan's own sizes
    sh = case.shape
    W, nb = plan.ng + plan.no, sh.axes * (sh.n * sh.N + sh.m * sh.N + sh.n)     # (base rows: states, inputs, x0)
    if rows[0] == pc.DIRECT:
        assert rows[6] == (W + (W & 1) + nb + (nb & 1)) * 8 + 33 * 8
        assert rows[7] == (rows[6] > 64 * 1024)
    else:
        assert 0 < rows[6] <= 64 * 1024 and rows[7] == 0
    if dist is not None:                   # four instances' rows and the terms' sums behind the streams
        assert dist[6] == rows[6] + 4 * (plan.pmrows + nterms) * 8 <= 64 * 1024


def test_the_family_reaches_every_selectable_kernel(cpu_api, monkeypatch):
    reached = set()
    for case in pc.CASES:
        _, _, rows, dist, no_blocks, _ = _routes(cpu_api, case, monkeypatch)
        reached |= {pc.route_key(r) for r in (rows, dist, no_blocks) if r is not None}
    assert len(pc.UNREACHABLE) <= 4 and set(pc.UNREACHABLE) <= pc.SELECTABLE
    assert len(pc.SELECTABLE) == 32 + 24 + 2
    missing = pc.SELECTABLE - set(pc.UNREACHABLE) - reached
    assert not missing, "no case reaches " + ", ".join(sorted(pc.route_id(k) for k in missing))
    assert reached <= pc.SELECTABLE, "not in the written list: " + ", ".join(
        sorted(pc.route_id(k) for k in reached - pc.SELECTABLE))
    assert not reached & set(pc.UNREACHABLE), "reached after all: take it off the list of exceptions"


def test_distances_fall_back_exactly_where_the_launch_would(cpu_api, monkeypatch):
    """MPCASM_ERR_LIMIT for the distances: a stream of an instance's own, more than 16 terms, more than 64
    goals, the blocked kernel's LDS above 64 KB -- each on a plan whose rows DO run on the blocked kernel, with
    the other conditions met."""
    monkeypatch.delenv("MPCASM_PREVIEW_NO_BLOCKS", raising=False)
    by_name = {c.shape.name: c for c in pc.CASES}
    rng = np.random.default_rng(5)
    form, plan = pc.compile_case(cpu_api, rng, by_name["e16-wide-2axes"].shape)
    shared = [0] * len(plan.sources)
    assert pc.route_key(engine.preview_route(plan, shared, 16, 64)) == pc.blocked(16, 8, 1, 1)
    assert engine.preview_route(plan, shared, 17, 64) is None
    assert engine.preview_route(plan, shared, 16, 65) is None
    assert pc.route_key(engine.preview_route(plan, shared, 1, 1)) == pc.blocked(16, 8, 1, 1)
    for s in range(len(plan.sources)):     # any one stream per instance
        own = list(shared)
        own[s] = int(np.prod(plan.sources[s].array.shape))
        assert pc.route_key(engine.preview_route(plan, own)) == pc.staged(16, 1, 8, 1)
        assert engine.preview_route(plan, own, 1, 1) is None
    # the rows fit the blocked kernel's LDS, four instances' rows on top of them do not
    form, plan = pc.compile_case(cpu_api, rng, by_name["goals-lds"].shape)
    terms, ngoals = pc.goal_table(form, plan)
    rows = engine.preview_route(plan, [0] * len(plan.sources))
    assert rows[0] == pc.BLOCKED and rows[6] <= 64 * 1024 < rows[6] + 4 * (plan.pmrows + len(terms)) * 8
    assert len(terms) <= 16 and ngoals <= 64
    assert engine.preview_route(plan, [0] * len(plan.sources), len(terms), ngoals) is None
    # the real goal tables of the two other refusals
    for name, (nterms, goals) in (("goals-18-terms", (18, 18)), ("goals-65", (65, 65))):
        form, plan = pc.compile_case(cpu_api, rng, by_name[name].shape)
        terms, ngoals = pc.goal_table(form, plan)
        assert (len(terms), ngoals) == (nterms, goals)


def test_query_checks_its_arguments(cpu_api):
    import ctypes

    rng = np.random.default_rng(2)
    _, plan = pc.compile_case(cpu_api, rng, pc.CASES[0].shape)
    lib = capi.load()
    itab, dtab = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab)
    out = (ctypes.c_int32 * 8)()
    strides = (ctypes.c_int64 * len(plan.sources))()
    args = (itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size)
    assert lib.mpcasm_preview_route(*args, strides, 0, 0, out) == 0 and out[0] == pc.BLOCKED
    assert lib.mpcasm_preview_route(*args, None, 0, 0, out) == -1          # sources, no strides
    assert lib.mpcasm_preview_route(*args, strides, -1, 0, out) == -1
    assert lib.mpcasm_preview_route(*args, strides, 0, 0, None) == -1
    strides[0] = -8
    assert lib.mpcasm_preview_route(*args, strides, 0, 0, out) == -1
    assert lib.mpcasm_preview_route(itab.ctypes.data, 4, dtab.ctypes.data, dtab.size, strides, 0, 0, out) == -2
