"""A family of formulations that spans every variant of the tiled path (csrc/tiled.hip: tiled_choose picks the
scan form -- fused or behind the pre-passes, one of seven instantiations of toeplitz_scan_kernel<KP, CB> --, the
Toeplitz form, the shared-model form with one of seven shared_p_kernel<TG>, or the general kernel), shared by the
CPU test of the dispatch and of the bound (test_tiled_routes_cpu.py) and the GPU test of the arithmetic
(test_gpu_tiled_variants.py).

Two builders.  ``fused``: the pattern of problems.random_lti with the number of tracked states independent of n -- a
cost over the whole horizon on the first ``tracked`` states, effort on every input, two-sided bounds on the tracked
states, given = x0: every workspace row is a row of one of the K = tracked terms, so the plan has T_SCAN_FUSED.
``tracking``: helpers.lti_tracking_problem with its features (a cost on every state: K = n); its scheduled limit on
s1 adds workspace rows, so T_SCAN_FUSED is 0.  Compiled with ``lti=["plant"]`` (every instance its own (A, B)) -- or,
``shared``, without: the formulation's own S, U for the whole batch, the shared-model form.  In the terms of the
dispatch:

  K, nblk        Hessian terms, column blocks of N columns (inputs that are unknowns): <KP, CB> is the first of
                 (4,4) (8,4) (4,8) (8,8) (12,4) (12,6) (16,4) that holds both; none: the Toeplitz form
  N              odd: no scan form; N % 16, no % 16: whole_lines; N > 64 (T_SCAN_NMAX): no scan tables
  n              > 16 (SCAN_AREG): the gradient's recursion reads A from memory
  LDS            records of G's rows in LDS up to 80 KB (rows_in_lds); above 64 KB the whole-LDS attribute
  path           MPCASM_OPT_PATH 0 best, 1 scan behind the pre-passes, 4 Toeplitz, 3 general
  weights        shared form: TG = 4, 8, 12, 16, 20, 24, 32 just above their number; more than 32, or a batch below
                 twice their number: the general kernel
"""
from collections import namedtuple

import numpy as np

SCAN, TOEPLITZ, SHARED, GENERAL = 1, 2, 3, 4          # capi.TILED_*
NONE, SMALL, SYSTEM = 0, 1, 2                         # capi.TILED_TABLES_*
FORMS = {SCAN: "scan", TOEPLITZ: "toeplitz", SHARED: "shared", GENERAL: "general"}

# what a case pins of mpcasm_tiled_route's answer (lds: None = not pinned, the figure is checked against its bounds)
Route = namedtuple("Route", "form fused kp cb rows_in_lds whole_lines whole_lds tables tg sym lds")
# kind: "fused" | "tracking" | "shared"; tracked: states with a cost (tracking, shared: n); kw: lti_tracking_problem's
Shape = namedtuple("Shape", "name kind n m N tracked kw")
# K, nblk: T_SCAN, T_SCAN_NBLK of the plan (0, 0: no scan tables); fused: T_SCAN_FUSED
Case = namedtuple("Case", "shape path batch K nblk fused route halves")

LIMIT = "limit"     # the route of a launch that is refused (MPCASM_ERR_LIMIT)
BATCH = 19          # scan, Toeplitz, general: a workgroup per instance or block pair
SHARED_BATCH = 67   # >= 2 weights + 3 for every shared case, no multiple of SH_PIB = 16, SH_GIB = 8, SH_QB = 4


def scan(kp, cb, fused, rows_in_lds=1, whole_lines=0, whole_lds=0, lds=None):
    return Route(SCAN, fused, kp, cb, rows_in_lds, whole_lines, whole_lds, None, 0, 0, lds)


def other(form, tg=0, sym=1, whole_lds=0):
    return Route(form, 0, 0, 0, 0, 0, whole_lds, None, tg, sym, None)


def tables_of(kind, n, m, N, fused_route):
    """The pre-pass that makes the horizon tables: none where the kernel makes its own (fused) or the plan has no
    generated group (shared); a wavefront per few systems while X = [B | A] fits a wavefront's lanes and the tables
    of four wavefronts' systems 64 KB of LDS; else a workgroup per system."""
    if fused_route or kind == "shared":
        return NONE
    return SMALL if n * (m + n) <= 64 and N * n * n + n * m * 2 * N <= 1800 else SYSTEM


def _case(name, kind, n, m, N, route, K, nblk, tracked=None, path=0, fused=None, batch=None, halves=False, **kw):
    tracked = n if tracked is None else tracked
    fused = int(kind == "fused") if fused is None else fused
    batch = (SHARED_BATCH if kind == "shared" else BATCH) if batch is None else batch
    if route != LIMIT:
        route = route._replace(tables=tables_of(kind, n, m, N, route.form == SCAN and route.fused))
    return Case(Shape(name, kind, n, m, N, tracked, tuple(sorted(kw.items()))), path, batch, K, nblk, fused, route, halves)


CASES = [
    # ---- scan form, set-up fused (N % 4 == 0) ----------------------------------------------------------------
    _case("fused-4-4-32", "fused", 4, 4, 32, scan(4, 4, 1, whole_lines=1), 4, 4, halves=True),    # K = KP, nblk = CB
    _case("fused-8-4-32", "fused", 8, 4, 32, scan(8, 4, 1, whole_lines=1), 8, 4),                 # K = KP
    _case("fused-12-4-32", "fused", 12, 4, 32, scan(12, 4, 1, whole_lines=1), 12, 4),             # <12,4>, K = KP
    _case("fused-16-4-32", "fused", 16, 4, 32, scan(16, 4, 1, whole_lines=1), 16, 4),             # n = SCAN_AREG
    _case("fused-8-8-16", "fused", 8, 8, 16, scan(8, 8, 1, whole_lines=1), 8, 8),                 # a block = 16 columns
    _case("fused-4-8-64", "fused", 4, 8, 64, scan(4, 8, 1, whole_lines=1), 4, 8),                 # no = 512: 4 chunks
    _case("fused-12-6-24", "fused", 12, 6, 24, scan(12, 6, 1), 12, 6, halves=True),               # N % 16: no whole lines; have 16 + 8
    _case("fused-4-4-36", "fused", 4, 4, 36, scan(4, 4, 1), 4, 4),                                # have 32 + 4
    _case("fused-6-4-32-k5", "fused", 6, 4, 32, scan(8, 4, 1, whole_lines=1), 5, 4, tracked=5),   # K < n
    # ---- more than 16 states, fused --------------------------------------------------------------------------
    _case("fused-17-4-32-k16", "fused", 17, 4, 32, scan(16, 4, 1, whole_lines=1), 16, 4, tracked=16, halves=True),
    _case("fused-20-4-32-k4", "fused", 20, 4, 32, scan(4, 4, 1, whole_lines=1), 4, 4, tracked=4),
    _case("fused-24-6-64-k12", "fused", 24, 6, 64, scan(12, 6, 1, rows_in_lds=0, whole_lines=1, whole_lds=1, lds=102272),
          12, 6, tracked=12),
    _case("fused-40-3-44-k8", "fused", 40, 3, 44, scan(8, 4, 1, rows_in_lds=0, whole_lds=1, lds=85328), 8, 3, tracked=8),
    _case("fused-44-2-64-k4", "fused", 44, 2, 64, scan(4, 4, 1, rows_in_lds=0, whole_lines=1, whole_lds=1, lds=100928),
          4, 2, tracked=4),                                                                       # n (m + n) = 2024
    # ---- fused plans behind the pre-passes (MPCASM_OPT_PATH 1) -----------------------------------------------
    _case("prepass-4-4-32", "fused", 4, 4, 32, scan(4, 4, 0, whole_lines=1), 4, 4, path=1),
    _case("prepass-12-6-24", "fused", 12, 6, 24, scan(12, 6, 0), 12, 6, path=1),
    _case("prepass-20-4-32-k4", "fused", 20, 4, 32, scan(4, 4, 0, whole_lines=1), 4, 4, tracked=4, path=1),
    _case("prepass-24-6-64-k12", "fused", 24, 6, 64, scan(12, 6, 0, rows_in_lds=0, whole_lines=1, whole_lds=1),
          12, 6, tracked=12, path=1),
    # ---- scan form behind the pre-passes (T_SCAN_FUSED == 0) -------------------------------------------------
    _case("scan-5-4-34", "tracking", 5, 4, 34, scan(8, 4, 0), 5, 4, halves=True),                 # N even, N % 4 == 2
    _case("scan-9-4-32-mixed", "tracking", 9, 4, 32, scan(12, 4, 0, whole_lines=1), 9, 4, two_axis_limit=True),
    _case("scan-4-8-64-slack", "tracking", 4, 8, 64, scan(4, 8, 0, whole_lines=1), 4, 8, extra_unknown=True),   # no = 576
    _case("scan-4-4-32-scaled", "tracking", 4, 4, 32, scan(4, 4, 0, whole_lines=1), 4, 4, scaled=True),
    _case("scan-8-5-32-given", "tracking", 8, 5, 32, scan(8, 4, 0, whole_lines=1), 8, 4, given_input=True),     # nblk = m - 1
    _case("scan-3-4-40", "tracking", 3, 4, 40, scan(4, 4, 0), 3, 4),                              # the small table pre-pass
    _case("scan-16-4-32", "tracking", 16, 4, 32, scan(16, 4, 0, whole_lines=1), 16, 4),           # <16,4> behind the pre-passes
    _case("scan-8-8-16", "tracking", 8, 8, 16, scan(8, 8, 0, whole_lines=1), 8, 8),               # <8,8> likewise
    # ---- scan refused: the Toeplitz form ---------------------------------------------------------------------
    _case("toeplitz-13-5-32", "tracking", 13, 5, 32, other(TOEPLITZ), 13, 5),        # K > 12 with 5 blocks
    _case("toeplitz-9-7-32", "tracking", 9, 7, 32, other(TOEPLITZ), 9, 7),                        # K > 8 with 7 blocks
    _case("toeplitz-4-4-33", "tracking", 4, 4, 33, other(TOEPLITZ), 4, 4),                        # odd N
    # (odd N and odd n: S's table, n n N doubles, leaves U's on an odd double -- no 16-byte copies into LDS, so
    # neither the scan nor the Toeplitz form: the general kernel behind the pre-passes)
    _case("general-3-4-33", "tracking", 3, 4, 33, other(GENERAL), 3, 4),
    _case("toeplitz-4-2-100", "tracking", 4, 2, 100, other(TOEPLITZ), 0, 0, halves=True),         # N > T_SCAN_NMAX
    _case("toeplitz-4-4-40-scheduled", "tracking", 4, 4, 40, other(TOEPLITZ), 0, 0, scheduled_cost=True),
    # ---- a crossed cost: P is not symmetric, every block pair is multiplied (sym == 0) ------------------------
    _case("toeplitz-4-4-32-crossed", "tracking", 4, 4, 32, other(TOEPLITZ, sym=0), 0, 0, crossed_cost=True),
    _case("general-4-4-32-crossed", "tracking", 4, 4, 32, other(GENERAL, sym=0), 0, 0, path=3, crossed_cost=True),
    # ---- MPCASM_OPT_PATH 4: the Toeplitz form; 3: the general kernel -----------------------------------------
    _case("toeplitz-forced-fused-8-4-32", "fused", 8, 4, 32, other(TOEPLITZ), 8, 4, path=4),
    _case("toeplitz-forced-5-4-34", "tracking", 5, 4, 34, other(TOEPLITZ), 5, 4, path=4),
    _case("general-forced-fused-8-4-32", "fused", 8, 4, 32, other(GENERAL), 8, 4, path=3, halves=True),
    _case("general-forced-5-4-34", "tracking", 5, 4, 34, other(GENERAL), 5, 4, path=3),
    _case("general-3-3-43", "tracking", 3, 3, 43, other(GENERAL), 3, 3, path=3),    # odd width: 129
    # ---- refused outright (CPU only) -------------------------------------------------------------------------
    _case("refused-64-2-64-k4", "fused", 64, 2, 64, LIMIT, 4, 2, tracked=4),    # scan: 168 KB; tables: n (m + n) > 2048
] + [
    # ---- shared model: n + 1 weights, each the top of its TG -------------------------------------------------
    _case("shared-%d" % n, "shared", n, 4, 32, other(SHARED, tg=tg), 0, 0, fused=0, halves=n == 7)
    for n, tg in ((3, 4), (7, 8), (11, 12), (15, 16), (19, 20), (23, 24), (31, 32))
] + [
    _case("shared-32-over", "shared", 32, 4, 32, other(GENERAL), 0, 0, fused=0),     # 33 weights
    _case("shared-15-batch31", "shared", 15, 4, 32, other(GENERAL), 0, 0, fused=0, batch=31),   # batch < 2 x 16
]
BY_NAME = {c.shape.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
GPU_CASES = [c for c in CASES if c.route != LIMIT]

# every variant tiled_choose can select, written down from the dispatch: the scan form's seven instantiations times
# fused / behind the pre-passes, the shared form's seven TG, the Toeplitz and the general form
SCAN_INSTANTIATIONS = ((4, 4), (8, 4), (4, 8), (8, 8), (12, 4), (12, 6), (16, 4))
SHARED_TG = (4, 8, 12, 16, 20, 24, 32)
SELECTABLE = ({("scan", kp, cb, fused) for kp, cb in SCAN_INSTANTIATIONS for fused in (0, 1)}
              | {("shared", tg) for tg in SHARED_TG}
              | {(form, sym) for form in ("toeplitz", "general") for sym in (0, 1)}
              | {("tables", SMALL), ("tables", SYSTEM)})
# what no plan selects, with the reason: nothing -- the instantiation follows from the terms and blocks, fused from
# the plan's rows and the path option, TG from the weights, sym from whether a cost is crossed
UNREACHABLE = {}


def variant_of(r):
    if r.form == SCAN:
        return ("scan", r.kp, r.cb, r.fused)
    if r.form == SHARED:
        return ("shared", r.tg)
    return (FORMS[r.form], r.sym)


def plants(rng, batch, shape):
    """``batch`` plants free of cancellation (helpers.cancellation_free_plants), Perron root 1.3 -- 1.25 where the
    horizon does not keep the premise at 1.3."""
    from helpers import cancellation_free_plants

    state = rng.bit_generator.state
    try:
        return cancellation_free_plants(rng, batch, shape.n, shape.m, 1.3, shape.N)
    except AssertionError:
        rng.bit_generator.state = state
        return cancellation_free_plants(rng, batch, shape.n, shape.m, 1.25, shape.N)


def build(api, rng, shape, plant):
    """The Formulation of ``shape`` on the nominal pair ``plant = (A, B)``."""
    if shape.kind != "fused":
        from helpers import lti_tracking_problem

        return lti_tracking_problem(api, rng, shape.n, shape.m, shape.N, plant=plant, **dict(shape.kw))[0]
    n, m, N = shape.n, shape.m, shape.N
    A, B = plant
    inputs = ["u%d" % j for j in range(m)]
    states = ["s%d" % i for i in range(n)]
    ext = api.ExtendedSystem.from_cotrol_system(api.ControlSystem(inputs, states, A, B), "x", N)
    form = api.Formulation()
    form.incorporate_dynamics("plant", ext)
    for name in states[:shape.tracked]:
        form.incorporate_goal("track " + name, api.Cost(name, float(rng.uniform(0.1, 1)), aim=[float(rng.normal())]))
    for name in inputs:
        form.incorporate_goal("effort " + name, api.Cost(name, float(rng.uniform(0.1, 1))))
    for name in states[:shape.tracked]:
        form.incorporate_constraint("bounds " + name, [api.Constraint(name, float(rng.uniform(2, 6))),
                                                       api.Constraint(name, float(rng.uniform(2, 6)), arrow=[-1])])
    form.identify_qp_domain(inputs)
    form.make_preview_matrices()
    return form


def compile_case(api, rng, case, plant):
    from mpcasm.plan import compile_plan

    form = build(api, rng, case.shape, plant)
    return form, compile_plan(form, **({} if case.shape.kind == "shared" else {"lti": ["plant"]}))


def src_stride(plan, case):
    """The strides of a launch of the case: every instance its own (A, B) in the group's first two slots -- or
    every source shared."""
    strides = [0] * len(plan.sources)
    if case.shape.kind != "shared":
        n, m = case.shape.n, case.shape.m
        ids = plan.lti[0]["ids"]
        strides[ids[0]], strides[ids[1]] = n * n, n * m
    return strides
