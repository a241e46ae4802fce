"""A family of formulations that spans every variant of the persistent kernel (csrc/resident.hip:
resident_assemble_kernel<JC, STAMPS, GEN> ahead of time, resident_spec_kernel per plan), shared by the CPU test of
the plan words and of the bound (test_persistent_variants_cpu.py) and the GPU test of the arithmetic
(test_gpu_persistent_variants.py).  What a plan selects inside the kernel is read from its RS_* words (variant_of):

  jc_inst    launch_jc<JC>: the smallest of 3, 4, 5, 8, 12 that holds RS_JC compose ops per thread
  gen, nlti  GEN: the horizon tables made on chip from (A, B) of RS_NLTI systems (lti=); false: S, U fetched from
             memory with the image ("-mem": compiled without lti=)
  g_mode     resident_g_mode: 0 a record per row of G, 1 packed 16-byte pieces, 2 a descriptor per piece, 3 CSC
  sym        RS_SYM: P mirrored from its upper block triangle; 0 (a crossed cost): every block pair computed
  unit       RS_UNIT: bytes per image load, 4 where a stream is no whole number of 16-byte pieces
  compact    RS_COMPACT: every row-set of the workspace keeps its own window of the columns
  gfix       RS_NGFIX != 0: one-axis rounds of the descriptors with a second axis added for single lanes
  gsingle    mode 2, RS_GSINGLE: "all" rounds read one axis, or "mixed"; mode 3, CSC_GSINGLE: "all" entries by the
             one-axis product, or "two"; "none" without either table
  nzblk, nsplit   blocks of P no term reaches (zero-filled) / workspace elements two threads share (zeroed between
             instances)

Builders: problems.biped, random_lti, lipm3d, body_case; helpers.lti_tracking_problem; sweep_cases.build compiled
with lti= instead of ltv= (its limits have at most two axes: "-wide" adds one over three or four, the most a row record
holds, RS_AXMAX -- mode 0 at an even width); and three of this module -- ``systems`` (2 to 4 plants of different
sizes in one
formulation, a cost and a limit on a combination of the first two: RS_NLTI 2 .. 4), ``diagonal`` (an input that
carries two effort costs: both slots of RS_DIAG_MAX; a third takes the plan off the kernel) and ``shared-columns`` (a
limit over two axes whose variables depend on the same unknowns: every live piece of G needs both axes, so the
rounds that hold live pieces are two-axis rounds and the ones behind them one-axis rounds -- RS_GSINGLE mixed).

kappa: helpers.kappa(N, n) = 2 N (n + 1) with n the largest generated system: two table entries of at most N n-term
products each (2 N n), an N-term sum, and N to spare, which holds the few multiplications by an output's
coefficients, a weight, an arrow (the sweep and tiled families apply the same bound to their two-state outputs and
two-axis limits).  A ``systems`` case adds to it: a row of the combination sums the free responses of two plants,
n_a + n_b products instead of n_max, so n_min more additions and as many multiplications by the combination's
coefficients -- kappa + 2 n_min (Case.kappa_extra).  Derived, never fitted.
"""
import zlib
from collections import namedtuple

import numpy as np

JC_INSTANCES = (3, 4, 5, 8, 12)                    # launch_jc<JC> of resident.hip; 12 = RS_JC_MAX
Variant = namedtuple("Variant", "jc_inst gen nlti g_mode sym unit compact gfix gsingle nzblk nsplit")
# make: (builder, *arguments); kw: compile keywords (lti, csc, workspace); systems: ((dynamics, n, m), ...) whose
# (A, B) every instance has of its own, N their horizon; p_in_lds: P fits in LDS beside the workspace
# (mpcasm_resident_lds_bytes out[1] != 0 and within the limit); halves / count_index / fetch_runs / stride0 /
# sample: what the GPU test does with the case beyond the four builds
Case = namedtuple("Case", "name make kw systems N variant p_in_lds kappa_extra halves count_index fetch_runs stride0 "
                          "sample")

BATCH = 67                                         # >= 16 x 3: runs of four on a grid of 3, a tail of three
SAMPLES = (0, 33, 66)
GSINGLE_ALL = (1 << 24) - 1                        # RS_GDESC_PIECES x RS_GDESC_THREADS / 64 rounds


def V(jc, g_mode, gen=True, nlti=None, sym=1, unit=16, compact=0, gfix=False, gsingle=None, nzblk=False, nsplit=True):
    if gsingle is None:
        gsingle = "all" if g_mode in (2, 3) else "none"
    return Variant(jc, gen, (1 if gen else 0) if nlti is None else nlti, g_mode, sym, unit, compact, gfix, gsingle,
                   nzblk, nsplit)


def _case(name, make, systems, N, variant, p_in_lds=True, lti=True, csc=None, workspace=None, kappa_extra=0,
          halves=False, count_index=False, fetch_runs=False, stride0=False, sample=SAMPLES):
    kw = {}
    if lti:
        kw["lti"] = [s[0] for s in systems]
    if csc:
        kw["csc"] = csc
    if workspace:
        kw["workspace"] = workspace
    return Case(name, make, kw, tuple(systems), N, variant, p_in_lds, kappa_extra, halves, count_index, fetch_runs,
                stride0, sample)


LIP, PLANT = [("LIP", 3, 1)], lambda n, m: [("plant", n, m)]
B16, B16O, B24 = ("biped", 8, (6, 14)), ("biped", 8, (7, 15)), ("biped", 12, (10, 22))
SW9 = ("sweep", 3, 1, 9, 2, 4)                     # n, m, N, axes, limits
SW16 = ("sweep", 3, 1, 16, 2, 4)

CASES = [
    # ---- the biped: descriptors (36 and 34 unknowns: the 34-wide phase has pieces across the axes, 68 fixes) -----
    _case("biped16", B16, LIP, 16, V(4, 2, nzblk=True), halves=True, count_index=True, fetch_runs=True),
    _case("biped16-odd", B16O, LIP, 16, V(4, 2, gfix=True, nzblk=True), halves=True),
    _case("biped16-csc", B16, LIP, 16, V(4, 3, nzblk=True), csc="upper", halves=True, count_index=True),
    _case("biped16-odd-csc", B16O, LIP, 16, V(4, 3, gfix=True, nzblk=True), csc="upper"),
    _case("biped16-csc-full", B16, LIP, 16, V(4, 3, nzblk=True), csc="full"),
    _case("biped16-compact", B16, LIP, 16, V(4, 2, compact=1, nzblk=True), workspace="compact", halves=True),
    _case("biped16-odd-compact", B16O, LIP, 16, V(4, 2, compact=1, gfix=True, nzblk=True), workspace="compact"),
    _case("biped16-mem", B16, LIP, 16, V(4, 2, gen=False, nzblk=True), lti=False),
    _case("biped24", B24, LIP, 24, V(5, 1, nzblk=True), halves=True),
    _case("biped24-compact", B24, LIP, 24, V(5, 1, compact=1, nzblk=True), workspace="compact"),
    _case("biped24-mem", B24, LIP, 24, V(12, 1, gen=False, compact=1, nzblk=True, nsplit=False), lti=False,
          stride0=True),      # (RS_JC 9; compacted by plan_for_device: the dense plan leaves one workgroup a CU)
    # ---- problems.random_lti ------------------------------------------------------------------------------------
    _case("lti-8-4-16", ("lti", 8, 4, 16), PLANT(8, 4), 16, V(12, 1, nsplit=False), sample=(0, 66)),   # RS_JC 11
    _case("lti-4-1-9", ("lti", 4, 1, 9), PLANT(4, 1), 9, V(3, 0), halves=True),
    _case("lti-6-3-7", ("lti", 6, 3, 7), PLANT(6, 3), 7, V(3, 0)),
    _case("lti-6-3-7-mem", ("lti", 6, 3, 7), PLANT(6, 3), 7, V(3, 0, gen=False), lti=False),
    _case("lti-5-2-5", ("lti", 5, 2, 5), PLANT(5, 2), 5, V(3, 2, unit=4)),
    _case("lti-5-2-5-mem", ("lti", 5, 2, 5), PLANT(5, 2), 5, V(3, 2, gen=False, unit=4), lti=False),
    _case("lti-3-1-11", ("lti", 3, 1, 11), PLANT(3, 1), 11, V(3, 0, unit=4, nsplit=False)),
    # ---- helpers.lti_tracking_problem --------------------------------------------------------------------------
    _case("crossed-4-2-12", ("tracking", 4, 2, 12, "crossed_cost"), PLANT(4, 2), 12, V(3, 2, sym=0)),
    _case("crossed-5-3-9", ("tracking", 5, 3, 9, "crossed_cost"), PLANT(5, 3), 9, V(3, 0, sym=0, unit=4)),
    _case("given-4-2-12", ("tracking", 4, 2, 12, "given_input"), PLANT(4, 2), 12, V(8, 2, unit=4)),
    _case("slack-4-2-12", ("tracking", 4, 2, 12, "extra_unknown"), PLANT(4, 2), 12, V(3, 2, unit=4, nzblk=True)),
    # ---- sweep_cases.build, lti= in the place of ltv= -----------------------------------------------------------
    _case("sweep-3-1-9", SW9, PLANT(3, 1), 9, V(3, 2, unit=4, gfix=True, nzblk=True), fetch_runs=True),
    _case("sweep-3-1-9-compact", SW9, PLANT(3, 1), 9, V(3, 2, unit=4, compact=1, gfix=True, nzblk=True),
          workspace="compact"),
    _case("sweep-3-1-9-csc", SW9, PLANT(3, 1), 9, V(3, 3, unit=4, gfix=True, nzblk=True), csc="full",
          halves=True),
    _case("sweep-3-1-16-mem", SW16, PLANT(3, 1), 16, V(8, 2, gen=False, unit=4, nzblk=True, nsplit=False), lti=False,
          workspace="dense"),
    _case("sweep-4-1-10-a3-mem", ("sweep", 4, 1, 10, 3, 6), PLANT(4, 1), 10, V(5, 2, gen=False, nzblk=True), lti=False),
    _case("sweep-4-1-10-a3", ("sweep", 4, 1, 10, 3, 6), PLANT(4, 1), 10, V(4, 2, nzblk=True)),
    _case("sweep-2-1-6-a4", ("sweep", 2, 1, 6, 4, 8), PLANT(2, 1), 6, V(3, 2, nzblk=True)),
    _case("sweep-2-1-6-a4-wide", ("sweep", 2, 1, 6, 4, 8, 4), PLANT(2, 1), 6, V(3, 0, unit=4, nzblk=True)),   # 4 axes
    _case("sweep-2-1-6-a3-wide", ("sweep", 2, 1, 6, 3, 6, 3), PLANT(2, 1), 6, V(3, 0, unit=4, nzblk=True)),   # 3 axes
    # ---- problems.lipm3d (C3 in small and at its own size) and the reference's test_body problem -----------------
    _case("lipm3d-8", ("lipm3d", 8), LIP, 8, V(3, 2, unit=4, nzblk=True)),
    _case("lipm3d-32", ("lipm3d", 32), LIP, 32, V(12, 1, unit=4, compact=1, nzblk=True, nsplit=False),
          sample=(0, 66)),
    _case("body", ("body",), LIP, 9, V(3, 2, gen=False, sym=0, unit=4, gfix=True, nzblk=True, nsplit=False), lti=False),
    # ---- builders of this module -------------------------------------------------------------------------------
    _case("systems-2", ("systems", 6, ((3, 1), (2, 2))), [("p0", 3, 1), ("p1", 2, 2)], 6, V(3, 2, nlti=2, unit=4),
          kappa_extra=4, halves=True),
    _case("systems-4", ("systems", 5, ((3, 1), (2, 2), (4, 1), (1, 1))),
          [("p0", 3, 1), ("p1", 2, 2), ("p2", 4, 1), ("p3", 1, 1)], 5, V(3, 0, nlti=4, unit=4, nzblk=True),
          kappa_extra=4),
    _case("diagonal-3-2-6", ("diagonal", 3, 2, 6, 2), PLANT(3, 2), 6, V(3, 2, unit=4, nsplit=False)),
    _case("shared-columns-3-2-6", ("shared-columns", 3, 2, 6), PLANT(3, 2), 6, V(3, 2, unit=4, gsingle="mixed")),
    _case("shared-columns-3-2-6-csc", ("shared-columns", 3, 2, 6), PLANT(3, 2), 6, V(3, 3, unit=4, gsingle="two"),
          csc="full"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# plans the kernel refuses (RS_OK == 0), pinned by the CPU test: a third diagonal cost on one column
REFUSED = {"diagonal-3-2-6-third": ("diagonal", 3, 2, 6, 3)}

# every combination of the axes the family must reach (the CPU test enumerates the cases against it) ...
REQUIRED = ([("jc", jc, gen) for jc in JC_INSTANCES for gen in (True, False)]
            + [("g_mode", g) for g in (0, 1, 2, 3)]
            + [("compact", g) for g in (1, 2)]
            + [("gfix", compact) for compact in (0, 1)]
            + [("sym 0, P in LDS",)]
            + [("unit", unit, gen) for unit in (4, 16) for gen in (True, False)]
            + [("nlti", k) for k in (0, 1, 2, 4)]
            + [("gsingle", g, s) for g, s in ((2, "all"), (2, "mixed"), (3, "all"), (3, "two"))]
            + [("nzblk and nsplit",)])
# ... and the ones no plan reaches, with the reason
UNREACHABLE = {}


def variant_of(plan):
    """The Variant of a compiled plan, from its words."""
    from mpcasm.plan import _H

    it = plan.itab
    w = lambda name: int(it[_H[name]])
    csc = w("CSC_PNNZ") != 0 or w("CSC_GNNZ") != 0
    g_mode = 3 if csc else (0 if not w("RR_PACKED") else (2 if w("RS_NGDESC") else 1))
    if g_mode == 3:
        gsingle = "all" if w("CSC_GSINGLE") else "two"      # (one word for the plan: the one- or the two-axis product)
    elif g_mode == 2:
        gsingle = {0: "none", GSINGLE_ALL: "all"}.get(w("RS_GSINGLE"), "mixed")
    else:
        gsingle = "none"
    return Variant(next(j for j in JC_INSTANCES if j >= w("RS_JC")), w("RS_NLTI") != 0, w("RS_NLTI"), g_mode,
                   w("RS_SYM"), w("RS_UNIT"), w("RS_COMPACT"), w("RS_NGFIX") != 0, gsingle, w("RS_NZBLK") > 0,
                   w("RS_NSPLIT") > 0)


def kappa_of(case):
    from helpers import kappa

    return kappa(case.N, max(n for _, n, _ in case.systems)) + case.kappa_extra


def seed_of(case):
    """From the formulation alone: the lti, -mem, CSC and compact plans of one formulation, and the four builds of
    each, run on the same inputs and share one reference."""
    return zlib.crc32(repr(case.make).encode())


# --------------------------------------------------------------------------------------------------
# builders
# --------------------------------------------------------------------------------------------------
def _systems(api, rng, N, sizes, plants):
    form = api.Formulation()
    for k, (n, m) in enumerate(sizes):
        A, B = plants["p%d" % k]
        inputs = ["u%d_%d" % (k, j) for j in range(m)]
        states = ["s%d_%d" % (k, i) for i in range(n)]
        ext = api.ExtendedSystem.from_cotrol_system(api.ControlSystem(inputs, states, A, B), "x%d_" % k, N)
        form.incorporate_dynamics("p%d" % k, ext)
    form.incorporate_definition("mix", api.LineCombo({"s0_0": 1.0, "s1_0": -0.5}))
    for k, (n, m) in enumerate(sizes):
        for i in range(n):
            form.incorporate_goal("track %d %d" % (k, i), api.Cost("s%d_%d" % (k, i), float(rng.uniform(0.1, 1)),
                                                                    aim=[float(rng.normal())]))
        form.incorporate_goal("effort %d" % k, api.Cost("u%d_0" % k, float(rng.uniform(0.1, 1))))
        form.incorporate_constraint("bounds %d" % k, [api.Constraint("s%d_0" % k, 4.0),
                                                      api.Constraint("s%d_%d" % (k, n - 1), 3.0, arrow=[-1])])
    form.incorporate_goal("track mix", api.Cost("mix", 0.6, aim=[float(rng.normal())]))
    form.incorporate_constraint("mixed", [api.Constraint("mix", 1.5)])
    form.identify_qp_domain(["u%d_%d" % (k, j) for k, (n, m) in enumerate(sizes) for j in range(m)])
    form.make_preview_matrices()
    return form


def _plant_system(api, n, m, N, plant):
    inputs = ["u%d" % j for j in range(m)]
    states = ["s%d" % i for i in range(n)]
    A, B = plant
    return inputs, states, api.ExtendedSystem.from_cotrol_system(api.ControlSystem(inputs, states, A, B), "x", N)


def _diagonal(api, rng, n, m, N, efforts, plant):
    """random_lti's pattern with ``efforts`` effort costs on input u0 (a diagonal term each), one on the others."""
    inputs, states, ext = _plant_system(api, n, m, N, plant)
    form = api.Formulation()
    form.incorporate_dynamics("plant", ext)
    for name in states:
        form.incorporate_goal("track " + name, api.Cost(name, float(rng.uniform(0.1, 1)), aim=[float(rng.normal())]))
    for j, name in enumerate(inputs):
        for e in range(efforts if j == 0 else 1):
            form.incorporate_goal("effort %s %d" % (name, e),
                                  api.Cost(name, float(rng.uniform(0.1, 1)), aim=[float(rng.normal())]))
    for name in states[:2]:
        form.incorporate_constraint("bounds " + name, [api.Constraint(name, 5.0), api.Constraint(name, 5.0, arrow=[-1])])
    form.identify_qp_domain(inputs)
    form.make_preview_matrices()
    return form


def _shared_columns(api, rng, n, m, N, plant):
    """Limits over two "axes" y_a, y_b that are outputs of ONE plant: both rows of every line depend on every
    unknown, so each 16-byte piece of such a line has two live axes."""
    inputs, states, ext = _plant_system(api, n, m, N, plant)
    ext.define_output("y_a", {"s0": 1.0, "s1": -0.7})
    ext.define_output("y_b", {"s1": 1.3, "s2": 0.4})
    form = api.Formulation()
    form.incorporate_dynamics("plant", ext)
    for name in states:
        form.incorporate_goal("track " + name, api.Cost(name, float(rng.uniform(0.1, 1)), aim=[float(rng.normal())]))
    form.incorporate_goal("effort", api.Cost(inputs[-1], 0.3))
    form.incorporate_constraint("both", [
        api.Constraint("y", 2.0, axes=["_a", "_b"], arrow=[0.8, -1.1], center=[0.1, -0.2]),
        api.Constraint("y", 3.0, axes=["_a", "_b"], arrow=[-0.6, 0.9])])
    form.identify_qp_domain(inputs)
    form.make_preview_matrices()
    return form


def build(api, rng, make, plants):
    """The Formulation of ``make`` on the nominal pairs ``plants`` (dynamics name -> (A, B)); the builders of
    mpcasm.problems keep their own nominal system -- the plan's structure does not depend on it."""
    from mpcasm import problems

    kind, args = make[0], make[1:]
    if kind == "biped":
        form = problems.biped(api, problems.BipedConfig(step_samples=args[0]))
        form.update(step_times=np.array(args[1]), step_count=0)
        return form
    if kind == "lti":
        return problems.random_lti(api, rng, nx=args[0], nu=args[1], N=args[2])
    if kind == "tracking":
        from helpers import lti_tracking_problem

        return lti_tracking_problem(api, rng, args[0], args[1], args[2], plant=plants["plant"], **{args[3]: True})[0]
    if kind == "sweep":
        import sweep_cases as sc

        n, m, N, axes, limits = args[:5]
        form = sc.build(api, rng, sc._case("x", n, m, N, axes, None, limits=limits).shape, plants["plant"])
        if len(args) > 5:       # one more limit over ``args[5]`` axes at once (a row record holds RS_AXMAX = 4)
            over = sc.AXES[:args[5]]
            arrow = rng.uniform(0.5, 1.5, len(over)) * rng.choice([-1.0, 1.0], len(over))
            form.incorporate_constraint("wide", [api.Constraint("s0", 2.5, axes=over, arrow=[float(v) for v in arrow],
                                                                center=[float(v) for v in rng.normal(0, 0.2, len(over))])])
            form.make_preview_matrices()
        return form
    if kind == "lipm3d":
        return problems.lipm3d(api, N=args[0])
    if kind == "body":
        return problems.body_case(api)
    if kind == "systems":
        return _systems(api, rng, args[0], args[1], plants)
    if kind == "diagonal":
        return _diagonal(api, rng, *args, plant=plants["plant"])
    if kind == "shared-columns":
        return _shared_columns(api, rng, *args, plant=plants["plant"])
    raise KeyError(kind)


def inputs(api, case, batch, given_rows=1):
    """``(rng, plants, form, given)`` of a case: per system ``batch`` plants free of cancellation at Perron root 1.3
    (dynamics name -> (A, B) batched), the formulation on the first of them, ``given_rows x batch`` rows of given."""
    from helpers import cancellation_free_plants

    rng = np.random.default_rng(seed_of(case))
    plants = {name: cancellation_free_plants(rng, batch, n, m, 1.3, case.N) for name, n, m in case.systems}
    form = build(api, rng, case.make, {name: (A[0], B[0]) for name, (A, B) in plants.items()})
    given = rng.normal(0, 0.3, [given_rows * batch, form.given_len])
    return rng, plants, form, given


def params_of(plan, case, batch):
    """``(batch, nparams)``: every instance its own weights, aims, arrows, centres and extremes
    (sweep_cases.perturb_params), from the case's seed."""
    import sweep_cases as sc

    host = np.tile(np.asarray(plan.params, dtype=float), (batch, 1))
    return sc.perturb_params(plan, host, np.random.default_rng(seed_of(case) + 1))


def fetch_limit(plan, fetch_segments):
    """A limit of runs per chunk (MPCASM_OPT_JIT_FETCH_RUNS) that leaves the per-plan kernel chunks of both kinds:
    the fewest runs any chunk of the plan's fetch tables has, where another chunk has more
    (``fetch_segments``: test_fetch_segments_cpu's reading of mpcasm_fetch_segments)."""
    counts = [len(runs) for runs in fetch_segments(plan, 8).values() if runs]
    assert counts and min(counts) < max(counts), counts
    return min(counts)


def compile_case(form, case):
    """The plan an Assembler of BATCH instances compiles: compile_plan and engine.plan_for_device's choice of the
    workspace by the kernel's own LDS layout (no device needed)."""
    from mpcasm.engine import plan_for_device

    return plan_for_device(form, batch=BATCH, **case.kw)


def reference(form, case, plants, b, given):
    """``(x*, M)`` pairs in long double of instance ``b``: helpers.precise_reference, every generated system of
    the case set to the instance's own (A, B)."""
    from helpers import LD, precise_reference
    from oracle import qp_oracle as orc

    if len(case.systems) == 1:
        name = case.systems[0][0]
        return precise_reference(form, name, plants[name][0][b], plants[name][1][b], given)
    given = np.asarray(given, dtype=float).reshape(-1, 1)
    dyns = {name: form.dynamics[name] for name, _, _ in case.systems}
    out, saved = {}, {name: list(dyn.matrices) for name, dyn in dyns.items()}
    try:
        for magnitude in (False, True):
            for name, dyn in dyns.items():
                A, B = plants[name][0][b], plants[name][1][b]
                S, U = orc.extend_matrices(case.N, np.abs(A) if magnitude else A, np.abs(B) if magnitude else B, dtype=LD)
                dyn.matrices = list(U) + [S]
                dyn.update_definitions()
            PM = orc.preview_matrices(form, dtype=LD, magnitude=magnitude)
            G, h, P, q = orc.assemble(form, given, PM=PM, dtype=LD, magnitude=magnitude)
            for key, value in {"G": G, "h": h.ravel(), "P": P, "q": q.ravel()}.items():
                out.setdefault(key, []).append(value)
    finally:
        for name, dyn in dyns.items():
            dyn.matrices = saved[name]
            dyn.update_definitions()
    return {key: tuple(pair) for key, pair in out.items()}


def csc_reference(ref, csc):
    """The pairs of a CSC plan's outputs: the stored entries of P and G."""
    out = dict(ref)
    out["P"] = tuple(x.reshape(-1)[csc["p_flat"]] for x in ref["P"])
    out["G"] = tuple(x.reshape(-1)[csc["g_flat"]] for x in ref["G"])
    return out


def emulator_sources(plan, case, plants, b):
    """The sources of plan_emulator.run_resident for instance ``b``: (A, B) in the first two slots of a generated
    group; S, U in fp64 (the oracle's recurrence, what the fill kernel computes) where they come from memory."""
    from oracle import qp_oracle as orc

    srcs = [s.array for s in plan.sources]
    if plan.lti:
        for g in plan.lti:
            srcs[g["ids"][0]], srcs[g["ids"][1]] = plants[g["name"]][0][b], plants[g["name"]][1][b]
        return srcs
    keys = [s.key for s in plan.sources]
    for name, n, m in case.systems:
        S, U = orc.extend_matrices(case.N, plants[name][0][b], plants[name][1][b])
        for j in range(m):
            srcs[keys.index((name, j))] = np.asarray(U[j])
        srcs[keys.index((name, m))] = np.asarray(S)
    return srcs
