"""A family of formulations that spans every variant of the staged pipeline (csrc/assemble.hip: staged_choose picks
hessian_kernel, a wavefront per 32 x 32 block of [P | q], or from 128 unknowns on hessian_gemm_kernel, a workgroup per
128 x 128 block pair, symmetric with the mirror store or all pairs, with gradient_kernel; constraints_kernel's three
branches) and of the per-instance fused kernel (csrc/fused.hip), shared by the CPU test of the dispatch and of the
bound (test_staged_routes_cpu.py) and the GPU test of the arithmetic (test_gpu_staged_variants.py).

Two builders.  A shape without an option of this module's own is helpers.lti_tracking_problem with its features.
``two_plants=m2`` (a second, decoupled dynamics "plant2" of n states and m2 inputs behind the first: a cost on one
plant's state has no structural non-zero in the other plant's columns, so its tile masks are empty there), ``axes=k``
(ControlSystem(..., axes=[k names]): the unknowns are the inputs on every axis, the limits run over 1, 2, ... up to k
axes) and ``per_row`` (arrows, centres and extremes of their own on every row of a limit) go to ``_build_own``.  The
plans are compiled WITHOUT ``lti=``: the sources are the horizon matrices S, U of every instance's own plant(s), which
the GPU test takes from engine.fill_su.  One plant per instance serves every axis; ``reference`` is
helpers.precise_reference over all the dynamics of a formulation (the helper itself takes one name).

In the terms of the kernels:

  no < 128       hessian_kernel: nbr x nbc blocks of 32 x 32, q in column no -- at no = 32 alone in a block column of
                 its own; a block pair whose rows or columns a term's masks leave empty is skipped
  no >= 128      hessian_gemm_kernel: nb = ceil(no / 128); sym (no crossed cost) nb (nb + 1) / 2 pairs, else nb nb;
                 stages of 16 rows, the last of a term shorter; 16-byte loads with a scalar tail at odd no; a term
                 whose masks are empty over a block's 8 tiles is skipped, unless the plan is beyond FUSED_MAX_OPS
                 (all-ones masks) or the block beyond tile 30; gradient_kernel: ceil(no / 64) column blocks
  K4             odd no: scalar; even no and a row of up to 2 axes: unrolled pairs, trips of 128 columns, whole
                 lines when 16 | no; even no and 3 to 8 axes: the loop over axes; more than 8: refused
  fused          nt = ceil(no / 16) <= 6 tiles a side (36 slots of 4 wavefronts x 9), two q columns per lane, up to
                 4 axes, arena + workspace within 80 KiB
"""
from collections import namedtuple

import numpy as np

NONE, BLOCK, GEMM = 0, 1, 2                        # capi.STAGED_*
FUSED, STAGED = 3, 4                               # capi.KERNEL_*
FORMS = {NONE: "none", BLOCK: "block", GEMM: "gemm"}
AXES = ["_a", "_b", "_c", "_d", "_e", "_f", "_g", "_h", "_i"]
LIMIT = "limit"     # the route of a launch that is refused (MPCASM_ERR_LIMIT)
WIDE_BATCH, SMALL_BATCH = 11, 70                   # neither a multiple of 8; 11 < 16
OWN = ("two_plants", "axes", "per_row")

# what a case pins of mpcasm_staged_route's answer (grids apart: they follow, and the CPU test holds them to it);
# lds: the fused kernel's, from mpcasm_assemble_route (None on the staged pipeline)
Route = namedtuple("Route", "kernel hessian sym nb npairs nbr nbc whole_lines max_axes lds")
Shape = namedtuple("Shape", "name n m N kw")
# facts: what table_facts must say of the plan (a subset of its keys); own_params: every instance its own weights,
# aims, arrows, centres, extremes; zero_weight: a cost weight of exactly 0 in some instances; gpu: False = CPU only
Case = namedtuple("Case", "shape path batch route facts halves own_params zero_weight gpu")


def staged(no, sym=1, max_axes=1, nc=True):
    """The route of a plan of ``no`` unknowns on the staged pipeline, written down from the dispatch."""
    whole = int(nc and no % 16 == 0)
    if no >= 128:
        nb = -(-no // 128)
        return Route(STAGED, GEMM, sym, nb, nb * (nb + 1) // 2 if sym else nb * nb, 0, 0, whole, max_axes, None)
    return Route(STAGED, BLOCK, 0, 0, 0, -(-no // 32), -(-(no + 1) // 32), whole, max_axes, None)


def fused(no, lds, max_axes=1):
    return staged(no, max_axes=max_axes)._replace(kernel=FUSED, lds=lds)


def _case(name, n, m, N, route, path=2, batch=None, facts=None, halves=False, own_params=False, zero_weight=False,
          gpu=True, **kw):
    no = (m - (1 if kw.get("given_input") else 0)) * N * kw.get("axes", 1) + kw.get("two_plants", 0) * N \
        + (N if kw.get("extra_unknown") else 0)
    batch = (WIDE_BATCH if no >= 128 else SMALL_BATCH) if batch is None else batch
    return Case(Shape(name, n, m, N, tuple(sorted(kw.items()))), path, batch, route, dict(facts or {}, no=no), halves,
                own_params, zero_weight, gpu and route != LIMIT)


# (flags of a gterm: 1 P, 2 half -- a crossed cost's two gradient terms --, 4 diagonal)
CASES = [
    # ---- hessian_kernel, forced by MPCASM_OPT_PATH 2 -----------------------------------------------------------
    _case("block-32", 3, 2, 16, staged(32), facts=dict(odd=0, axes=(1,)), halves=True),      # q alone in block column 1
    _case("block-33", 3, 3, 11, staged(33), facts=dict(odd=1)),                  # scalar K4; q inside block column 1
    _case("block-64", 3, 4, 16, staged(64), facts=dict(odd=0), own_params=True),             # whole lines, nbr 2
    _case("block-96-two-plants", 3, 4, 16, staged(96), two_plants=2, facts=dict(skip32=True, all_ones=False),
          zero_weight=True),
    _case("block-127", 2, 1, 127, staged(127), facts=dict(odd=1)),               # 4 x 4 blocks over 4 workgroups
    # ---- hessian_gemm_kernel -----------------------------------------------------------------------------------
    _case("gemm-128", 3, 4, 32, staged(128), facts=dict(odd=0), halves=True),    # nb 1; one K4 trip exactly full
    _case("gemm-129", 3, 3, 43, staged(129), facts=dict(odd=1)),                 # nb 2, second block 1 column wide
    _case("gemm-144-crossed", 3, 4, 36, staged(144, sym=0), crossed_cost=True, facts=dict(crossed=True)),
    _case("gemm-128-crossed", 3, 4, 32, staged(128, sym=0), crossed_cost=True, facts=dict(crossed=True)),   # nb 1
    _case("gemm-144-scheduled", 3, 4, 36, staged(144), scheduled_cost=True, facts=dict(short_stage=True, rows_mod4=True)),
    _case("gemm-160-two-plants", 3, 4, 32, staged(160), two_plants=1, facts=dict(skip128=True, all_ones=False)),
    _case("gemm-208-all-ones", 12, 2, 104, staged(208), facts=dict(all_ones=True, skip128=False)),   # second K4 trip
    _case("gemm-258", 3, 3, 86, staged(258), facts=dict(odd=0), own_params=True),            # nb 3: pairs bi = 1, 2
    _case("gemm-264-crossed", 3, 3, 88, staged(264, sym=0), crossed_cost=True, facts=dict(crossed=True)),   # 9 pairs
    _case("gemm-528", 2, 6, 88, staged(528), batch=5, facts=dict(odd=0)),        # block index 4: 8 bi >= 30
    # ---- also on the staged pipeline ---------------------------------------------------------------------------
    _case("axes-3", 2, 2, 4, staged(24, max_axes=3), axes=3, facts=dict(axes=(1, 2, 3), odd=0)),
    _case("axes-3-odd", 2, 1, 5, staged(15, max_axes=3), axes=3, facts=dict(axes=(1, 2, 3), odd=1)),
    _case("axes-5", 2, 1, 4, staged(20, max_axes=5), axes=5, path=0, facts=dict(axes=(1, 2, 3, 5), odd=0)),
    _case("axes-8", 2, 1, 4, staged(32, max_axes=8), axes=8, path=0, facts=dict(axes=(1, 2, 3, 8), odd=0)),
    _case("axes-9", 2, 1, 2, LIMIT, axes=9, path=0, facts=dict(axes=(1, 2, 3, 9))),
    _case("per-row", 3, 2, 10, staged(20), per_row=True, facts=dict(per_row=True), own_params=True),
    _case("slack", 3, 2, 12, staged(36), extra_unknown=True, facts=dict(diagonal=True)),
    _case("scaled", 3, 2, 12, staged(24), scaled=True),
    _case("two-axis-limit", 3, 2, 12, staged(24), two_axis_limit=True),
    _case("given-input", 3, 3, 12, staged(24), given_input=True),
    # ---- the fused kernel, MPCASM_OPT_PATH 1 -------------------------------------------------------------------
    _case("fused-16", 2, 4, 4, fused(16, 4264), path=1, facts=dict(odd=0), halves=True),     # one tile
    _case("fused-17", 2, 1, 17, fused(17, 15712), path=1, facts=dict(odd=1)),
    _case("fused-72", 2, 12, 6, fused(72, 22328), path=1, facts=dict(odd=0)),                 # second QSLOT column
    _case("fused-96", 2, 16, 6, fused(96, 29240), path=1, facts=dict(odd=0), zero_weight=True),   # all 36 tile slots
    _case("fused-axes-3", 2, 2, 4, fused(24, 8440, max_axes=3), path=1, axes=3, facts=dict(axes=(1, 2, 3))),
    _case("fused-axes-4", 2, 1, 4, fused(16, 9856, max_axes=4), path=1, axes=4, facts=dict(axes=(1, 2, 3, 4))),
    _case("fused-two-plants", 2, 4, 8, fused(48, 23944), path=1, two_plants=2, facts=dict(skip16=True, all_ones=False),
          own_params=True),
    _case("fused-scheduled", 2, 3, 9, fused(27, 15104), path=1, scheduled_cost=True, facts=dict(rows_mod4=True)),
]
BY_NAME = {c.shape.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
GPU_CASES = [c for c in CASES if c.gpu]


def names_of(shape):
    """The dynamics of a shape: name -> (n, m)."""
    kw = dict(shape.kw)
    out = {"plant": (shape.n, shape.m)}
    if kw.get("two_plants"):
        out["plant2"] = (shape.n, kw["two_plants"])
    return out


def plants(rng, batch, shape, rho=1.3):
    """name -> ``(A, B)`` of ``batch`` plants free of cancellation (helpers.cancellation_free_plants), Perron root
    ``rho`` -- 1.25, then 1.1, where the horizon does not keep the premise."""
    from helpers import cancellation_free_plants

    out = {}
    for name, (n, m) in names_of(shape).items():
        for r in (rho, 1.25, 1.1):
            state = rng.bit_generator.state
            try:
                out[name] = cancellation_free_plants(rng, batch, n, m, r, shape.N)
                break
            except AssertionError:
                rng.bit_generator.state = state
        else:
            raise AssertionError("no plant free of cancellation over %d steps" % shape.N)
    return out


def instance(plant, b):
    return {name: (A[b], B[b]) for name, (A, B) in plant.items()}


def _build_own(api, rng, shape, plant):
    n, m, N, kw = shape.n, shape.m, shape.N, dict(shape.kw)
    k = kw.get("axes", 0)
    axes = AXES[:k] if k else [""]
    per_row = bool(kw.get("per_row"))
    aim = lambda cols: [float(rng.normal()) for _ in range(cols)]
    form = api.Formulation()
    inputs = ["u%d" % j for j in range(m)]
    states = ["s%d" % i for i in range(n)]
    A, B = plant["plant"]
    ext = api.ExtendedSystem.from_cotrol_system(
        api.ControlSystem(inputs, states, A, B, **({"axes": axes} if k else {})), "x", N)
    form.incorporate_dynamics("plant", ext)
    domain = [u + a for a in axes for u in inputs]
    for s in states:
        form.incorporate_goal("track " + s, api.Cost(s, float(rng.uniform(0.1, 1)), aim=aim(len(axes)),
                                                     **({"axes": axes} if k else {})))
    form.incorporate_goal("effort", api.Cost(inputs[-1], 0.3, **({"axes": axes[:1]} if k else {})))
    if kw.get("two_plants"):
        m2 = kw["two_plants"]
        inputs2 = ["v%d" % j for j in range(m2)]
        states2 = ["t%d" % i for i in range(n)]
        A2, B2 = plant["plant2"]
        form.incorporate_dynamics("plant2", api.ExtendedSystem.from_cotrol_system(
            api.ControlSystem(inputs2, states2, A2, B2), "z", N))
        for s in states2:
            form.incorporate_goal("track " + s, api.Cost(s, float(rng.uniform(0.1, 1)), aim=aim(1)))
        form.incorporate_goal("effort2", api.Cost(inputs2[-1], 0.2))
        domain += inputs2

    def limit(var, extreme, over, **more):
        rows = len(more["schedule"]) if "schedule" in more else N
        shape_ = (rows, len(over)) if per_row else (len(over),)
        arrow = rng.choice([-1.0, 1.0], shape_) * rng.uniform(0.5, 1.5, shape_)
        center = rng.normal(0, 1, shape_)
        ext_ = extreme * rng.uniform(0.5, 1.5, (rows, 1)) if per_row else extreme
        return api.Constraint(var, ext_, arrow=arrow, center=center, **({"axes": over} if k else {}), **more)

    limits = [limit("s0", 4.0, axes[:1]), limit("s1", 2.0, axes[:1], schedule=range(N - 3, N))]
    if k:
        limits.append(limit("s0", 3.0, axes[:2]))
        limits.append(limit("s1", 3.5, axes[:3]))
        if k > 3:
            limits.append(limit("s0", 5.0, axes, schedule=range(1, N)))
    if kw.get("two_plants"):
        limits.append(limit("t0", 3.0, axes[:1]))
    if per_row:
        limits.append(api.Constraint("s0", 2.5))        # ... as well as one arrow, centre and extreme for all rows
    form.incorporate_constraint("limits", limits)
    form.identify_qp_domain(domain)
    form.make_preview_matrices()
    return form


def build(api, rng, shape, plant):
    """The Formulation of ``shape`` on the nominal plants ``plant`` (name -> (A, B))."""
    kw = dict(shape.kw)
    if any(key in kw for key in OWN):
        return _build_own(api, rng, shape, plant)
    from helpers import lti_tracking_problem

    return lti_tracking_problem(api, rng, shape.n, shape.m, shape.N, plant=plant["plant"], **kw)[0]


def compile_case(api, rng, case, plant):
    from mpcasm.plan import compile_plan

    form = build(api, rng, case.shape, plant)
    return form, compile_plan(form)


def source_arrays(form, plant, N):
    """(key, array) of every horizon matrix of an instance's plants, as the plan's sources name them: ``(name, j)``
    U_j for input j, ``(name, m)`` S -- in fp64 by the oracle (the CPU tests' stand-in for engine.fill_su)."""
    from oracle import qp_oracle as orc

    out = []
    for name, (A, B) in plant.items():
        S, U = orc.extend_matrices(N, A, B)
        out += [((name, j), np.asarray(Uj)) for j, Uj in enumerate(U)] + [((name, len(U)), np.asarray(S))]
    return out


def zero_weight_slots(plan, shape):
    """The parameter slots a ``zero_weight`` case sets to exactly 0 in some instances: every cost of the second
    plant where there is one (its block of P, its part of q: nothing but exact zeros), else every cost on a state
    (what remains of P is the effort's diagonal)."""
    second = bool(dict(shape.kw).get("two_plants"))
    picked = [start for (kind, name, field), (start, rows, cols) in plan.param_slots.items()
              if kind == "cost" and field == "weight"
              and ((name.startswith("track t") or name == "effort2") if second else name.startswith("track "))]
    assert picked
    return picked


def table_facts(plan):
    """What the kernels' tables hold (plan.itab): the parity of ``no``; the axis counts of the limits; whether a limit
    has arrows of its own per row; per gterm its flags, ``nrows % 4`` and ``nrows % 16``; whether some gterm's
    ``GT_MASKA`` / ``GT_MASKB`` is empty over a whole block of the kernel in question (``skip16`` the fused kernel's
    tile, ``skip32`` hessian_kernel's block, ``skip128`` the GEMM's -- among the blocks whose masks are consulted,
    tiles below 30); whether every mask is the all-ones of a plan above FUSED_MAX_OPS."""
    from mpcasm import plan as P

    it, H = np.asarray(plan.itab), P._H
    no, nc = int(it[H["NO"]]), int(it[H["NC"]])
    off = int(it[H["OFF_GTERM"]])
    gt = it[off:off + int(it[H["NGTERM"]]) * P.GT_WORDS].reshape(-1, P.GT_WORDS)
    off = int(it[H["OFF_LIMIT"]])
    lm = it[off:off + int(it[H["NLIMIT"]]) * P.LM_WORDS].reshape(-1, P.LM_WORDS)
    flags = gt[:, 6]
    dense = gt[(flags & P.GT_FLAG_DIAG) == 0]
    with_p = dense[(dense[:, 6] & P.GT_FLAG_P) != 0]
    ntile = -(-no // 16)

    def skip(tiles):
        """Some term with a Hessian part has no tile in some block of ``tiles`` tiles (rows or columns)."""
        for b in range(-(-ntile // tiles)):
            if tiles * b >= 30 and tiles > 1:
                break
            bits = sum(1 << min(t, 30) for t in range(tiles * b, min(tiles * (b + 1), ntile)))
            if any(not (int(r[7]) & bits) or not (int(r[8]) & bits) for r in with_p):
                return True
        return False

    return dict(
        no=no, nc=nc, odd=no & 1, nc_mod16=nc % 16, axes=tuple(sorted({int(x) for x in lm[:, 2]})),
        per_row=bool((lm[:, 5] != 1).any()), per_row_center=bool((lm[:, 7] != 1).any()),
        per_row_extreme=bool((lm[:, 9] != 1).any()),
        gterms=tuple((int(r[6]), int(r[2]) % 4, int(r[2]) % 16) for r in gt),
        diagonal=bool((flags & P.GT_FLAG_DIAG).any()), crossed=bool((flags & P.GT_FLAG_HALF).any()),
        short_stage=bool((with_p[:, 2] % 16 != 0).any()), rows_mod4=bool((dense[:, 2] % 4 != 0).any()),
        skip16=skip(1), skip32=skip(2), skip128=skip(8),
        # (from 31 tiles on a dense term sets all 31 bits by itself: then the empty fused program tells)
        all_ones=bool(len(with_p) and (with_p[:, 7:9] == 0x7FFFFFFF).all() and (ntile < 31 or it[H["NOPS"]] == 0)))


def reference(form, plant, given):
    """helpers.precise_reference over every dynamics of the formulation: ``(x*, M)`` pairs in long double of
    ``G, h, P, q`` for one instance whose dynamics ``name`` is ``plant[name] = (A, B)``."""
    from helpers import LD, precise_reference
    from oracle import qp_oracle as orc

    if len(plant) == 1:
        (name, (A, B)), = plant.items()
        return precise_reference(form, name, A, B, given)
    given = np.asarray(given, dtype=float).reshape(-1, 1)
    saved = {name: list(form.dynamics[name].matrices) for name in plant}
    out = {}
    try:
        for magnitude in (False, True):
            for name, (A, B) in plant.items():
                dyn = form.dynamics[name]
                N = dyn.matrices[-1].shape[0]
                S, U = orc.extend_matrices(N, np.abs(A) if magnitude else A, np.abs(B) if magnitude else B, dtype=LD)
                dyn.matrices = list(U) + [S]
                dyn.update_definitions()
            PM = orc.preview_matrices(form, dtype=LD, magnitude=magnitude)
            G, h, P, q = orc.assemble(form, given, PM=PM, dtype=LD, magnitude=magnitude)
            for key, value in (("G", G), ("h", h.ravel()), ("P", P), ("q", q.ravel())):
                out.setdefault(key, []).append(value)
    finally:
        for name, matrices in saved.items():
            form.dynamics[name].matrices = matrices
            form.dynamics[name].update_definitions()
    return {key: tuple(pair) for key, pair in out.items()}
