"""A family of formulations that spans every kernel variant of f2 (csrc/preview.hip: launch_preview_or_goals),
shared by the CPU test of the dispatch (test_preview_routes_cpu.py) and the GPU test of the arithmetic
(test_gpu_preview_variants.py).

One plant ``x+ = A x + B u`` (n states, m inputs) over N steps on ``axes`` axes that share its horizon
matrices, plus outputs that combine 2 states (``narrow``, one per axis) and 5 to 8 states across the axes
(``wide``; the first one 8 wherever the formulation has 8 states), with coefficients of both signs.  In the terms of the dispatch:

  entries per base row  e1 = n + m N      -> E1 = 8, 16, 24, 32; more: the direct kernel
  longest definition row e2 = 2 or 5..8   -> E2 = 4, 8
  base rows             axes (n N + m N + n)       -> R1 = ceil(base rows / 256)
  definition rows       base rows + N (axes narrow + wide) -> R2 = ceil(definition rows / 256)

Every base variable is a definition too, so R2 >= R1 always: R1 = 2 with R2 = 1 does not exist
(UNREACHABLE below)."""
from collections import namedtuple

import numpy as np

from mpcasm import capi

DIRECT, STAGED, BLOCKED = capi.PREVIEW_DIRECT, capi.PREVIEW_STAGED, capi.PREVIEW_BLOCKED
AXES = ["_%s" % c for c in "abcdefghijklmnopqrstuvwxyz"]      # (an axis is matched on two characters: dynamics.py)

# streams: "shared" (one S, U for the batch), "bound" (engine.fill_su's S, U per instance), "lti" (tables
# generated on chip from per-instance (A, B)).  goals: "few" (4 or 5 terms), "terms18" (18 goals of one term),
# "goals65" (65 goals of one term).  batches: the sizes the GPU test launches.
Shape = namedtuple("Shape", "name n m N axes narrow wide streams goals batches")


def _shape(name, n, m, N, axes, narrow, wide, streams="shared", goals="few", batches=(5,)):
    return Shape(name, n, m, N, axes, narrow, wide, streams, goals, tuple(batches))


def blocked(e1, e2, r2, dist=0):
    return (BLOCKED, e1, 1, e2, r2, dist, 0)


def staged(e1, r1, e2, r2):
    return (STAGED, e1, r1, e2, r2, 0, 0)


def direct(whole_lds=0):
    return (DIRECT, 0, 0, 0, 0, 0, whole_lds)


def route_key(out):
    """(route, E1, R1, E2, R2, DIST, whole LDS) of ``engine.preview_route``'s answer (None stays None)."""
    return None if out is None else tuple(out[:6]) + (out[7],)


def route_id(key):
    if key is None:
        return "limit"
    name = capi.PREVIEW_ROUTES[key[0]]
    if key[0] == DIRECT:
        return name + ("-whole-lds" if key[6] else "")
    return "%s<%d,%d,%d,%d>%s" % ((name,) + tuple(key[1:5]) + ("-dist" if key[5] else "",))


# Every instantiation launch_preview_or_goals can select, written down from the dispatch:
#   preview_blocked_kernel<E1, E2, R2, 4, DIST>   (R1 = 1)
#   preview_staged_kernel<E1, R1, E2, R2>         R1 = 1 with E1 <= 32, R1 = 2 with E1 <= 16
#   preview_direct_kernel                         below and above 64 KB of LDS
SELECTABLE = (
    {blocked(e1, e2, r2, d) for e1 in (8, 16, 24, 32) for e2 in (4, 8) for r2 in (1, 2) for d in (0, 1)}
    | {staged(e1, 1, e2, r2) for e1 in (8, 16, 24, 32) for e2 in (4, 8) for r2 in (1, 2)}
    | {staged(e1, 2, e2, r2) for e1 in (8, 16) for e2 in (4, 8) for r2 in (1, 2)}
    | {direct(0), direct(1)})
# ... and those no plan reaches: every base variable (an input, x0, a state) is a definition of the
# formulation, so the definition rows are at least the base rows and R2 >= R1.
UNREACHABLE = {
    staged(8, 2, 4, 1): "R1 = 2 needs more than 256 base rows, R2 = 1 at most 256 definition rows; base rows are definition rows",
    staged(8, 2, 8, 1): "as <8,2,4,1>",
    staged(16, 2, 4, 1): "as <8,2,4,1>",
    staged(16, 2, 8, 1): "as <8,2,4,1>",
}

# name, n, m, N, axes, narrow, wide, streams, goals, batches; then the routes the dispatch must take:
# rows, distances (None: MPCASM_ERR_LIMIT), rows under MPCASM_PREVIEW_NO_BLOCKS
Case = namedtuple("Case", "shape rows dist no_blocks")


def _shared(name, n, m, N, axes, narrow, wide, e1, e2, r2, **kw):
    return Case(_shape(name, n, m, N, axes, narrow, wide, **kw), blocked(e1, e2, r2), blocked(e1, e2, r2, 1),
                staged(e1, 1, e2, r2))


def _own(name, n, m, N, axes, narrow, wide, streams, route, **kw):
    return Case(_shape(name, n, m, N, axes, narrow, wide, streams=streams, **kw), route, None, route)


CASES = [
    # every stream shared by the batch: the blocked kernel for rows and for distances, and the staged kernel
    # with no stream of an instance's own when blocks are switched off
    _shared("e8-narrow", 5, 1, 3, 1, 1, 0, 8, 4, 1),
    _shared("e8-wide-2axes", 5, 1, 3, 2, 0, 1, 8, 8, 1, batches=(37,)),
    _shared("e8-narrow-9axes", 4, 1, 3, 9, 4, 0, 8, 4, 2),
    _shared("e8-wide-9axes", 5, 1, 3, 9, 2, 1, 8, 8, 2, batches=(4099,)),
    _shared("e16-narrow", 5, 1, 11, 1, 1, 0, 16, 4, 1),
    _shared("e16-wide-2axes", 6, 1, 10, 2, 1, 1, 16, 8, 1),
    _shared("e16-narrow-3axes", 5, 1, 9, 3, 3, 0, 16, 4, 2, batches=(37,)),
    _shared("e16-wide-257-rows", 5, 1, 11, 3, 1, 1, 16, 8, 2, batches=(261,)),
    _shared("e24-narrow", 6, 2, 8, 1, 1, 0, 24, 4, 1),
    _shared("e24-wide", 8, 2, 8, 1, 0, 1, 24, 8, 1),
    _shared("e24-narrow-3axes", 6, 2, 9, 3, 1, 0, 24, 4, 2),
    _shared("e24-wide-2axes", 8, 2, 8, 2, 5, 2, 24, 8, 2, batches=(37,)),
    _shared("e32-narrow", 8, 2, 11, 1, 1, 0, 32, 4, 1),
    _shared("e32-wide", 8, 3, 8, 1, 0, 1, 32, 8, 1),
    _shared("e32-narrow-256-base-rows", 8, 2, 12, 2, 1, 0, 32, 4, 2),
    _shared("e32-wide-256-base-rows", 8, 2, 12, 2, 0, 1, 32, 8, 2),
    # a stream per instance: the staged kernel, R1 = 1 ...
    _own("own-e8-lti", 5, 1, 3, 1, 1, 0, "lti", staged(8, 1, 4, 1)),
    _own("own-e16-bound", 5, 1, 11, 1, 1, 1, "bound", staged(16, 1, 8, 1), batches=(37,)),
    _own("own-e24-lti", 6, 2, 9, 3, 1, 0, "lti", staged(24, 1, 4, 2), batches=(261,)),
    # (56 KB of LDS: two workgroups per CU, so that 4099 instances are more than 8 x the grid)
    _own("own-e32-bound-56kb", 9, 1, 23, 1, 0, 1, "bound", staged(32, 1, 8, 2), batches=(4099,)),
    # ... and R1 = 2 (more than 256 base rows)
    _own("own-e8-bound-299-base-rows", 5, 1, 3, 13, 2, 0, "bound", staged(8, 2, 4, 2)),
    _own("own-e8-lti-299-base-rows", 5, 1, 3, 13, 0, 1, "lti", staged(8, 2, 8, 2), batches=(37,)),
    _own("own-e16-lti-284-base-rows", 5, 1, 11, 4, 2, 0, "lti", staged(16, 2, 4, 2)),
    _own("own-e16-bound-284-base-rows", 5, 1, 11, 4, 1, 1, "bound", staged(16, 2, 8, 2), batches=(261,)),
    _own("shared-299-base-rows", 5, 1, 3, 13, 1, 1, "shared", staged(8, 2, 8, 2)),
    # the direct kernel: lists longer than 32, more than 512 definition rows, LDS below and above 64 KB
    _own("direct-38-entries", 5, 3, 11, 1, 1, 0, "bound", direct()),
    _own("direct-580-rows", 5, 1, 3, 20, 1, 1, "shared", direct()),
    _own("direct-66kb", 12, 1, 64, 9, 0, 0, "shared", direct(1)),
    # distances the blocked kernel refuses: more than 16 terms, more than 64 goals, its LDS above 64 KB
    Case(_shape("goals-18-terms", 5, 1, 3, 1, 1, 0, goals="terms18"), blocked(8, 4, 1), None, staged(8, 1, 4, 1)),
    Case(_shape("goals-65", 5, 1, 11, 1, 1, 1, goals="goals65"), blocked(16, 8, 1), None, staged(16, 1, 8, 1)),
    Case(_shape("goals-lds", 9, 1, 23, 1, 0, 1), blocked(32, 8, 2), None, staged(32, 1, 8, 2)),
]


def wide_width(shape, k):
    """Entries of the k-th wide output: 8, 5, 6, 7, ... states, as far as the formulation has that many."""
    width = min(shape.n * shape.axes, 5 + (k + 3) % 4)
    assert width >= 5, "a wide output needs five states"
    return width


def build(api, rng, shape, plant=None):
    """The Formulation of ``shape``; ``plant``: the nominal ``(A, B)`` (default: problems.random_lti_matrices)."""
    from mpcasm import problems

    n, m, N = shape.n, shape.m, shape.N
    axes = AXES[:shape.axes]
    A, B = problems.random_lti_matrices(rng, n, m) if plant is None else plant
    inputs = ["u%d" % j for j in range(m)]
    states = ["s%d" % i for i in range(n)]
    ext = api.ExtendedSystem.from_cotrol_system(api.ControlSystem(inputs, states, A, B, axes=axes), "x", N)
    outputs = []
    for k in range(shape.narrow):           # two states, the second coefficient negative
        i = k % n
        ext.define_output("y%d" % k, {states[i]: float(rng.uniform(0.5, 2.0)),
                                      states[(i + 1) % n]: -float(rng.uniform(0.5, 2.0))})
        outputs.append("y%d" % k)
    wide = {}
    for k in range(shape.wide):             # 8, 5, 6, 7, ... states, across the axes, alternating signs
        sign = float(rng.choice([-1.0, 1.0]))
        wide["w%d" % k] = api.LineCombo({states[(k + i) % n] + axes[(i // n) % len(axes)]:
                                         sign * (-1.0) ** i * float(rng.uniform(0.3, 3.0))
                                         for i in range(wide_width(shape, k))})
    form = api.Formulation()
    form.incorporate_dynamics("plant", ext)
    for name, combo in wide.items():
        form.incorporate_definition(name, combo)
    tracked = outputs + states + inputs     # what the goals cycle over (a name per axis)
    aim = lambda k: [float(rng.normal()) for _ in range(k)]
    if shape.goals == "few":
        two = axes[:2]
        form.incorporate_goal("track", api.Cost(tracked[0], 0.7, aim=aim(len(two)), axes=two))
        form.incorporate_goal("hold", api.Cost(states[-1], 0.2, aim=aim(1), axes=axes[-1:]))
        form.incorporate_goal("effort", api.Cost(inputs[-1], 0.3, aim=aim(1), axes=axes[:1]))
        if wide:
            form.incorporate_goal("wide", api.Cost("w0", 0.5, aim=aim(1)))
    else:
        for g in range({"terms18": 18, "goals65": 65}[shape.goals]):
            form.incorporate_goal("goal %d" % g, api.Cost(tracked[g % len(tracked)], float(rng.uniform(0.1, 1)),
                                                          aim=aim(1), axes=[axes[g % len(axes)]]))
    form.incorporate_constraint("bounds", [api.Constraint(states[0] + axes[0], 4.0),
                                           api.Constraint(states[0] + axes[0], 3.0, arrow=[-1])])
    form.identify_qp_domain([u + a for a in axes for u in inputs])
    form.make_preview_matrices()
    return form


def goal_table(form, plan):
    """The records of ``Assembler.goal_terms`` from the plan alone: (goal, first row, rows, aim's slot)."""
    recs = []
    for gi, (name, goal) in enumerate(form.goals.items()):
        aim0 = plan.param_slots[("cost", name, "aim")][0]
        for i, axis in enumerate(goal.axes):
            r0, rows = plan.pm_rows[goal.variable + axis]
            recs.append((gi, r0, rows, aim0 + i))
    return np.asarray(recs, dtype=np.int64).reshape(-1, 4), len(form.goals)


def source_strides(plan, streams):
    """``h_src_stride`` of a launch: 0 for shared streams, the block's size for bound ones; the (A, B) slots
    of a generated group carry a system per instance."""
    if streams == "shared":
        return [0] * len(plan.sources)
    if streams == "bound":
        return [int(np.prod(s.array.shape)) for s in plan.sources]
    strides = [0] * len(plan.sources)
    for g in plan.lti:
        strides[g["ids"][0]], strides[g["ids"][1]] = g["n"] * g["n"], g["n"] * g["m"]
    return strides


def compile_case(api, rng, shape, plant=None):
    from mpcasm.plan import compile_plan

    form = build(api, rng, shape, plant)
    return form, compile_plan(form, lti=("plant",) if shape.streams == "lti" else ())


# --------------------------------------------------------------------------------------------------
# References of the rows, in long double (helpers.assert_componentwise takes the pairs (x*, M))
# --------------------------------------------------------------------------------------------------
def longest_definition_row(shape):
    """e2: the entries of the longest row of a definition (a state, an input: one)."""
    widths = [2] * bool(shape.narrow) + [wide_width(shape, k) for k in range(shape.wide)]
    return max([1] + widths)


def dense_matrix(form, plan, dtype=float):
    """The oracle's dense ``[Mg | Mo]`` of every definition, rows in the plan's order (``plan.pm_rows``), from
    the horizon matrices the formulation holds."""
    from oracle import qp_oracle as orc

    PM = orc.preview_matrices(form)
    M = np.zeros((plan.pmrows, plan.ng + plan.no), dtype=dtype)
    for var, (r0, rows) in plan.pm_rows.items():
        M[r0:r0 + rows, :plan.ng], M[r0:r0 + rows, plan.ng:] = PM[var]
    return M


def dense_rows_reference(PM, given, optim):
    """Rows of instances that read fp64 ``S, U``: the long-double product of the dense fp64 ``[Mg | Mo]`` with
    ``[given ; optim]`` (``(B, ng)``, ``(B, no)``), and ``M = |Mg| |given| + |Mo| |optim|``.  A row is a sum of
    at most e2 products of sums of at most W terms: kappa = W + e2 + 2."""
    from helpers import LD

    x = np.concatenate([np.asarray(given, dtype=LD), np.asarray(optim, dtype=LD)], axis=-1)
    PM = np.asarray(PM, dtype=LD)
    return x @ PM.T, np.abs(x) @ np.abs(PM).T


def generated_rows_reference(form, name, A, B, given, optim, plan):
    """Rows of an instance whose tables are generated on chip from ``(A, B)``: everything from the plant on in
    long double (helpers.precise_reference), kappa = helpers.kappa(N, n)."""
    from helpers import precise_reference

    return precise_reference(form, name, A, B, given, optim=optim, pm_rows=plan.pm_rows)["rows"]


def distance_reference(table, ngoals, rows, mag, params, kappa):
    """``d* = sum_r (row*_r - aim)^2`` per goal in long double, and the bound of its error: the rows' bound
    pushed through one subtraction, one square and a sum of ``rows`` terms,
    ``(2 kappa + rows + 4) u sum_r (M_r + |aim|)^2``."""
    from helpers import LD, U64

    d, scale, count = np.zeros(ngoals, dtype=LD), np.zeros(ngoals, dtype=LD), np.zeros(ngoals, dtype=np.int64)
    for goal, r0, n, slot in table:
        aim = LD(params[slot])
        v = rows[r0:r0 + n] - aim
        d[goal] += np.sum(v * v)
        w = mag[r0:r0 + n] + abs(aim)
        scale[goal] += np.sum(w * w)
        count[goal] += n
    return d, (2 * kappa + count + 4) * LD(U64) * scale
