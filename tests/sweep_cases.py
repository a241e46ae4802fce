"""A family of formulations that spans every variant of the sweep kernel (csrc/sweep.hip: sweep_choose picks one of
six instantiations of ltv_sweep_kernel<CPT, NS, MS, AS, PAIR>, and inside each the lines of G take one of three
paths), shared by the CPU test of the dispatch and of the bound (test_sweep_routes_cpu.py) and the GPU test of the
arithmetic (test_gpu_sweep_variants.py).

One plant ``x+ = A_k x + B_k u`` (n states, m inputs) over N steps on 1 to 4 axes, compiled with ``ltv=``; outputs
that combine two states with coefficients of both signs; a tracking cost on every state over the whole horizon; an
effort cost on one input (the diagonal term); optional costs on part of the horizon (strided, descending, a single
step); limits with an arrow each over one or two axes, on the whole horizon (``limits``), on its last three steps
(``part``), with an arrow per line (``per_line``), or none on the whole horizon at all (``late``: so many limits on
the last three steps, one more on steps 1 and 2 -- steps without a line, steps with more lines than are fetched at
once).  In the terms of the dispatch:

  unknowns  no = axes m N            CPT = 1 (no <= 256), 2 (<= 512), 4 (<= 1024); PAIR with no and N even, no <= 512
  n, m, axes = 3, 1, 2               the instantiation with these sizes as constants (CPT 1 and PAIR only)
  per_line                           some limit's arrow changes from line to line
  reg_lines                          min(4, the limits on every step), 0 with per_line
  LR                                 8, 4, 2 by CPT: lines of a step fetched at once where reg_lines == 0
"""
from collections import namedtuple

import numpy as np

AXES = ["_x", "_y", "_z", "_w"]
Route = namedtuple("Route", "cpt specialised pair per_line reg_lines lr")
# extra: schedules of costs on outputs of their own (each on every axis: a term per axis)
Shape = namedtuple("Shape", "name lipm n m N axes limits part per_line late extra")
Case = namedtuple("Case", "shape no route")

LIMIT = None        # the route of a plan the launch refuses (MPCASM_ERR_LIMIT)


def _lr(cpt):
    return {1: 8, 2: 4, 4: 2}[cpt]


def route(cpt, specialised=0, pair=0, per_line=0, reg_lines=0):
    return Route(cpt, specialised, pair, per_line, reg_lines, _lr(cpt))


def _lipm(N, no, r):
    return Case(Shape("lipm-%d" % N, N, 3, 1, N, 2, 0, False, False, 0, ()), no, r)


def _case(name, n, m, N, axes, r, limits=0, part=False, per_line=False, late=0, extra=()):
    return Case(Shape(name, None, n, m, N, axes, limits, part, per_line, late, tuple(extra)), axes * m * N, r)


CASES = [
    # problems.lipm_ltv: 4 limits on every step, 4 more at the last one
    _lipm(33, 66, route(1, specialised=1, reg_lines=4)),                  # (odd N, two axes: the 8-byte zero-fill)
    _lipm(128, 256, route(2, specialised=1, pair=1, reg_lines=4)),        # (every thread of the block a pair)
    _lipm(129, 258, route(2, reg_lines=4)),                               # (the first width past 256, odd N)
    _case("one-1-1-1", 1, 1, 1, 1, route(1)),                             # (one thread live; no limit at all)
    _case("one-4-4-63", 4, 4, 63, 1, route(1, reg_lines=4), limits=10),   # (10 lines a step: 4 regular + 6)
    _case("one-perline", 4, 3, 85, 1, route(1, per_line=1), per_line=True),
    _case("pair-a3", 4, 1, 40, 3, route(2, pair=1, reg_lines=2), limits=2),
    _case("terms>8", 3, 2, 12, 2, route(2, pair=1, reg_lines=1), limits=1, part=True,
          extra=[range(1 + t, 12, 1 + t % 3) for t in range(5)] + [range(3, 12, 2)]),   # (12 terms on part of the horizon)
    _case("desc", 3, 2, 12, 2, route(2, pair=1, reg_lines=1), limits=1, extra=[range(11, 2, -2)]),
    _case("one-step", 3, 2, 13, 1, route(1, reg_lines=1), limits=1, part=True, extra=[range(12, 13)]),
    _case("two-n1", 1, 4, 65, 1, route(2, reg_lines=3), limits=3),
    _case("two-a3", 3, 1, 129, 3, route(2, reg_lines=4), limits=6),
    _case("four-a4-n2", 2, 2, 65, 4, route(4, reg_lines=4), limits=4, extra=[range(5, 60, 3), range(0, 65, 2)]),
    _case("four-a4-n4", 4, 4, 33, 4, route(4, reg_lines=3), limits=3),    # (naxes n n = 64: the limit)
    _case("four-lines", 2, 4, 131, 1, route(4, reg_lines=4), limits=5, part=True),
    _case("four-noreg", 2, 4, 131, 1, route(4, per_line=1), limits=1, part=True, per_line=True),
    _case("four-full", 3, 1, 256, 4, route(4)),                           # (the widest plan: 1024 unknowns)
    _case("over", 3, 1, 257, 4, LIMIT),
    # no limit on the whole horizon and none with an arrow per line: reg_lines == 0, weights per limit, steps without
    # a line, LR + 1 lines on each of the last three steps
    _case("one-late", 3, 2, 21, 1, route(1), late=9),
    _case("two-late", 1, 4, 65, 1, route(2), late=5),
    _case("pair-late", 3, 2, 12, 2, route(2, pair=1), late=5),
    _case("four-late", 2, 4, 131, 1, route(4), late=3),
    # an arrow per line on the two widths the table above leaves out
    _case("pair-perline", 3, 2, 12, 2, route(2, pair=1, per_line=1), limits=5, per_line=True),
    _case("two-perline", 1, 4, 65, 1, route(2, per_line=1), limits=5, per_line=True),
    # the instantiations with n, m, axes = 3, 1, 2 as constants on limits problems.lipm_ltv does not have
    _case("lipm-pair-late", 3, 1, 12, 2, route(2, specialised=1, pair=1), late=5),
    _case("lipm-pair-perline", 3, 1, 12, 2, route(2, specialised=1, pair=1, per_line=1), limits=5, per_line=True),
    _case("lipm-one-late", 3, 1, 13, 2, route(1, specialised=1), late=9),
    _case("lipm-one-perline", 3, 1, 13, 2, route(1, specialised=1, per_line=1), limits=9, per_line=True),
]
BY_NAME = {c.shape.name: c for c in CASES}

# every instantiation sweep_choose can select, (CPT, specialised, PAIR), written down from the dispatch ...
INSTANTIATIONS = {(2, 1, 1), (1, 1, 0), (2, 0, 1), (1, 0, 0), (2, 0, 0), (4, 0, 0)}
# ... times the three paths of the lines of G
MODES = ("regular", "per-limit", "per-line")
SELECTABLE = {inst + (mode,) for inst in INSTANTIATIONS for mode in MODES}
# combinations no plan can select, with the reason: none -- the line mode follows from the limits alone, the
# instantiation from the sizes alone
UNREACHABLE = {}


def mode_of(r):
    return "per-line" if r.per_line else ("regular" if r.reg_lines else "per-limit")


def dynamics_name(shape):
    return "LIP" if shape.lipm else "plant"


def build(api, rng, shape, plant=None):
    """The Formulation of ``shape`` on the nominal pair ``plant = (A, B)`` (default: random)."""
    from mpcasm import problems

    if shape.lipm:
        return problems.lipm_ltv(api, N=shape.lipm)
    n, m, N = shape.n, shape.m, shape.N
    axes = AXES[:shape.axes]
    A, B = problems.random_lti_matrices(rng, n, m) if plant is None else plant
    inputs = ["u%d" % j for j in range(m)]
    states = ["s%d" % i for i in range(n)]
    ext = api.ExtendedSystem.from_cotrol_system(api.ControlSystem(inputs, states, A, B, axes=axes), "x", N)
    outputs = []

    def output(prefix):
        k = len(outputs)
        combo = {states[k % n]: float(rng.uniform(0.5, 2.0))}
        if n > 1:
            combo[states[(k + 1) % n]] = -float(rng.uniform(0.5, 2.0))
        outputs.append("%s%d" % (prefix, k))
        ext.define_output(outputs[-1], combo)
        return outputs[-1]

    limited = [output("y") for _ in range(2)] + states
    extras = [output("z") for _ in shape.extra]
    form = api.Formulation()
    form.incorporate_dynamics("plant", ext)
    aim = lambda k: [float(rng.normal()) for _ in range(k)]
    for s in states:
        form.incorporate_goal("track " + s, api.Cost(s, float(rng.uniform(0.1, 1)), aim=aim(len(axes)), axes=axes))
    for t, schedule in enumerate(shape.extra):
        form.incorporate_goal("extra %d" % t, api.Cost(extras[t], float(rng.uniform(0.1, 1)), aim=aim(len(axes)),
                                                       axes=axes, schedule=schedule))
    form.incorporate_goal("effort", api.Cost(inputs[-1], 0.3, aim=aim(1), axes=axes[:1]))

    def limit(k, **kw):
        """Limit k: over one axis, every other one over two where there are two; an arrow of its own."""
        over = [axes[k % len(axes)]]
        if len(axes) > 1 and k % 2:
            over.append(axes[(k + 1) % len(axes)])
        arrow = [float(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1.5)) for _ in over]
        return api.Constraint(limited[k % len(limited)], 2.0 + k, axes=over, arrow=arrow, center=aim(len(over)), **kw)

    limits = [limit(k) for k in range(shape.limits)]
    if shape.part:
        limits.append(limit(len(limits), schedule=range(N - 3, N)))
    for k in range(shape.late):
        limits.append(limit(len(limits), schedule=range(N - 3, N)))
    if shape.late:
        limits.append(limit(len(limits), schedule=range(1, 3)))
    if shape.per_line:
        limits.append(api.Constraint(limited[1], 3.0, axes=axes, arrow=rng.uniform(0.5, 1.5, (N, len(axes)))
                                     * rng.choice([-1.0, 1.0], (N, len(axes)))))
    if limits:
        form.incorporate_constraint("limits", limits)
    form.identify_qp_domain([u + a for a in axes for u in inputs])
    form.make_preview_matrices()
    return form


def compile_case(api, rng, shape, plant=None):
    from mpcasm.plan import compile_plan

    form = build(api, rng, shape, plant)
    return form, compile_plan(form, ltv=[dynamics_name(shape)])


def table_facts(plan):
    """What the kernel's tables hold: the axes, the cost terms on part of the horizon (more than 8: the recursion
    reads them from the table, ``in_regs`` false), their steps' strides, the most lines of G at one step."""
    from mpcasm import plan as P

    it, H = plan.itab, P._H
    N, naxes = int(it[H["SW_HORIZON"]]), int(it[H["SW_NAXES"]])
    off = int(it[H["OFF_SW_TERM"]])
    terms = np.asarray(it[off:off + int(it[H["SW_NTERM"]]) * P.SW_TERM_WORDS]).reshape(-1, P.SW_TERM_WORDS)
    partial = [t for t in terms if not (t[1] == 0 and t[2] == 1 and t[3] == N)]
    off = int(it[H["OFF_SW_GPTR"]])
    gptr = np.asarray(it[off:off + N + 1])
    return dict(axes=naxes, terms=len(terms), partial=len(partial), ksteps=sorted({int(t[2]) for t in partial}),
                most_lines=int(np.diff(gptr).max()) if N else 0, fewest_lines=int(np.diff(gptr).min()) if N else 0)


# --------------------------------------------------------------------------------------------------
# An instance's own parameters, and the formulation's objects set to them for the reference
# --------------------------------------------------------------------------------------------------
def perturb_params(plan, host, rng):
    """Every instance its own weights, aims, arrows, centres and extremes, in place in ``host (B, nparams)``:
    weights, arrows and extremes scaled (they keep their sign: a Constraint flips a negative extreme), aims and
    centres shifted."""
    B = host.shape[0]
    for (kind, name, field), (start, rows, cols) in plan.param_slots.items():
        block = host[:, start:start + rows * cols]
        if field == "weight":
            block *= rng.uniform(0.5, 2.0, [B, 1])
        elif field in ("arrow", "extreme"):
            block *= rng.uniform(0.5, 1.5, [B, 1])
        else:
            block += rng.normal(0, 0.2, block.shape)
    return host


class instance_params:
    """Context: the goals and limits of ``form`` hold row ``values`` of the parameters, then their own again."""

    def __init__(self, form, plan):
        from oracle import qp_oracle as orc

        self.slots, self.goals, self.limits = plan.param_slots, form.goals, orc.all_limits(form)
        self.saved = {key: np.array(getattr(self._obj(key), key[2])) for key in self.slots}

    def _obj(self, key):
        return self.goals[key[1]] if key[0] == "cost" else self.limits[key[1]]

    def set(self, values):
        for key, (start, rows, cols) in self.slots.items():
            value = np.asarray(values[start:start + rows * cols]).reshape(rows, cols)
            self._obj(key).update(**{key[2]: float(value[0, 0]) if key[2] == "weight" else value})

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for key, value in self.saved.items():
            self._obj(key).update(**{key[2]: float(value.ravel()[0]) if key[2] == "weight" else value})


def reference(form, name, A, B, given, want_P=True):
    """helpers.precise_reference(..., ltv=True) for every case of the family: that very function where the
    formulation has limits and ``P`` is wanted; else the same sums of the oracle in long double without the parts
    that are not there (no limit: no ``G, h``) or not affordable (``want_P`` False: ``q`` from ``S, U`` without the
    products ``Mo^T Mo``, which take a minute at 1024 unknowns -- oracle qp_cost, uncrossed:
    ``q = sum w Mo^T (Mg given - aim)``)."""
    from helpers import LD, precise_reference
    from oracle import qp_oracle as orc

    if want_P and orc.all_limits(form):
        return precise_reference(form, name, A, B, given, ltv=True)
    dyn = form.dynamics[name]
    N = dyn.matrices[-1].shape[0]
    given = np.asarray(given, dtype=float).reshape(-1, 1)
    out, saved = {}, list(dyn.matrices)
    try:
        for magnitude in (False, True):
            S, U = orc.extend_matrices_ltv(N, np.abs(A) if magnitude else A, np.abs(B) if magnitude else B, dtype=LD)
            dyn.matrices = list(U) + [S]
            dyn.update_definitions()
            PM = orc.preview_matrices(form, dtype=LD, magnitude=magnitude)
            res = {}
            if want_P:
                P, q = orc.qp_all_costs(form, PM, given, LD, magnitude)
                res.update(P=P, q=q.ravel())
            else:
                g = np.abs(given).astype(LD) if magnitude else given.astype(LD)
                q = None
                for cost in form.goals.values():
                    assert not cost.crossed and not cost.L
                    w = LD(abs(cost.weight) if magnitude else cost.weight)
                    aim = np.abs(cost.aim).astype(LD) if magnitude else np.asarray(cost.aim, dtype=LD)
                    for i, axis in enumerate(cost.axes):
                        Mg, Mo = PM[cost.variable + axis]
                        picked = list(cost.schedule) if cost.schedule else list(range(Mg.shape[0]))
                        d = Mg[picked] @ g + (aim[:, i] if magnitude else -aim[:, i]).reshape(-1, 1)
                        term = w * (Mo[picked].T @ d)
                        q = term if q is None else q + term
                res["q"] = q.ravel()
            if orc.all_limits(form):
                G, h = orc.qp_all_constraints(form, PM, given, LD, magnitude)
                res.update(G=G, h=h.ravel())
            for key, value in res.items():
                out.setdefault(key, []).append(value)
    finally:
        dyn.matrices = saved
        dyn.update_definitions()
    return {key: tuple(pair) for key, pair in out.items()}


def plants(rng, batch, shape):
    """Per-step plants of ``batch`` instances, free of cancellation (helpers.cancellation_free_plants) with Perron
    root 1.3 -- 1.25 where a long horizon (N >= 129) does not keep the premise at 1.3."""
    from helpers import cancellation_free_plants

    state = rng.bit_generator.state
    try:
        return cancellation_free_plants(rng, batch, shape.n, shape.m, 1.3, shape.N, per_step=True)
    except AssertionError:
        if shape.N < 129:
            raise
        rng.bit_generator.state = state
        return cancellation_free_plants(rng, batch, shape.n, shape.m, 1.25, shape.N, per_step=True)
