"""What the CPU and GPU tests of the assembly's derivative (mpcasm_assemble_jvp / _vjp, csrc/adjoint.hip) share  --
TEST INFRASTRUCTURE ONLY: small formulations which together hold every kind of record the operator walks, the
properties asserted on the compiled plan so that the coverage cannot rot silently, and kappa from the plan's tables.

``mix``: one plant (3 states, 1 input, N = 6) on two axes, a bias ``n`` in ``given``, an output ``y`` that combines
states and the bias, a one-row given variable ``p``, a given variable ``idle`` nothing reads, and
  costs   plain (y, two axes) | crossed (s2_a x s0_b: two GT_FLAG_HALF terms) | with L | with a schedule |
          on a free variable (the input itself: GT_FLAG_DIAG)
  limits  with L | with a schedule | two axes, arrow of one row | arrow of nrows rows |
          one row of ``p`` broadcast over three lines
``diag``: the same plant with a cost on the free variable only: J_q = 0, dq exactly 0.
Each for the three stream kinds of preview_cases.py (shared, bound, lti)."""
from collections import namedtuple

import numpy as np

from mpcasm._tables import VALUES
from mpcasm.plan import (GT_FLAG_DIAG, GT_FLAG_HALF, GT_WORDS, LM_WORDS, LX_WORDS)

N, NS, NI = 6, 3, 1
AXES = ["_a", "_b"]
STREAMS = ("shared", "bound", "lti")
Case = namedtuple("Case", "name kind streams")
CASES = [Case("%s-%s" % (kind, streams), kind, streams) for kind in ("mix", "diag") for streams in STREAMS]
IDS = [c.name for c in CASES]

# word offsets inside a gterm, a limit and a limit-axis record
globals().update({n: VALUES[n] for n in (
    "GT_AOFF GT_BOFF GT_NROWS GT_WPARAM GT_DOFF GT_AIMPARAM GT_FLAGS LX_ROWOFF LX_ROWS LM_OUT0 LM_NROWS LM_NAXES LM_LAX0 "
    "LM_ARROW_P LM_ARROW_ROWS LM_CENTER_P LM_CENTER_ROWS LM_EXTREME_P LM_EXTREME_ROWS").split()})


def build(api, rng, kind, plant=None):
    """The Formulation ``kind``; ``plant``: the nominal ``(A, B)`` (default: a random stable one)."""
    from mpcasm import problems

    A, B = problems.random_lti_matrices(rng, NS, NI) if plant is None else plant
    states, inputs = ["s%d" % i for i in range(NS)], ["u0"]
    ext = api.ExtendedSystem.from_cotrol_system(api.ControlSystem(inputs, states, A, B, axes=AXES), "x", N)
    form = api.Formulation()
    form.incorporate_dynamics("plant", ext)
    form.incorporate_dynamics("bias", api.DomainVariable("n", N, AXES))
    form.incorporate_dynamics("point", api.DomainVariable("p", 1, ["_a"]))
    form.incorporate_dynamics("idle", api.DomainVariable("idle", 2, ["_a"]))
    shift = np.diag(np.ones(N - 1), 1)
    form.incorporate_definitions({
        "y" + a: api.LineCombo({"s0" + a: 1.3, "n" + a: shift, "s1" + a: -0.7}) for a in AXES})
    u = lambda k: [float(v) for v in rng.uniform(-1.0, 1.0, k)]
    form.incorporate_goal("free", api.Cost("u0", 0.01, aim=u(2), axes=AXES))
    if kind == "mix":
        form.incorporate_goal("plain", api.Cost("y", 0.7, aim=u(2), axes=AXES))
        form.incorporate_goal("crossed", api.Cost("s2_a", 1.1, aim=0.4, cross="s0_b", cross_aim=0.3,
                                                  cross_L=np.eye(N)))
        form.incorporate_goal("with L", api.Cost("s1", 0.5, aim=u(1), axes=["_a"], L=rng.uniform(-1, 1, (2, N))))
        form.incorporate_goal("scheduled", api.Cost("s0", 0.9, aim=u(1), axes=["_b"], schedule=range(2, 5)))
        form.incorporate_constraint("with L", api.Constraint("s0_a", 4.0, L=rng.uniform(-1, 1, (2, N))))
        form.incorporate_constraint("scheduled", api.Constraint("s1_b", 3.0, arrow=[-1.5], schedule=range(1, 4)))
        form.incorporate_constraint("two axes", api.Constraint("y", 2.0, axes=AXES, arrow=[1.0, -0.5],
                                                               center=[0.1, 0.2]))
        form.incorporate_constraint("arrow rows", api.Constraint("s2", 5.0, axes=AXES,
                                                                 arrow=rng.uniform(-2, 2, (N, 2))))
        form.incorporate_constraint("broadcast", api.Constraint("p", np.array([[1.0], [2.0], [3.0]]), axes=["_a"],
                                                                arrow=np.array([[1.0], [-1.0], [0.5]])))
    else:
        form.incorporate_constraint("bound", api.Constraint("s0_a", 4.0))
    form.identify_qp_domain(["u0" + a for a in AXES])
    form.make_preview_matrices()
    return form


def compile_case(api, rng, case, plant=None):
    from mpcasm.plan import compile_plan

    form = build(api, rng, case.kind, plant)
    return form, compile_plan(form, lti=("plant",) if case.streams == "lti" else ())


def vary_params(form, rng):
    """Other weights and arrows (both signs) in the Cost and Constraint objects: ``plan.current_params()`` and the
    oracle read the same instance afterwards."""
    from oracle import qp_oracle as orc

    for cost in form.goals.values():
        cost.weight = float(cost.weight * rng.uniform(0.5, 2.0))
    for limit in orc.all_limits(form):
        shape = np.shape(limit.arrow)
        limit.arrow = np.asarray(limit.arrow, dtype=float) * rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)


def plant_sources(plan, S, U, name="plant"):
    """The plan's sources with the horizon matrices of ``name`` replaced by ``S (N, n, n)``, ``U (m, N, N, n)``."""
    out = []
    for s in plan.sources:
        if isinstance(s.key, tuple) and s.key[0] == name:
            out.append(np.ascontiguousarray(U[s.key[1]] if s.key[1] < len(U) else S, dtype=np.float64))
        else:
            out.append(s.array)
    return out


def records(plan):
    """``(gterms, limits)`` of a compiled plan: gterm records as rows of GT_WORDS words; per limit
    ``(record, [axis records])``."""
    from mpcasm import plan as P

    it = np.asarray(plan.itab)
    gt = it[it[P._H["OFF_GTERM"]]:][:it[P._H["NGTERM"]] * GT_WORDS].reshape(-1, GT_WORDS)
    lm = it[it[P._H["OFF_LIMIT"]]:][:it[P._H["NLIMIT"]] * LM_WORDS].reshape(-1, LM_WORDS)
    lx = it[it[P._H["OFF_LAX"]]:][:it[P._H["NLAX"]] * LX_WORDS].reshape(-1, LX_WORDS)
    return gt, [(rec, lx[rec[LM_LAX0]:rec[LM_LAX0] + rec[LM_NAXES]]) for rec in lm]


def assert_coverage(plans):
    """The cases together hold every kind of record (``plans``: name -> plan)."""
    gt, limits = records(plans["mix-shared"])
    flags = gt[:, GT_FLAGS]
    plain = gt[(flags & (GT_FLAG_DIAG | GT_FLAG_HALF)) == 0]
    assert len(plain) >= 4, "plain costs (two axes), a cost with L, a cost with a schedule"
    assert np.count_nonzero(flags & GT_FLAG_HALF) == 2, "a crossed cost: two halved terms"
    assert np.count_nonzero(flags & GT_FLAG_DIAG) == 2, "a cost on a free variable, per axis"
    assert {2, 3, N} <= set(int(n) for n in plain[:, GT_NROWS]), "rows of L, of a schedule, of the whole horizon"
    rows = {int(rec[LM_NROWS]) for rec, _ in limits}
    assert {2, 3, N} <= rows, "a limit with L (2 lines), with a schedule (3), over the horizon"
    assert any(rec[LM_NAXES] == 2 and rec[LM_ARROW_ROWS] == 1 for rec, _ in limits), "two axes, arrow of one row"
    assert any(rec[LM_NAXES] == 2 and rec[LM_ARROW_ROWS] == N for rec, _ in limits), "arrow of nrows rows"
    assert any(rec[LM_NROWS] == 3 and all(ax[:, LX_ROWS] == 1) for rec, ax in limits), \
        "an axis row-set of one row broadcast over three lines"
    gt, _ = records(plans["diag-shared"])
    assert len(gt) and np.all(gt[:, GT_FLAGS] & GT_FLAG_DIAG), "a plan whose every cost is on a free variable"
    for streams in STREAMS:
        assert len(plans["mix-" + streams].lti) == (streams == "lti")


def build_no_given(api, rng):
    """The plant alone with its initial state among the unknowns: ``ng == 0``."""
    from mpcasm import problems

    A, B = problems.random_lti_matrices(rng, NS, NI)
    states = ["s%d" % i for i in range(NS)]
    ext = api.ExtendedSystem.from_cotrol_system(api.ControlSystem(["u0"], states, A, B, axes=AXES), "x", N)
    form = api.Formulation()
    form.incorporate_dynamics("plant", ext)
    form.incorporate_goal("plain", api.Cost("s0", 0.7, aim=[0.1, 0.2], axes=AXES))
    form.incorporate_constraint("bound", api.Constraint("s1_a", 4.0))
    form.identify_qp_domain(["x0" + a for a in AXES] + ["u0" + a for a in AXES])
    form.make_preview_matrices()
    return form


def forward_kappa(plan, generated=False):
    """The rounded operations behind an element of ``q`` or ``h`` of the assembly kernels: a workspace element (the
    longest row of E), ``d = V_g given`` (ng terms), then the sum over every row of every gterm (at most RTOT products
    of three factors)."""
    from mpcasm import plan as P

    it = np.asarray(plan.itab)
    rtot = int(it[P._H["RTOT"]])
    rowptr = it[it[P._H["OFF_ROWPTR"]]:][:rtot + 1]
    k = 2 * ((int(np.max(np.diff(rowptr))) if rtot else 0) + plan.ng + rtot) + 8
    if generated:
        from helpers import kappa as horizon_kappa

        k += max(horizon_kappa(g["N"], g["n"]) for g in plan.lti)
    return int(k)


def unread_given_columns(form):
    """The columns of ``given`` that belong to ``idle``: no definition a cost or a limit uses reads them."""
    return [int(i) for i in form.given_ID["idle_a"]]


def kappa(plan, info=None, generated=False):
    """The rounded operations on the longest path of the operator's six steps, from the plan's tables: the longest
    base row over either half of the columns (steps 1 and 6 read the same tables, one along rows, one along
    columns: the longest transposed list is the base rows that cover one column), the longest row of E and the
    longest column of E (steps 2 and 5), the most contributions to a rho row (gterms, and for the VJP limit axes) and
    the axes of a row of h, each product and each addition counted, plus the three roundings of ``s w`` and the
    sign; for tables generated on chip helpers.kappa(N, n) on top."""
    from mpcasm import plan as P

    it = np.asarray(plan.itab)
    nbase, ng, no, rtot = int(it[P._H["NBASE"]]), plan.ng, plan.no, int(it[P._H["RTOT"]])
    brow0 = it[it[P._H["OFF_T_BROW0"]]:][:nbase + 1]
    bcolptr = it[it[P._H["OFF_T_BCOLPTR"]]:][:nbase + 1]
    bcols = it[it[P._H["OFF_T_BCOLS"]]:][:bcolptr[nbase]]
    longest_base_row = max([int(bcolptr[b + 1] - bcolptr[b]) for b in range(nbase)] + [1])
    cover = np.zeros(ng + no, dtype=np.int64)
    for b in range(nbase):
        cover[bcols[bcolptr[b]:bcolptr[b + 1]]] += brow0[b + 1] - brow0[b]
    rowptr = it[it[P._H["OFF_ROWPTR"]]:][:rtot + 1]
    nent = int(rowptr[rtot])
    entbase, entk = it[it[P._H["OFF_ENTBASE"]]:][:nent], it[it[P._H["OFF_ENTK"]]:][:nent]
    longest_row = int(np.max(np.diff(rowptr))) if rtot else 0
    longest_col = int(np.max(np.bincount(brow0[entbase] + entk))) if nent else 0
    gt, limits = records(plan)
    contrib = np.zeros(max(rtot, 1), dtype=np.int64)
    for g in gt:
        if not g[GT_FLAGS] & GT_FLAG_DIAG:
            contrib[g[GT_AOFF]:g[GT_AOFF] + g[GT_NROWS]] += 1
            contrib[g[GT_DOFF]:g[GT_DOFF] + g[GT_NROWS]] += 1
    axes = 0
    for rec, ax in limits:
        axes = max(axes, int(rec[LM_NAXES]))
        for off, rows in ax:
            span = slice(off, off + 1) if rows == 1 else slice(off, off + rec[LM_NROWS])
            contrib[span] += rec[LM_NROWS] if rows == 1 else 1
    k = 2 * (longest_base_row + longest_row + int(contrib.max()) + axes + longest_col + int(cover.max())) + 4
    if generated:
        from helpers import kappa as horizon_kappa

        k += max(horizon_kappa(g["N"], g["n"]) for g in plan.lti)
    return int(k)
