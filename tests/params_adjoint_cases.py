"""What the CPU and GPU tests of the assembly's derivative with respect to the parameters
(mpcasm_assemble_params_vjp, csrc/adjoint.hip) share beside adjoint_cases.py  --  TEST INFRASTRUCTURE ONLY: the
coverage the limit fields need on top of adjoint_cases.assert_coverage, kappa counted from the plan's tables, and the
per-instance set-up of a case (parameters, sources, long-double Jacobians)."""
import numpy as np

import adjoint_cases as ac
from adjoint_cases import LM_CENTER_P, LM_CENTER_ROWS, LM_EXTREME_P, LM_EXTREME_ROWS
from mpcasm import plan as P

WIDEST = 10     # rounded operations of the widest contribution (a row of a gterm with a Hessian part, below)


def assert_coverage(plans):
    """adjoint_cases.assert_coverage, and the row counts of the centre and the extreme: a limit with one row of each
    (broadcast over its lines) and a limit with a row of extreme per line."""
    ac.assert_coverage(plans)
    _, limits = ac.records(plans["mix-shared"])
    assert any(rec[ac.LM_NROWS] > 1 and rec[LM_CENTER_ROWS] == 1 and rec[LM_EXTREME_ROWS] == 1 for rec, _ in limits)
    assert any(rec[ac.LM_NROWS] > 1 and rec[LM_EXTREME_ROWS] == rec[ac.LM_NROWS] for rec, _ in limits)
    assert any(rec[ac.LM_NROWS] > 1 and rec[ac.LM_ARROW_ROWS] == rec[ac.LM_NROWS] and rec[LM_CENTER_ROWS] == 1
               for rec, _ in limits), "an arrow per line against one row of centre"


def build_centres(api, rng):
    """adjoint_cases' ``diag`` formulation with the two kinds of limit its ``mix`` lacks: a centre per line under an
    arrow of one row (two axes), and arrow, centre and extreme all per line."""
    form = ac.build(api, rng, "diag")
    form.incorporate_constraint("centre rows", api.Constraint(
        "s1", 1.5, axes=ac.AXES, arrow=[0.8, -1.2], center=rng.uniform(-1, 1, (ac.N, 2))))
    form.incorporate_constraint("all rows", api.Constraint(
        "s2_b", rng.uniform(1, 2, (3, 1)), arrow=rng.uniform(-2, 2, (3, 1)), center=rng.uniform(-1, 1, (3, 1)),
        schedule=range(2, 5)))
    return form


def assert_centres_coverage(plan):
    _, limits = ac.records(plan)
    n = lambda rec: rec[ac.LM_NROWS]
    assert any(n(rec) > 1 and rec[ac.LM_NAXES] == 2 and rec[ac.LM_ARROW_ROWS] == 1 and rec[LM_CENTER_ROWS] == n(rec)
               for rec, _ in limits), "a centre per line under an arrow of one row"
    assert any(n(rec) > 1 and rec[ac.LM_ARROW_ROWS] == rec[LM_CENTER_ROWS] == rec[LM_EXTREME_ROWS] == n(rec)
               for rec, _ in limits), "arrow, centre and extreme per line"


def contributions(plan):
    """Per parameter slot the rows (gterms) and lines (limits) summed into it."""
    gt, limits = ac.records(plan)
    count = np.zeros(max(len(plan.params), 1), dtype=np.int64)
    for g in gt:
        count[g[ac.GT_WPARAM]] += g[ac.GT_NROWS]
        count[g[ac.GT_AIMPARAM]] += g[ac.GT_NROWS]
    for rec, axes in limits:
        n, naxes = int(rec[ac.LM_NROWS]), int(rec[ac.LM_NAXES])
        for first, rows, width in ((rec[ac.LM_ARROW_P], rec[ac.LM_ARROW_ROWS], naxes),
                                   (rec[LM_CENTER_P], rec[LM_CENTER_ROWS], naxes),
                                   (rec[LM_EXTREME_P], rec[LM_EXTREME_ROWS], 1)):
            if rows == 1:
                count[first:first + width] += n
            else:
                count[first:first + n * width] += 1
    return count


def kappa(plan, generated=False):
    """The rounded operations behind one element of the result, from the plan's tables, each product and each
    addition counted.  A contribution is a product of two entries of the row vectors ``r_x, r_u, r_g``, and each of
    those carries the error of its own chain -- the longest base row (step 1), the longest row of E (step 2), for
    tables generated on chip helpers.kappa(N, n) on top -- so the chain counts twice.  Then the sum: the most
    contributions to one slot times the operations of the widest contribution (a row of a gterm with a Hessian part:
    ``-1/2 (r_u r_x + r_x r_u) - s r_u (r_g - aim)``, added: 10), and the six levels of the widest butterfly."""
    it = np.asarray(plan.itab)
    nbase, rtot = int(it[P._H["NBASE"]]), int(it[P._H["RTOT"]])
    bcolptr = it[it[P._H["OFF_T_BCOLPTR"]]:][:nbase + 1]
    longest_base_row = max([int(bcolptr[b + 1] - bcolptr[b]) for b in range(nbase)] + [1])
    rowptr = it[it[P._H["OFF_ROWPTR"]]:][:rtot + 1]
    longest_row = int(np.max(np.diff(rowptr))) if rtot else 0
    chain = 2 * (longest_base_row + longest_row)
    if generated:
        from helpers import kappa as horizon_kappa

        chain += max(horizon_kappa(g["N"], g["n"]) for g in plan.lti)
    return int(2 * chain + WIDEST * int(contributions(plan).max()) + 6)
