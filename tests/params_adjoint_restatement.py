"""An fp64 numpy restatement of mpcasm_assemble_params_vjp (csrc/adjoint.hip) from the plan's tables  --  TEST
INFRASTRUCTURE ONLY, in the style of adjoint_restatement.py: the three row vectors through the column tables and the
row program, then the parameter index -- per slot its records, the gterms in the plan's order, then the limits by line
and axis -- built here from the gterm, limit and limit-axis records as params_adjoint_build_index builds it, and
walked slot by slot.

    r_x = E (Bm_o x),  r_u = E (Bm_o u),  r_g = E (Bm_g given)
    weight of a gterm   [P] -1/2 sum (r_u[a+k] r_x[b+k] + r_x[a+k] r_u[b+k]) - s sum r_u[a+k] (r_g[dd+k] - aim)
    aim of a gterm      s w sum r_u[a+k]
    diagonal gterm      weight: sum coef_k u_c (aim - coef_k x_c);  aim: w sum coef_k u_c
    limit, line R       arrow: -(y_R r_u[row] + w_R r_x[row]) + w_R (center - r_g[row]);  center: w_R arrow;  extreme: w_R
"""
import numpy as np

import adjoint_restatement as rs
from mpcasm import plan as P

H = P._H
GT_AOFF, GT_BOFF, GT_NROWS, GT_WPARAM, GT_DOFF, GT_AIMPARAM, GT_FLAGS = range(7)
(LM_OUT0, LM_NROWS, LM_NAXES, LM_LAX0, LM_ARROW_P, LM_ARROW_ROWS, LM_CENTER_P, LM_CENTER_ROWS, LM_EXTREME_P,
 LM_EXTREME_ROWS) = range(10)


def parameter_index(plan):
    """Per slot the list of its records ``(kind, rows, fields...)`` in the kernel's order."""
    gt, lm, lx = rs._records(plan)
    it = plan.itab
    index = [[] for _ in range(len(plan.params))]
    for g in gt:
        a, b, n, wp, dd, ap, flags = (int(v) for v in g[:7])
        if flags & P.GT_FLAG_DIAG:
            coef0 = int(it[H["DOFF_DIAGCOEF"]]) + b
            index[wp].append(("diag weight", n, a, coef0, ap))
            index[ap].append(("diag aim", n, a, coef0, wp))
            continue
        s = 0.5 if flags & P.GT_FLAG_HALF else 1.0
        index[wp].append(("weight", n, a, b if flags & P.GT_FLAG_P else None, dd, ap, s))
        index[ap].append(("aim", n, a, wp, s))
    for rec in lm:
        out0, nr, naxes = int(rec[LM_OUT0]), int(rec[LM_NROWS]), int(rec[LM_NAXES])
        a1, c1, e1 = (int(rec[k]) == 1 for k in (LM_ARROW_ROWS, LM_CENTER_ROWS, LM_EXTREME_ROWS))
        astep, cstep = (0 if a1 else naxes), (0 if c1 else naxes)
        for i in range(nr):
            for ax in range(naxes):
                off, rows = (int(v) for v in lx[rec[LM_LAX0] + ax])
                rstep = 0 if rows == 1 else 1
                arrow0, center0 = int(rec[LM_ARROW_P]) + ax, int(rec[LM_CENTER_P]) + ax
                if not a1 or i == 0:
                    first, n = (0, nr) if a1 else (i, 1)
                    index[arrow0 + first * astep].append(
                        ("arrow", n, out0 + first, off + first * rstep, rstep, center0 + first * cstep, cstep))
                if not c1 or i == 0:
                    first, n = (0, nr) if c1 else (i, 1)
                    index[center0 + first * cstep].append(("center", n, out0 + first, arrow0 + first * astep, astep))
            if not e1 or i == 0:
                first, n = (0, nr) if e1 else (i, 1)
                index[int(rec[LM_EXTREME_P]) + (0 if e1 else first)].append(("extreme", n, out0 + first))
    return index


def params_vjp(plan, given, x, u, y, w, params=None, sources=None, ab=None):
    """``gparams`` of one instance."""
    th = np.asarray(plan.params if params is None else params, dtype=float)
    Bm, E = rs.operators(plan, sources, ab)
    ng = plan.ng
    x, u, y, w = (np.asarray(v, dtype=float) for v in (x, u, y, w))
    rx, ru = E @ (Bm[:, ng:] @ x), E @ (Bm[:, ng:] @ u)
    rg = E @ (Bm[:, :ng] @ np.asarray(given, dtype=float)) if ng else np.zeros(E.shape[0])
    dt = plan.dtab
    out = np.zeros(len(th))
    for slot, records in enumerate(parameter_index(plan)):
        acc = 0.0
        for kind, n, *f in records:
            k = np.arange(n)
            if kind == "weight":
                a, b, dd, ap, s = f
                if b is not None:
                    acc += float(np.sum(-0.5 * (ru[a + k] * rx[b + k] + rx[a + k] * ru[b + k])))
                acc += float(np.sum(-s * ru[a + k] * (rg[dd + k] - th[ap])))
            elif kind == "aim":
                a, wp, s = f
                acc += s * th[wp] * float(np.sum(ru[a + k]))
            elif kind == "diag weight":
                c0, coef0, ap = f
                cf = dt[coef0 + k]
                acc += float(np.sum(cf * u[c0 + k] * (th[ap] - cf * x[c0 + k])))
            elif kind == "diag aim":
                c0, coef0, wp = f
                acc += th[wp] * float(np.sum(dt[coef0 + k] * u[c0 + k]))
            elif kind == "arrow":
                R0, row0, rstep, center0, cstep = f
                R, row = R0 + k, row0 + k * rstep
                acc += float(np.sum(-(y[R] * ru[row] + w[R] * rx[row]) + w[R] * (th[center0 + k * cstep] - rg[row])))
            elif kind == "center":
                R0, arrow0, astep = f
                acc += float(np.sum(w[R0 + k] * th[arrow0 + k * astep]))
            else:
                acc += float(np.sum(w[f[0] + k]))
        out[slot] = acc
    return out
