"""The Jacobian of the assembly with respect to the parameters in long double, host only  --  TEST INFRASTRUCTURE ONLY.

``P, q, G, h`` are affine in each single parameter with the others fixed, so column ``j`` of the Jacobian is the
oracle's ``assemble`` with slot ``j`` raised by 1 minus the one without, exactly.  Both evaluations are taken at
values every format holds -- slot ``j`` at 1 and at 0 -- because ``theta_j + 1`` rounds in fp64 and the difference
would then be the column times ``fl(theta_j + 1) - theta_j``, no longer the column; by affinity it is the same
difference.  The slot is set through the Cost and Constraint objects (``plan.current_params()`` is asserted to move in
slot ``j`` alone, by 1; an aim that a non-crossed cost shares between its two roles moves as one).  The same
difference in the oracle's ``magnitude=True`` mode (``|1| - |0|``) is the column's magnitude.  By default the
difference is taken on the term of the one Cost or Constraint that owns the slot (the oracle's ``qp_cost`` /
``qp_constraint``; see :func:`jacobian`), ``whole=True`` on the whole ``assemble``.  For the cotangent that
``(x, u, y, w)`` stand for (include/mpcasm.h), formed densely in long double,

    gP = -1/2 (u x' + x u')     gq = -u     gG_R = -(y_R u' + w_R x')     gh = w

the reference is ``g*_j = <gP, dP_j> + gq'dq_j + <gG, dG_j> + gh'dh_j`` and ``M_j`` the same with absolute values
throughout.
"""
from collections import namedtuple
from contextlib import contextmanager

import numpy as np

import adjoint_reference as ar
from helpers import LD

ParamJacobian = namedtuple("ParamJacobian", "dP dq dG dh MP Mq MG Mh")   # each (n_params, ...) in long double


def slot_table(form, plan):
    """Per parameter slot ``(object, field, flat index in the field)``, or None for a slot no field owns."""
    from oracle import qp_oracle as orc

    limits = orc.all_limits(form)
    table = [None] * len(plan.params)
    for (kind, name, field), (start, rows, cols) in plan.param_slots.items():
        obj = form.goals[name] if kind == "cost" else limits[name]
        for i in range(rows * cols):
            assert table[start + i] is None
            table[start + i] = (obj, field, i)
    return table


@contextmanager
def slot_set(entry, value):
    """The Cost / Constraint object with one slot at ``value`` for the time being."""
    obj, field, i = entry
    if field == "weight":
        saved = {"weight": obj.weight}
        obj.weight = float(value)
    else:
        fields = [field]
        if field == "aim" and getattr(obj, "cross_aim", None) is obj.aim:    # (a plain cost: its twin follows)
            fields.append("cross_aim")
        saved = {f: getattr(obj, f) for f in fields}
        new = np.array(saved[field], dtype=float)
        new.reshape(-1)[i] = value
        for f in fields:
            setattr(obj, f, new)
    try:
        yield
    finally:
        for f, old in saved.items():
            setattr(obj, f, old)


def _horizon(form, magnitude, name, tables, plant):
    """The horizon matrices of an instance's own plant (adjoint_reference.jacobian's two ways), or None."""
    from oracle import qp_oracle as orc

    if plant is not None:
        A, B = (np.abs(m) if magnitude else np.asarray(m) for m in plant)
        N = form.dynamics[name].matrices[-1].shape[0]
        S, U = orc.extend_matrices(N, A, B, dtype=LD)
        return list(U) + [S]
    if tables is not None:
        S, U = tables
        return [np.asarray(u) for u in U] + [np.asarray(S)]
    return None


def _own_term(form, plan, entry, PM, g, magnitude):
    """``(G, h, P, q)`` of the one Cost or Constraint that owns a slot, by the oracle's ``qp_cost`` /
    ``qp_constraint``, each at its place in the stacked QP: what ``assemble`` adds up, less the terms of the other
    objects."""
    from oracle import qp_oracle as orc

    obj = entry[0]
    no, nc = plan.no, plan.nc
    G, h = np.zeros((nc, no), dtype=LD), np.zeros((nc, 1), dtype=LD)
    P, q = np.zeros((no, no), dtype=LD), np.zeros((no, 1), dtype=LD)
    limits = orc.all_limits(form)
    if any(obj is l for l in limits):
        idx = [obj is l for l in limits].index(True)
        out0, rows = plan.limit_rows[idx]
        G[out0:out0 + rows], h[out0:out0 + rows] = orc.qp_constraint(PM, obj, g, dtype=LD, magnitude=magnitude)
    else:
        P, q = orc.qp_cost(PM, obj, g, dtype=LD, magnitude=magnitude)
    return G, h, P, q


def jacobian(form, plan, given, name=None, tables=None, plant=None, whole=False):
    """The :class:`ParamJacobian` of ``form`` as it stands at ``given``; sources as adjoint_reference.jacobian.

    ``whole``: every column as the difference of the whole ``assemble``.  The default differences the term of the
    one Cost or Constraint that owns the slot (the oracle's own ``qp_cost`` / ``qp_constraint``, which ``assemble``
    adds up): the other objects' terms do not move and cancel, but in the whole difference they leave their
    rounding behind -- 2^-64 of the whole assembly, which for a badly scaled plant is many orders above a column --
    and the reference has to be far better than the yardstick it serves."""
    from oracle import qp_oracle as orc

    table = slot_table(form, plan)
    base = plan.current_params()
    g = np.asarray(given, dtype=float).reshape(-1, 1) if form.given_len else np.zeros((0, 1))
    out = []
    for magnitude in (False, True):
        mats = _horizon(form, magnitude, name, tables, plant)
        with ar.horizon_matrices(form, name if mats is not None else None, mats):
            PM = orc.preview_matrices(form, dtype=LD, magnitude=magnitude)
            entry = None
            if whole:
                at = lambda: orc.assemble(form, g, PM=PM, dtype=LD, magnitude=magnitude)
            else:
                at = lambda: _own_term(form, plan, entry, PM, g, magnitude)
            cols = None
            for j, entry in enumerate(table):
                if entry is None:
                    continue
                with slot_set(entry, 0.0):
                    low, p0 = at(), plan.current_params()
                with slot_set(entry, 1.0):
                    high, p1 = at(), plan.current_params()
                moved = p1 - p0
                assert moved[j] == 1.0 and np.count_nonzero(moved) == 1, (j, moved)
                assert np.array_equal(np.delete(p0, j), np.delete(base, j)), j
                if cols is None:
                    cols = [np.zeros((len(table),) + np.shape(m), dtype=LD) for m in low]
                for col, hi, lo in zip(cols, high, low):
                    col[j] = hi - lo
            G, h, P, q = cols
            out.extend([P, q[:, :, 0], G, h[:, :, 0]])
    assert np.array_equal(plan.current_params(), base)
    return ParamJacobian(*out)


def forward_magnitude(form, given, name=None, tables=None, plant=None):
    """``(M_G, M_h, M_P, M_q)`` of ``assemble(form, given)``: the oracle's magnitude mode, sources as :func:`jacobian`."""
    from oracle import qp_oracle as orc

    mats = _horizon(form, True, name, tables, plant)
    g = np.asarray(given, dtype=float).reshape(-1, 1) if form.given_len else np.zeros((0, 1))
    with ar.horizon_matrices(form, name if mats is not None else None, mats):
        G, h, P, q = orc.assemble(form, g, dtype=LD, magnitude=True)
    return G, h.ravel(), P, q.ravel()


def cotangents(x, u, y, w):
    """``((gP, gq, gG, gh), (|gP|, |gq|, |gG|, |gh|))`` in long double, the magnitudes of the formation."""
    x, u, y, w = (np.asarray(v, dtype=LD) for v in (x, u, y, w))
    ax, au, ay, aw = (np.abs(v) for v in (x, u, y, w))
    value = (-(np.outer(u, x) + np.outer(x, u)) / 2, -u, -(np.outer(y, u) + np.outer(w, x)), w)
    mag = ((np.outer(au, ax) + np.outer(ax, au)) / 2, au, np.outer(ay, au) + np.outer(aw, ax), aw)
    return value, mag


def contract(cot, dP, dq, dG, dh):
    """``<gP, dP_j> + gq'dq_j + <gG, dG_j> + gh'dh_j`` for every ``j`` of the leading axis."""
    gP, gq, gG, gh = cot
    return (np.tensordot(dP, gP, 2) + dq @ gq + np.tensordot(dG, gG, 2) + dh @ gh).astype(LD)


def vjp_reference(J, x, u, y, w):
    """``(gparams*, M)`` for one instance."""
    value, mag = cotangents(x, u, y, w)
    return contract(value, J.dP, J.dq, J.dG, J.dh), contract(mag, J.MP, J.Mq, J.MG, J.Mh)


def dense_gradient(form, plan, given, x, u, y, w):
    """``gparams`` composed per Cost and Constraint from the oracle's dense preview matrices in long double -- the
    formulas of include/mpcasm.h written per object, independent of ``assemble`` -- and its magnitude."""
    from oracle import qp_oracle as orc

    out = []
    for magnitude in (False, True):
        dat = (lambda v: np.abs(np.asarray(v, dtype=LD))) if magnitude else (lambda v: np.asarray(v, dtype=LD))
        sgn = LD(1) if magnitude else LD(-1)
        PM = orc.preview_matrices(form, dtype=LD, magnitude=magnitude)
        g = dat(given).reshape(-1)
        x_, u_, y_, w_ = (dat(v).reshape(-1) for v in (x, u, y, w))
        grad = np.zeros(len(plan.params), dtype=LD)
        for name, cost in form.goals.items():
            wp = plan.param_slots[("cost", name, "weight")][0]
            ap = plan.param_slots[("cost", name, "aim")][0]
            cp = plan.param_slots.get(("cost", name, "cross_aim"), (ap,))[0]
            wt, aim, caim = dat(cost.weight), dat(cost.aim), dat(cost.cross_aim)
            for i, axis in enumerate(cost.axes):
                vMg, vMo = PM[cost.variable + axis]
                cMg, cMo = PM[cost.cross + axis]
                picked = cost.schedule if cost.schedule else range(vMg.shape[0])
                vMg, vMo, cMg, cMo = (M[picked] for M in (vMg, vMo, cMg, cMo))
                if cost.L:
                    vMg, vMo = dat(cost.L[i]) @ vMg, dat(cost.L[i]) @ vMo
                if cost.cross_L:
                    cMg, cMo = dat(cost.cross_L[i]) @ cMg, dat(cost.cross_L[i]) @ cMo
                rxv, ruv, rxc, ruc = vMo @ x_, vMo @ u_, cMo @ x_, cMo @ u_
                dv, dc = vMg @ g + sgn * aim[0, i], cMg @ g + sgn * caim[0, i]      # (V_g given - aim, as a sum)
                # P += w vMo'cMo against gP;  q += w/2 (vMo'dc + cMo'dv) against gq = -u
                grad[wp] += sgn * (ruv @ rxc + rxv @ ruc) / 2 + sgn * (ruv @ dc + ruc @ dv) / 2
                grad[cp + i] += wt * np.sum(ruv) / 2
                grad[ap + i] += wt * np.sum(ruc) / 2
        for idx, limit in enumerate(orc.all_limits(form)):
            naxes = len(limit.axes)
            slots = {f: plan.param_slots[("limit", idx, f)] for f in ("arrow", "center", "extreme")}
            arrow, center = dat(limit.arrow).reshape(-1, naxes), dat(limit.center).reshape(-1, naxes)
            out0, nlines = plan.limit_rows[idx]
            for i, axis in enumerate(limit.axes):
                Mg, Mo = PM[limit.variable + axis]
                picked = limit.schedule if limit.schedule else range(Mg.shape[0])
                Mg, Mo = Mg[picked], Mo[picked]
                if limit.L:
                    Mg, Mo = dat(limit.L[i]) @ Mg, dat(limit.L[i]) @ Mo
                rx, ru, rg = (np.broadcast_to(v, (nlines,)) for v in (Mo @ x_, Mo @ u_, Mg @ g))
                for l in range(nlines):
                    R = out0 + l
                    a = slots["arrow"][0] + (0 if slots["arrow"][1] == 1 else l) * naxes + i
                    c = slots["center"][0] + (0 if slots["center"][1] == 1 else l) * naxes + i
                    al, cl = arrow[0 if arrow.shape[0] == 1 else l, i], center[0 if center.shape[0] == 1 else l, i]
                    # G_R = sum arrow V_o[row] against gG_R;  h_R = extreme + arrow (center - r_g) against gh_R = w_R
                    grad[a] += sgn * (y_[R] * ru[l] + w_[R] * rx[l]) + w_[R] * (cl + sgn * rg[l])
                    grad[c] += w_[R] * al
            for l in range(nlines):
                grad[slots["extreme"][0] + (0 if slots["extreme"][1] == 1 else l)] += w_[out0 + l]
        out.append(grad)
    return tuple(out)
