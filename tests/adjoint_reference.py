"""The Jacobian of the assembly with respect to ``given`` in long double, host only  --  TEST INFRASTRUCTURE ONLY.

``q`` and ``h`` are affine in ``given``, so column ``j`` of ``J = [J_q ; J_h]`` is ``assemble(form, e_j)`` minus
``assemble(form, 0)`` of the oracle, exactly (to long-double rounding); the same call with ``magnitude=True`` adds
where the value subtracts, so the same difference is the column's magnitude ``|J|``.  References and magnitudes:

    VJP   ggiven* = J_q' gq + J_h' gh        M = |J_q|' |gq| + |J_h|' |gh|
    JVP   dq* = J_q d,  dh* = J_h d          M = |J_q| |d|,  |J_h| |d|
"""
from collections import namedtuple
from contextlib import contextmanager

import numpy as np

from helpers import LD

Jacobian = namedtuple("Jacobian", "Jq Jh Mq Mh")


@contextmanager
def horizon_matrices(form, name, matrices):
    """``form`` with the horizon matrices ``[U_0, .., U_{m-1}, S]`` of the dynamics ``name`` for the time being."""
    if name is None:
        yield
        return
    dyn = form.dynamics[name]
    saved = list(dyn.matrices)
    try:
        dyn.matrices = list(matrices)
        dyn.update_definitions()
        yield
    finally:
        dyn.matrices = saved
        dyn.update_definitions()


def _columns(form, magnitude):
    from oracle import qp_oracle as orc

    ng = form.given_len
    PM = orc.preview_matrices(form, dtype=LD, magnitude=magnitude)
    at = lambda g: orc.assemble(form, g, PM=PM, dtype=LD, magnitude=magnitude)
    _, h0, _, q0 = at(np.zeros((ng, 1)))
    no, nc = q0.shape[0], h0.shape[0]
    Jq, Jh = np.zeros((no, ng), dtype=LD), np.zeros((nc, ng), dtype=LD)
    for j in range(ng):
        e = np.zeros((ng, 1))
        e[j] = 1.0
        _, h, _, q = at(e)
        Jq[:, j], Jh[:, j] = (q - q0).ravel(), (h - h0).ravel()
    return Jq, Jh


def jacobian(form, name=None, tables=None, plant=None):
    """The :class:`Jacobian` of ``form`` as it stands (its weights and arrows).  ``name``: a dynamics whose horizon
    matrices are an instance's own -- ``tables = (S, U)``, the fp64 arrays the kernel reads (``U`` stacked), or
    ``plant = (A, B)`` for tables generated on chip: everything from the plant on in long double, the magnitude from
    ``|A|, |B|`` (helpers.precise_reference's way)."""
    from oracle import qp_oracle as orc

    out = []
    for magnitude in (False, True):
        mats = None
        if plant is not None:
            A, B = (np.abs(x) if magnitude else np.asarray(x) for x in plant)
            N = form.dynamics[name].matrices[-1].shape[0]
            S, U = orc.extend_matrices(N, A, B, dtype=LD)
            mats = list(U) + [S]
        elif tables is not None:
            S, U = tables
            mats = [np.asarray(u) for u in U] + [np.asarray(S)]
        with horizon_matrices(form, name if mats is not None else None, mats):
            out.extend(_columns(form, magnitude))
    Jq, Jh, Mq, Mh = out
    return Jacobian(Jq, Jh, Mq, Mh)


def forward_magnitude(form, given, name=None, tables=None, plant=None):
    """``(M_q, M_h)`` of ``assemble(form, given)``: the oracle's magnitude mode, sources as for :func:`jacobian`."""
    from oracle import qp_oracle as orc

    mats = None
    if plant is not None:
        N = form.dynamics[name].matrices[-1].shape[0]
        S, U = orc.extend_matrices(N, np.abs(plant[0]), np.abs(plant[1]), dtype=LD)
        mats = list(U) + [S]
    elif tables is not None:
        mats = [np.asarray(u) for u in tables[1]] + [np.asarray(tables[0])]
    with horizon_matrices(form, name if mats is not None else None, mats):
        _, h, _, q = orc.assemble(form, np.asarray(given, dtype=float).reshape(-1, 1), dtype=LD, magnitude=True)
    return q.ravel(), h.ravel()


def vjp_reference(J, gq, gh):
    """``(ggiven*, M)`` for one instance; a None cotangent is zero."""
    ng = J.Jq.shape[1]
    ref, mag = np.zeros(ng, dtype=LD), np.zeros(ng, dtype=LD)
    if gq is not None:
        g = np.asarray(gq, dtype=LD)
        ref, mag = ref + J.Jq.T @ g, mag + J.Mq.T @ np.abs(g)
    if gh is not None:
        g = np.asarray(gh, dtype=LD)
        ref, mag = ref + J.Jh.T @ g, mag + J.Mh.T @ np.abs(g)
    return ref, mag


def jvp_reference(J, d):
    """``((dq*, M), (dh*, M))`` for one instance."""
    d = np.asarray(d, dtype=LD)
    return (J.Jq @ d, J.Mq @ np.abs(d)), (J.Jh @ d, J.Mh @ np.abs(d))


def dense_jacobian(form):
    """``J_q = sum s w cMo_a' cMg_b`` and ``J_h = -sum_i diag(arrow_i) cMg_i`` composed from the oracle's dense
    preview matrices in long double -- the formulas of include/mpcasm.h, independent of ``assemble``."""
    from oracle import qp_oracle as orc

    PM = orc.preview_matrices(form, dtype=LD)
    ng = form.given_len
    Jq = None
    for cost in form.goals.values():
        w = LD(cost.weight)
        for i, axis in enumerate(cost.axes):
            vMg, vMo = PM[cost.variable + axis]
            cMg, cMo = PM[cost.cross + axis]
            picked = cost.schedule if cost.schedule else range(vMg.shape[0])
            vMg, vMo, cMg, cMo = (M[picked] for M in (vMg, vMo, cMg, cMo))
            if cost.L:
                L = np.asarray(cost.L[i], dtype=LD)
                vMg, vMo = L @ vMg, L @ vMo
            if cost.cross_L:
                L = np.asarray(cost.cross_L[i], dtype=LD)
                cMg, cMo = L @ cMg, L @ cMo
            term = w * (vMo.T @ cMg + cMo.T @ vMg) / 2
            Jq = term if Jq is None else Jq + term
    blocks = []
    for limit in orc.all_limits(form):
        arrow = np.asarray(limit.arrow, dtype=LD).reshape(-1, len(limit.axes))
        rows = PM[limit.variable + limit.axes[0]][0].shape[0]
        nlines = orc.constraint_nlines(limit)
        block = np.zeros((rows if nlines is None else nlines, ng), dtype=LD)
        picked = limit.schedule if limit.schedule else range(rows)
        for i, axis in enumerate(limit.axes):
            Mg = PM[limit.variable + axis][0][picked]
            if limit.L:
                Mg = np.asarray(limit.L[i], dtype=LD) @ Mg
            block -= arrow[:, i][:, None] * Mg
        blocks.append(block)
    return Jq, (np.vstack(blocks) if blocks else np.zeros((0, ng), dtype=LD))
