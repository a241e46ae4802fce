"""CPU oracle for the QP-assembly hot path  --  TEST INFRASTRUCTURE ONLY.

This module is a numpy restatement of the reference's algorithm for the path
``Formulation.update() -> make_preview_matrices() -> generate_all_qp_matrices()``
plus ``tools.extend_matrices``.  It is the checker the HIP kernels are compared
with.  Only ``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline``
leg of ``bench.py`` may import it; nothing under ``mpc-interface_amd/`` does,
and the product path never routes through it.

Parity pinned: every function here is checked against outputs of the real
reference (imported in the build container by ``tests/golden/make_golden.py``)
and against the reference's own fixture ``python/tests/LIP_matrices``; see
``tests/test_oracle_golden.py``.  The LTV generalisation (per-step ``A_k, B_k``)
has no reference counterpart and is pinned only in the degenerate LTI case
("parity unpinned" beyond that).

The functions are duck-typed on the reference's attribute names
(``definitions``, ``of``, ``dynamics``, ``goals``, ``constraints``,
``constraint_boxes``, ``domain`` ...), so they run unchanged on reference
objects (to pin the oracle) and on this repository's mirror classes.

Each function cites the reference lines it follows, relative to
``/root/reference/python/mpc_interface/``.
"""
import numpy as np


# --------------------------------------------------------------------------
# a1  tools.extend_matrices                                   tools.py:14-33
# --------------------------------------------------------------------------
def extend_matrices(N, A, B, dtype=float):
    """``S[k, j, i] = (A^{k+1})[i, j]``, ``U[j][k, l, i] = (A^{k-l} B)[i, j]``.

    Same recurrence as tools.py:23-29 (left-multiply the previous block row by
    ``A``; no repeated squaring), written per block instead of per stacked row.
    ``dtype``: the arithmetic (``np.longdouble`` for the tests' precise reference).
    """
    A = np.asarray(A, dtype=dtype)
    B = np.asarray(B, dtype=dtype)
    n, m = B.shape

    S = np.zeros([N, n, n], dtype=dtype)
    U = [np.zeros([N, N, n], dtype=dtype) for _ in range(m)]

    power = A.copy()                     # A^{k+1}
    blocks = [B.copy()]                  # blocks[d] = A^d B, built by A.dot(previous)
    for k in range(N):
        if k > 0:
            power = A.dot(power)         # tools.py:29
            blocks.append(A.dot(blocks[-1]))   # tools.py:24-26 (column 0 chain)
        S[k] = power.T
        for l in range(k + 1):
            AB = blocks[k - l]
            for j in range(m):
                U[j][k, l, :] = AB[:, j]
    return S, U


def extend_matrices_ltv(N, A_steps, B_steps, dtype=float):
    """Per-step dynamics ``x_{k+1} = A_k x_k + B_k u_k``.

    ``S[k] = (A_k ... A_0)^T``, ``U[j][k, l, :] = (A_k ... A_{l+1} B_l)[:, j]``.
    Generalisation used by BASELINE config C5; equals :func:`extend_matrices`
    when all steps share one ``(A, B)`` (the only case the reference has,
    dynamics.py:222-231).
    """
    A_steps = np.asarray(A_steps, dtype=dtype)
    B_steps = np.asarray(B_steps, dtype=dtype)
    n, m = B_steps.shape[1:]
    S = np.zeros([N, n, n], dtype=dtype)
    U = [np.zeros([N, N, n], dtype=dtype) for _ in range(m)]
    row = np.zeros([N, n, m], dtype=dtype)   # row[l] = A_k..A_{l+1} B_l for the current k
    power = np.eye(n, dtype=dtype)
    for k in range(N):
        power = A_steps[k].dot(power)
        S[k] = power.T
        for l in range(k):
            row[l] = A_steps[k].dot(row[l])
        row[k] = B_steps[k]
        for l in range(k + 1):
            for j in range(m):
                U[j][k, l, :] = row[l][:, j]
    return S, U


# --------------------------------------------------------------------------
# a3  domain / index maps                                    body.py:97-136
# --------------------------------------------------------------------------
def qp_index_maps(domain, optim_variables):
    """Sizes and ``range`` index maps of the QP unknowns and givens.

    ``domain`` is the ordered ``{variable: size}`` dict; givens are the domain
    variables not listed as unknowns, in domain order (body.py:101-106); IDs
    are prefix sums (body.py:123-133).
    """
    given_variables = [v for v in domain.keys() if v not in optim_variables]

    def ranges(names):
        out, start = {}, 0
        for name in names:
            out[name] = range(start, start + domain[name])
            start += domain[name]
        return out, start

    optim_ID, optim_len = ranges(optim_variables)
    given_ID, given_len = ranges(given_variables)
    return {
        "optim_variables": list(optim_variables),
        "given_variables": given_variables,
        "optim_ID": optim_ID,
        "given_ID": given_ID,
        "optim_len": optim_len,
        "given_len": given_len,
    }


# --------------------------------------------------------------------------
# a4  preview matrices                                      body.py:149-193
# --------------------------------------------------------------------------
def _datum(x, dtype, magnitude):
    """``x`` in the arithmetic ``dtype``; its absolute value for the magnitude of the result."""
    x = np.asarray(x, dtype=dtype)
    return np.abs(x) if magnitude else x


def preview_matrices(form, maps=None, dtype=float, magnitude=False):
    """``PM[var] = (Mg, Mo)`` for every definition, in definition order.

    ``dtype``: the arithmetic.  ``magnitude=True``: the same sums over the absolute values of the
    coefficients (the componentwise bound of the rounding errors, with ``|S|``, ``|U|`` in the
    dynamics' matrices).
    """
    if maps is None:
        maps = qp_index_maps(form.domain, form.optim_variables)
    ng, no = maps["given_len"], maps["optim_len"]
    PM = {}
    for var, combo in form.definitions.items():
        if var in form.of:                                  # body.py:158-177
            rows = form.dynamics[form.of[var]].all_variables[var]
            Mg, Mo = np.zeros([rows, ng], dtype=dtype), np.zeros([rows, no], dtype=dtype)
            for dep, coef in combo.items():
                if magnitude:
                    coef = np.abs(np.asarray(coef, dtype=dtype))
                if dep in maps["given_variables"]:
                    Mg[:, maps["given_ID"][dep]] = coef
                elif dep in maps["optim_variables"]:
                    Mo[:, maps["optim_ID"][dep]] = coef
                else:
                    raise ValueError(
                        "The variable {} in the definition of {} seems to not "
                        "be given nor optimal.".format(dep, var)
                    )
        else:                                               # body.py:179-193
            Mg = Mo = None
            for dep, coef in combo.items():
                c = np.array(coef) if dtype is float else np.array(coef, dtype=dtype)
                if magnitude:
                    c = np.array(np.abs(c))
                tg, to = c.dot(PM[dep][0]), c.dot(PM[dep][1])
                if Mg is None:
                    Mg, Mo = tg, to
                    if Mg.ndim == 1:
                        Mg, Mo = Mg[None, :], Mo[None, :]
                else:
                    Mg += tg
                    Mo += to
        PM[var] = (Mg, Mo)
    return PM


def arrange_given(maps, collector):
    """Scatter the collector's column vectors by ``given_ID`` (body.py:195-207)."""
    if not maps["given_len"]:
        return np.array([])
    given = np.zeros([maps["given_len"], 1])
    for var, ids in maps["given_ID"].items():
        given[ids] = collector[var]
    return given


# --------------------------------------------------------------------------
# a6  constraint row rule, coefficients and bound    restrictions.py:147-199
# --------------------------------------------------------------------------
def constraint_nlines(limit):
    if limit.L:
        return limit.L[0].shape[0]
    if limit.schedule:
        return limit.schedule.stop - limit.schedule.start
    rows = [limit.arrow.shape[0], limit.center.shape[0], limit.extreme.shape[0]]
    wide = [r for r in rows if r != 1]
    return wide[0] if wide else None


def constraint_coefficients(limit, dtype=float, magnitude=False):
    arrow = _datum(limit.arrow, dtype, magnitude)
    cols = [arrow[:, i][:, None] for i in range(len(limit.axes))]
    if limit.L:
        return [c * _datum(l, dtype, magnitude) for c, l in zip(cols, limit.L)]
    return cols


def constraint_bound(limit, dtype=float, magnitude=False):
    arrow, center = _datum(limit.arrow, dtype, magnitude), _datum(limit.center, dtype, magnitude)
    return _datum(limit.extreme, dtype, magnitude) + np.sum(arrow * center, axis=1).reshape([-1, 1])


# --------------------------------------------------------------------------
# a7  one constraint                                        body.py:236-264
# --------------------------------------------------------------------------
def qp_constraint(PM, limit, given, dtype=float, magnitude=False):
    """``magnitude=True``: absolute values of the data, ``bound + cMg given`` (``PM`` and ``given``
    of the magnitude too)."""
    Mg0 = PM[limit.variable + limit.axes[0]][0]
    rows = Mg0.shape[0]
    nlines = constraint_nlines(limit)
    out_rows = rows if nlines is None else nlines
    ng = Mg0.shape[1]
    no = PM[limit.variable + limit.axes[0]][1].shape[1]

    cMg, cMo = np.zeros([out_rows, ng], dtype=dtype), np.zeros([out_rows, no], dtype=dtype)
    picked = limit.schedule if limit.schedule else range(rows)
    coefs = constraint_coefficients(limit, dtype, magnitude)
    for i, axis in enumerate(limit.axes):
        Mg, Mo = PM[limit.variable + axis]
        if limit.L:
            cMg += coefs[i] @ Mg[picked]
            cMo += coefs[i] @ Mo[picked]
        else:
            cMg += coefs[i] * Mg[picked]
            cMo += coefs[i] * Mo[picked]
    given = _datum(given, dtype, magnitude)
    if magnitude:
        return cMo, constraint_bound(limit, dtype, True) + cMg @ given
    return cMo, constraint_bound(limit, dtype) - cMg @ given


# --------------------------------------------------------------------------
# a9  one cost                                              body.py:266-302
# --------------------------------------------------------------------------
def qp_cost(PM, cost, given, dtype=float, magnitude=False):
    """``magnitude=True``: absolute values of the data, both differences ``... given - aim`` as sums
    (``PM`` and ``given`` of the magnitude too)."""
    first = PM[cost.variable + cost.axes[0]]
    rows, no = first[0].shape[0], first[1].shape[1]
    Q, q = np.zeros([no, no], dtype=dtype), np.zeros([no, 1], dtype=dtype)
    picked = cost.schedule if cost.schedule else range(rows)
    given = _datum(given, dtype, magnitude)
    weight = cost.weight if dtype is float and not magnitude else _datum(cost.weight, dtype, magnitude)
    aim, cross_aim = _datum(cost.aim, dtype, magnitude), _datum(cost.cross_aim, dtype, magnitude)
    sign = 1 if magnitude else -1

    for i, axis in enumerate(cost.axes):
        vMg, vMo = (M[picked] for M in PM[cost.variable + axis])
        cMg, cMo = (M[picked] for M in PM[cost.cross + axis])
        if cost.L:
            L = _datum(cost.L[i], dtype, magnitude)
            vMg, vMo = L @ vMg, L @ vMo
        if cost.cross_L:
            L = _datum(cost.cross_L[i], dtype, magnitude)
            cMg, cMo = L @ cMg, L @ cMo

        Q += weight * vMo.T @ cMo                            # (w vMo^T) @ cMo
        q += (
            weight
            * (vMo.T @ (cMg @ given + sign * cross_aim[:, i])
               + cMo.T @ (vMg @ given + sign * aim[:, i]))
            / 2
        )
    return Q, q


# --------------------------------------------------------------------------
# a8, a10, a11  stacking                                    body.py:304-348
# --------------------------------------------------------------------------
def all_limits(form):
    """Constraint order of the stacked G: named constraints, then boxes."""
    limits = [l for group in form.constraints.values() for l in group]
    limits += [l for box in form.constraint_boxes.values() for l in box.constraints]
    return limits


def qp_all_constraints(form, PM, given, dtype=float, magnitude=False):
    parts = [qp_constraint(PM, limit, given, dtype, magnitude) for limit in all_limits(form)]
    return np.vstack([p[0] for p in parts]), np.vstack([p[1] for p in parts])


def qp_all_costs(form, PM, given, dtype=float, magnitude=False):
    parts = [qp_cost(PM, cost, given, dtype, magnitude) for cost in form.goals.values()]
    return (np.add.reduce([p[0] for p in parts]),
            np.add.reduce([p[1] for p in parts]))


def assemble(form, given, PM=None, maps=None, dtype=float, magnitude=False):
    """``(A, h, Q, q)`` = qpsolvers ``(G, h, P, q)`` (body.py:333-348).

    ``dtype``: the arithmetic.  ``magnitude=True``: the componentwise magnitude of every result,
    the same sums over the absolute values of every datum with the three differences as sums.
    """
    if maps is None:
        maps = qp_index_maps(form.domain, form.optim_variables)
    if PM is None:
        PM = preview_matrices(form, maps, dtype, magnitude)
    A, h = qp_all_constraints(form, PM, given, dtype, magnitude)
    Q, q = qp_all_costs(form, PM, given, dtype, magnitude)
    return A, h, Q, q


def preview(PM, given, optim, variable, axes=None, dtype=float, magnitude=False):
    """``Mg @ given + Mo @ optim`` (body.py:209-219); ``magnitude=True``: over absolute values."""
    if dtype is not float or magnitude:
        given, optim = _datum(given, dtype, magnitude), _datum(optim, dtype, magnitude)
        PM = {v: (_datum(Mg, dtype, magnitude), _datum(Mo, dtype, magnitude)) for v, (Mg, Mo) in PM.items()}
    if axes is None:
        Mg, Mo = PM[variable]
        return Mg @ given + Mo @ optim
    return np.hstack(
        [PM[variable + a][0] @ given + PM[variable + a][1] @ optim for a in axes]
    )
