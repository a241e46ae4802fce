"""The shift map of a receding-horizon loop's warm start: where every unknown and every row of this tick's QP
was in the QP of the tick before (``mpcasm_qp_warm_start``'s ``col_src`` and ``row_src``, include/mpcasm.h).

Between two ticks the horizon moves on by one sample, so sample ``k`` of the new preview was sample ``k + 1``
of the old one; when the walker's clock wrapped in between, the first previewed step has been taken and step
``j`` of the new preview was step ``j + 1``.  The structure may change with it (the biped: 34 <-> 36 unknowns,
72 <-> 76 rows).  Host only: no device needed."""
import numpy as np


def horizon_of(form):
    """The samples of the horizon as :func:`shift_map` sees them: the size of the largest unknown."""
    return max((form.domain[v] for v in form.optim_variables), default=0)


def limit_rows(form):
    """Rows of every limit of ``form`` in the order of ``G``'s rows (named constraints, then boxes): the
    compiled plan's ``limit_rows``."""
    from .plan import compile_plan

    return [int(n) for _, n in compile_plan(form).limit_rows]


def _shifted(n):
    """``k -> k + 1`` with the last entry repeating the previous last."""
    return np.minimum(np.arange(n) + 1, n - 1)


def shift_map(prev, new, step_left, horizon=None, prev_rows=None, new_rows=None):
    """``(col_src, row_src)``, int32: for every unknown and every row of ``G`` of ``new`` its place in ``prev``,
    or -1.  ``prev`` and ``new`` are formulations as updated for two consecutive ticks; ``step_left``: the
    clock wrapped between the two, so the first previewed step of ``prev`` has been taken.

    Unknowns, matched by variable name through ``optim_ID``: a variable with one entry per sample of the horizon
    (``horizon`` entries in both; by default :func:`horizon_of`) takes ``k + 1``, its last entry the previous
    last; any other variable counts as one entry per previewed step and takes ``j + 1`` when ``step_left``, else
    ``j``; an entry without a counterpart takes -1.
    Rows, limits matched by position in the order of ``G``'s rows (``prev_rows``, ``new_rows``: the rows of every
    limit, by default :func:`limit_rows`): the same row count and one row per sample: shifted like the samples;
    the same row count otherwise: copied; another row count: -1.
    A variable or limit that cannot be matched gives -1 entries, never an error."""
    N = int(horizon_of(new) if horizon is None else horizon)
    col = np.full(new.optim_len, -1, dtype=np.int32)
    for var, cols in new.optim_ID.items():
        if var not in prev.optim_ID:
            continue
        old = prev.optim_ID[var]
        n_new, n_old = len(cols), len(old)
        if n_new == N and n_old == N:
            src = _shifted(N)
        else:
            src = np.arange(n_new) + (1 if step_left else 0)
        ok = src < n_old
        col[np.arange(cols.start, cols.stop)[ok]] = old.start + src[ok]
    prev_rows = limit_rows(prev) if prev_rows is None else [int(n) for n in prev_rows]
    new_rows = limit_rows(new) if new_rows is None else [int(n) for n in new_rows]
    row = np.full(sum(new_rows), -1, dtype=np.int32)
    at_new = at_old = 0
    for i, n in enumerate(new_rows):
        if i < len(prev_rows):
            if prev_rows[i] == n:
                row[at_new:at_new + n] = at_old + (_shifted(n) if n == N else np.arange(n))
            at_old += prev_rows[i]
        at_new += n
    return col, row

