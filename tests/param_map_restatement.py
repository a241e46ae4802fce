"""Host restatement of a parameter map (``mpcasm_params_map``, include/mpcasm.h)  --  TEST INFRASTRUCTURE ONLY.

The records as the header states them, in numpy float64, every operation rounded on its own and in the kernel's
order: ``t = c1 * sign`` (a signed record), ``v = t * command``, ``c0 + v`` (a record with a constant).  What the
kernel gives must match this bit for bit."""
import numpy as np

SIGNED, CONST = 1, 2      # MPCASM_PMAP_SIGNED, MPCASM_PMAP_CONST


def apply_map(params, recs, coef, cmd, index=None, sign=None, count=None, ncmd=None):
    """``params`` ``(rows, n_params)`` with the records applied to its first ``count`` rows (a copy; default: all
    rows).  ``cmd``: ``(rows, >= ncmd)`` command table, or 1-D: one row shared by all (cmd_stride == 0);
    ``ncmd``: the columns a record may name (default: the table's width).  ``index[b]``: the command row of
    instance ``b`` (None: ``b``); ``sign[b]``: its factor (None: a signed record writes nothing).  A record with
    ``dst`` or ``col`` out of range or an unknown flag writes nothing."""
    out = np.array(params, dtype=np.float64, copy=True)
    n_params = out.shape[1]
    recs = np.asarray(recs, dtype=np.int64).reshape(-1, 4)
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 2)
    cmd = np.asarray(cmd, dtype=np.float64)
    shared = cmd.ndim == 1
    ncmd = cmd.shape[-1] if ncmd is None else int(ncmd)
    count = out.shape[0] if count is None else int(count)
    rows = np.arange(count) if index is None else np.asarray(index, dtype=np.int64)[:count]
    for (dst, col, flags, _), (c0, c1) in zip(recs, coef):
        if not (0 <= dst < n_params and 0 <= col < ncmd) or flags & ~(SIGNED | CONST):
            continue
        if flags & SIGNED and sign is None:
            continue
        c = np.broadcast_to(cmd[col], (count,)) if shared else cmd[rows, col]
        t = c1 * np.asarray(sign, dtype=np.float64)[:count] if flags & SIGNED else np.full(count, c1)
        v = t * c
        out[:count, dst] = c0 + v if flags & CONST else v
    return out
