"""numpy restatement of the loops' warm start  --  TEST INFRASTRUCTURE ONLY (the checker of
``mpcasm_qp_warm_store`` / ``mpcasm_qp_warm_start`` and of ``WalkerFleet(warm=True)``).

The rule of include/mpcasm.h, instance by instance: a record is warm when its tag is the expected one, the bit of
its status is in the mask, its rho is finite and inside [1e-6, 1e6] and every value gathered through the tables
is finite; then ``x0``, ``y0`` are the gathered values (0 where a table says -1 or points outside the store),
``z0 = min(G x0, h)`` and ``rho0`` the record's; otherwise the cold start ``0, 0, min(0, h), rho_cold``.
``z0`` is given in fp64 and, beside it, ``G x0`` in long double with ``|G| |x0|``, for a componentwise check.

Also the closed warm loop of one walker: fleet_loop_reference.HostWalker's tick with the solve started from the
last tick's record through ``mpcasm.warm.shift_map``."""
import collections
import types

import numpy as np

import osqp_restatement as rs
from fleet_loop_reference import APPLIES, HostWalker, rest_given, update_given
from helpers import LD
from mpcasm import warm as shift
from oracle import qp_oracle as orc

RHO_MIN, RHO_MAX, RHO_COLD = 1e-6, 1e6, 0.1

Start = collections.namedtuple("Start", "x y z rho warm gx_ld mag")


def qp_bit(status):
    return 1 << abs(int(status))


def gather(rec, src, width):
    """``rec[src]`` with 0 where ``src`` is outside ``[0, width)`` (bit for bit where it is inside)."""
    src = np.asarray(src, dtype=np.int64)
    ok = (src >= 0) & (src < width)
    out = np.zeros(src.size)
    out[ok] = rec[src[ok]]
    return out


def warm_start(G, h, SX, SY, SR, SM, index, col_src, row_src, expect_tag, warm_mask, rho_cold=RHO_COLD):
    """One :class:`Start` per instance.  ``G (B, nc, no)``, ``h (B, nc)``; the store ``SX (R, store_no)``,
    ``SY (R, store_nc)``, ``SR (R,)``, ``SM (R, 2)`` = (status, tag); ``index`` (B,) or None."""
    B, nc, no = G.shape
    out = []
    for b in range(B):
        r = b if index is None else int(index[b])
        warm = 0 <= r < SX.shape[0]
        if warm:
            status, tag, rho = int(SM[r, 0]), int(SM[r, 1]), float(SR[r])
            warm = tag == expect_tag and abs(status) < 32 and bool(warm_mask & qp_bit(status)) and \
                np.isfinite(rho) and RHO_MIN <= rho <= RHO_MAX
        if warm:
            x0 = gather(SX[r], col_src, SX.shape[1])
            y0 = gather(SY[r], row_src, SY.shape[1]) if nc else np.zeros(0)
            warm = bool(np.isfinite(x0).all() and np.isfinite(y0).all())
        if not warm:
            out.append(Start(np.zeros(no), np.zeros(nc), np.minimum(0.0, h[b]), rho_cold, 0, None, None))
            continue
        gx = G[b].astype(LD) @ x0.astype(LD)
        mag = np.abs(G[b]).astype(LD) @ np.abs(x0).astype(LD)
        out.append(Start(x0, y0, np.minimum(G[b] @ x0, h[b]), rho, 1, gx, mag))
    return out


def warm_store(SX, SY, SR, SM, index, x, y, rho, status, tag):
    """The scatter, in place: instance b into row ``index[b]`` (None: row b), the padding zeroed; an index
    outside the store is skipped."""
    for b in range(x.shape[0]):
        r = b if index is None else int(index[b])
        if not 0 <= r < SX.shape[0]:
            continue
        SX[r] = 0.0
        SX[r, :x.shape[1]] = x[b]
        SY[r] = 0.0
        SY[r, :y.shape[1]] = y[b]
        SR[r] = rho[b]
        SM[r] = (status[b], tag)


# ---- the closed warm loop of one walker -------------------------------------------------------------------------
def structure_of(form, given):
    """What ``shift_map`` reads of ``form`` as it is updated now: a snapshot (the walker re-points one
    formulation every tick) and the rows of every limit, counted on the oracle's own constraint blocks."""
    snap = types.SimpleNamespace(optim_ID=dict(form.optim_ID), optim_len=form.optim_len,
                                 optim_variables=list(form.optim_variables), domain=dict(form.domain))
    PM = orc.preview_matrices(form)
    rows = [orc.qp_constraint(PM, limit, np.asarray(given).reshape(-1, 1))[0].shape[0]
            for limit in orc.all_limits(form)]
    return snap, rows


WarmTick = collections.namedtuple("WarmTick", "sol warm start given")


def warm_loop(form, conf, phase, ticks, policy="hold", given=None, forced=None):
    """``ticks`` ticks of one walker from rest, every solve started from the last tick's record when that was
    SOLVED (the fleet's mask), its rho kept: a list of :class:`WarmTick` (the solution, whether it started warm,
    the start ``(x0, y0, z0, rho0)`` and the ``given`` it was posed at).
    ``forced``: a callable ``(tick, given, sol, record) -> next given`` that overrides the walker's own next
    ``given`` and may rewrite ``record`` (``x``, ``y``, ``rho``, ``status``), what the next tick starts from:
    teacher forcing from a device's rows."""
    walker = HostWalker(form, conf, phase, policy)
    given = rest_given(form, conf) if given is None else np.array(given, dtype=np.float64)
    record, out = None, []
    for t in range(ticks):
        form.update(step_times=np.array(walker.clock.step_times), step_count=int(walker.clock.step_count))
        A, h, Q, q = orc.assemble(form, given.reshape(-1, 1))
        h = np.asarray(h).ravel()
        snap, rows = structure_of(form, given)
        warm = record is not None and record["status"] == rs.SOLVED and \
            np.isfinite(record["rho"]) and RHO_MIN <= record["rho"] <= RHO_MAX
        if warm:
            col, row = shift.shift_map(record["snap"], snap, record["count"] != walker.clock.step_count,
                                       prev_rows=record["rows"], new_rows=rows)
            x0, y0 = gather(record["x"], col, record["x"].size), gather(record["y"], row, record["y"].size)
            warm = bool(np.isfinite(x0).all() and np.isfinite(y0).all())
        if warm:
            start = (x0, y0, np.minimum(np.asarray(A) @ x0, h), record["rho"])
        else:
            start = (np.zeros(snap.optim_len), np.zeros(h.size), np.minimum(0.0, h), RHO_COLD)
        sol = rs.solve(Q, q, A, h, x=start[0], y=start[1], z=start[2], rho=start[3])
        out.append(WarmTick(sol, int(warm), start, given))
        record = dict(x=np.asarray(sol.x), y=np.asarray(sol.y), rho=sol.rho, status=sol.status, snap=snap,
                      rows=rows, count=walker.clock.step_count)
        if forced is not None:
            given = np.array(forced(t, given, sol, record), dtype=np.float64)
        elif sol.status in APPLIES[policy]:
            given = update_given(form, given, sol.x).ravel()
        walker.clock.tick()
    return out
