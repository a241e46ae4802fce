"""An fp64 numpy restatement of csrc/adjoint.hip's six steps from the plan's tables  --  TEST INFRASTRUCTURE ONLY,
in the style of plan_emulator.py: it proves the reading of the tables (column tables, row program, gterm and limit
records) without a GPU.  The transposed products are taken as transposes here; the kernel gathers them through an
index derived from the same tables.

    JVP  y = Bm_g d, r = E y, dh_R = -sum_i arrow_Ri r[row_i(R)], rho[a+k] += s w r[dd+k], yt = E' rho, dq = Bm_o' yt
    VJP  y = Bm_o gq, r = E y, rho[dd+k] += s w r[a+k], rho[row_i(R)] -= arrow_Ri gh_R, yt = E' rho, ggiven = Bm_g' yt
"""
import numpy as np

import plan_emulator as em
from mpcasm import plan as P

H = P._H
GT_AOFF, GT_BOFF, GT_NROWS, GT_WPARAM, GT_DOFF, GT_AIMPARAM, GT_FLAGS = range(7)
LM_OUT0, LM_NROWS, LM_NAXES, LM_LAX0, LM_ARROW_P, LM_ARROW_ROWS = range(6)


def operators(plan, sources=None, ab=None):
    """``(Bm, E)`` dense: the base rows over [given | unknowns] read through the column tables (``sources``: the
    instance's streams, default the plan's own; ``ab``: the (A, B) of every generated group), and the row program."""
    it, dt = plan.itab, plan.dtab
    assert it[H["T_CI_OK"]] == 1
    srcs = [s.array for s in plan.sources] if sources is None else sources
    streams = em._tiled_streams(plan, srcs, ab or [])
    nbase, ng, no, nop = int(it[H["NBASE"]]), plan.ng, plan.no, int(it[H["T_NOP"]])
    brow0 = em._section(it, "OFF_T_BROW0", nbase + 1)
    nbrow = int(brow0[-1])
    cig = em._section(it, "OFF_T_CIG", nbase * ng * 2).reshape(nbase, ng, 2)
    cio = em._section(it, "OFF_T_CIO", nbase * nop * 2).reshape(nbase, nop, 2)
    bcolptr = em._section(it, "OFF_T_BCOLPTR", nbase + 1)
    bcols = em._section(it, "OFF_T_BCOLS", bcolptr[-1])
    Bm = np.zeros((nbrow, ng + no))
    for b in range(nbase):
        for c in bcols[bcolptr[b]:bcolptr[b + 1]]:
            off, word = (int(v) for v in (cig[b, c] if c < ng else cio[b, c - ng]))
            stream, rs = streams[(word & 0xFFFFFFFF) >> 24], int(em._sext24(word))
            for k in range(brow0[b + 1] - brow0[b]):
                Bm[brow0[b] + k, c] = stream[off + k * rs]
    rtot = int(it[H["RTOT"]])
    rowptr = em._section(it, "OFF_ROWPTR", rtot + 1)
    nent = int(rowptr[-1])
    entbase, entk = em._section(it, "OFF_ENTBASE", nent), em._section(it, "OFF_ENTK", nent)
    coef = dt[it[H["DOFF_ENTCOEF"]]:it[H["DOFF_ENTCOEF"]] + nent]
    E = np.zeros((rtot, nbrow))
    for r in range(rtot):
        for e in range(rowptr[r], rowptr[r + 1]):
            E[r, brow0[entbase[e]] + entk[e]] += coef[e]
    return Bm, E


def _records(plan):
    it = plan.itab
    gt = em._section(it, "OFF_GTERM", it[H["NGTERM"]] * P.GT_WORDS).reshape(-1, P.GT_WORDS)
    lm = em._section(it, "OFF_LIMIT", it[H["NLIMIT"]] * P.LM_WORDS).reshape(-1, P.LM_WORDS)
    lx = em._section(it, "OFF_LAX", it[H["NLAX"]] * P.LX_WORDS).reshape(-1, P.LX_WORDS)
    return gt, lm, lx


def _limit_axes(lm, lx):
    """(row of h, workspace row, arrow's parameter slot) of every axis of every line of every limit."""
    for rec in lm:
        naxes = int(rec[LM_NAXES])
        for i in range(rec[LM_NROWS]):
            for ax in range(naxes):
                off, rows = lx[rec[LM_LAX0] + ax]
                yield (int(rec[LM_OUT0] + i), int(off + (0 if rows == 1 else i)),
                       int(rec[LM_ARROW_P] + (0 if rec[LM_ARROW_ROWS] == 1 else i) * naxes + ax))


def jvp(plan, d, params=None, sources=None, ab=None):
    """``(dq, dh)`` of one instance."""
    params = plan.params if params is None else params
    Bm, E = operators(plan, sources, ab)
    gt, lm, lx = _records(plan)
    ng = plan.ng
    r = E @ (Bm[:, :ng] @ np.asarray(d, dtype=float))
    dh = np.zeros(plan.nc)
    for R, row, slot in _limit_axes(lm, lx):
        dh[R] -= params[slot] * r[row]
    rho = np.zeros(E.shape[0])
    for g in gt:
        if g[GT_FLAGS] & P.GT_FLAG_DIAG:
            continue
        sw = (0.5 if g[GT_FLAGS] & P.GT_FLAG_HALF else 1.0) * params[g[GT_WPARAM]]
        n = g[GT_NROWS]
        rho[g[GT_AOFF]:g[GT_AOFF] + n] += sw * r[g[GT_DOFF]:g[GT_DOFF] + n]
    return Bm[:, ng:].T @ (E.T @ rho), dh


def vjp(plan, gq, gh, params=None, sources=None, ab=None):
    """``ggiven`` of one instance; a None cotangent is zero."""
    params = plan.params if params is None else params
    Bm, E = operators(plan, sources, ab)
    gt, lm, lx = _records(plan)
    ng = plan.ng
    rho = np.zeros(E.shape[0])
    if gq is not None:
        r = E @ (Bm[:, ng:] @ np.asarray(gq, dtype=float))
        for g in gt:
            if g[GT_FLAGS] & P.GT_FLAG_DIAG:
                continue
            sw = (0.5 if g[GT_FLAGS] & P.GT_FLAG_HALF else 1.0) * params[g[GT_WPARAM]]
            n = g[GT_NROWS]
            rho[g[GT_DOFF]:g[GT_DOFF] + n] += sw * r[g[GT_AOFF]:g[GT_AOFF] + n]
    if gh is not None:
        for R, row, slot in _limit_axes(lm, lx):
            rho[row] -= params[slot] * gh[R]
    return Bm[:, :ng].T @ (E.T @ rho)
