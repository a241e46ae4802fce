"""numpy restatement of the solve to tolerance with soft limits  --  TEST INFRASTRUCTURE ONLY (the checker of
``mpcasm_qp_solve_soft`` and ``mpcasm_qp_solve_wide_soft``).

The problem: ``min 1/2 x'Px + q'x + sum_i phi_i((Gx - h)_i)``; a hard row (``lin_i = +inf``) has ``phi_i`` = the
indicator of ``t <= 0``, a soft row ``phi_i(t) = 0`` for ``t <= 0`` and ``lin_i t + 1/2 quad_i t^2`` for ``t > 0``.
It is tests/osqp_restatement.py's solve -- the same stopping rules, adaptive step and ``margin`` bookkeeping, its
``check`` called as it is -- with two changes:

* the z update: with ``v = alpha zt + (1 - alpha) z + y / rho``, a hard row takes ``min(v, h)`` (oracle/admm_oracle's
  expression, in its order); a soft row takes ``v`` when ``v <= h``, else
  ``h + max(0, (rho (v - h) - lin) / (rho + quad))`` -- the minimiser of ``phi(z - h) + rho / 2 (z - v)^2``;
* the primal-infeasibility certificate: a soft row's entry of ``dy`` is 0 (``mask=False``: left in, to show what
  goes wrong without).

An instance where any ``lin_i`` is NaN or < 0, or any ``quad_i`` is NaN, < 0 or +inf: NON_CVX, NaN iterates.

:func:`slack_qp` builds the equivalent QP in ``(x, s)``: ``min ... + sum lin_i s_i + 1/2 quad_i s_i^2``,
``Gx - s <= h``, ``s >= 0``, a slack per soft row; its ``x`` and the multipliers of its first ``nc`` rows are this
problem's ``x`` and ``y``.
"""
import numpy as np

import osqp_restatement as rs
from oracle import admm_oracle as ao


def penalties_ok(lin, quad):
    with np.errstate(invalid="ignore"):
        return bool(np.all(lin >= 0.0) and np.all(quad >= 0.0) and np.all(quad < np.inf))


def admm(P, q, G, h, lin, quad, x, y, z, iters, rho=ao.RHO, sigma=ao.SIGMA, alpha=ao.ALPHA):
    """``iters`` iterations from ``(x, y, z)``: oracle/admm_oracle.admm line by line, the z update above."""
    no = P.shape[0]
    soft = np.isfinite(lin)
    M = P + sigma * np.eye(no) + rho * (G.T @ G)
    for _ in range(iters):
        xt = np.linalg.solve(M, sigma * x - q + G.T @ (rho * z - y))
        zt = G @ xt
        x = alpha * xt + (1.0 - alpha) * x
        zr = alpha * zt + (1.0 - alpha) * z
        v = zr + y / rho
        zn = np.minimum(v, h)
        over = soft & (v > h)
        if over.any():
            zn[over] = h[over] + np.maximum(0.0, (rho * (v[over] - h[over]) - lin[over]) / (rho + quad[over]))
        y = y + rho * (zr - zn)
        z = zn
    return x, y, z


def solve(P, q, G, h, lin, quad, x=None, y=None, z=None, rho=ao.RHO, sigma=ao.SIGMA, alpha=ao.ALPHA, eps_abs=1e-3,
          eps_rel=1e-3, eps_prim_inf=1e-4, eps_dual_inf=1e-4, max_iter=4000, check_every=25,
          adaptive_rho_interval=100, mask=True, rho_record=None):
    """One QP with soft rows, osqp_restatement.solve's arguments, rules and :class:`osqp_restatement.Solution`.
    ``lin``, ``quad``: scalars or ``(nc,)``.  ``rho_record``: a list that gets ``(r_p, scale_p, r_d, scale_d)`` of
    every check at which rho moved (what the new rho was computed from)."""
    P, G = np.asarray(P, dtype=np.float64), np.asarray(G, dtype=np.float64)
    q, h = np.asarray(q, dtype=np.float64).ravel(), np.asarray(h, dtype=np.float64).ravel()
    no, nc = P.shape[0], G.shape[0]
    lin = np.broadcast_to(np.asarray(lin, dtype=np.float64), (nc,)).copy()
    quad = np.broadcast_to(np.asarray(quad, dtype=np.float64), (nc,)).copy()
    assert check_every >= 1 and max_iter >= 0 and adaptive_rho_interval >= 0
    assert adaptive_rho_interval % check_every == 0
    if x is None:
        x, y, z = np.zeros(no), np.zeros(nc), np.minimum(0.0, h)
    else:
        x, y, z = (np.array(v, dtype=np.float64).ravel() for v in (x, y, z))
    rho = float(rho)
    nan = lambda n: np.full(n, np.nan)
    if not (rho > 0.0) or not penalties_ok(lin, quad) or not rs._factor_ok(P, G, rho, sigma):
        return rs.Solution(nan(no), nan(nc), nan(nc), rs.NON_CVX, 0, (np.nan, np.nan), rho, np.inf, 0)
    soft = np.isfinite(lin) if mask else np.zeros(nc, dtype=bool)
    margin, changes, k, status = np.inf, 0, 0, rs.MAX_ITER
    while k < max_iter:
        nxt = min((k // check_every + 1) * check_every, max_iter)
        if nxt - k > 1:
            x, y, z = admm(P, q, G, h, lin, quad, x, y, z, nxt - k - 1, rho=rho, sigma=sigma, alpha=alpha)
        x_prev, y_prev = x, y
        x, y, z = admm(P, q, G, h, lin, quad, x, y, z, 1, rho=rho, sigma=sigma, alpha=alpha)
        k = nxt
        # (a soft row's dy is 0: its y as its own predecessor)
        verdict, norms, m = rs.check(P, q, G, h, x, y, z, x_prev, np.where(soft, y, y_prev), eps_abs, eps_rel,
                                     eps_prim_inf, eps_dual_inf)
        margin = min(margin, m)
        if verdict:
            status = verdict
            break
        if adaptive_rho_interval > 0 and k % adaptive_rho_interval == 0 and k < max_iter:
            rn = rs.new_rho(rho, norms)
            up, down = rn > 5.0 * rho, rn < rho / 5.0
            if up or down:
                margin = min(margin, max(rs._rel(rn, 5.0 * rho) if up else 0.0,
                                         rs._rel(rn, rho / 5.0) if down else 0.0))
            elif rn == rn:
                margin = min(margin, rs._rel(rn, 5.0 * rho), rs._rel(rn, rho / 5.0))
            if (up or down) and rho_record is not None:
                rho_record.append(norms)
            if up or down:
                rho, changes = rn, changes + 1
                if not rs._factor_ok(P, G, rho, sigma):
                    return rs.Solution(nan(no), nan(nc), nan(nc), rs.NON_CVX, k, (np.nan, np.nan), rho, margin,
                                       changes)
    return rs.Solution(x, y, z, status, k, ao.residuals(P, q, G, x, y, z), rho, margin, changes)


def slack_qp(P, q, G, h, lin, quad):
    """The slack QP of ``(P, q, G, h)`` with the penalties ``lin, quad`` (scalars or ``(nc,)``): ``(P', q', G', h')``
    in ``(x, s)``, one slack per soft row (``lin`` finite), rows ``[G  -E ; 0  -I]``."""
    P, G = np.asarray(P, dtype=np.float64), np.asarray(G, dtype=np.float64)
    no, nc = P.shape[0], G.shape[0]
    lin = np.broadcast_to(np.asarray(lin, dtype=np.float64), (nc,))
    quad = np.broadcast_to(np.asarray(quad, dtype=np.float64), (nc,))
    rows = np.flatnonzero(np.isfinite(lin))
    ns = rows.size
    E = np.zeros((nc, ns))
    E[rows, np.arange(ns)] = 1.0
    Ps = np.zeros((no + ns, no + ns))
    Ps[:no, :no] = P
    Ps[no:, no:] = np.diag(quad[rows])
    Gs = np.block([[G, -E], [np.zeros((ns, no)), -np.eye(ns)]])
    return Ps, np.concatenate([np.asarray(q, dtype=np.float64).ravel(), lin[rows]]), Gs, np.concatenate(
        [np.asarray(h, dtype=np.float64).ravel(), np.zeros(ns)])
