"""Shared helpers of the tests: golden loading, error measure, tolerances."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# BASELINE.json north_star: "fp64 P,q,G,h within 1e-10 relative"; measured as
# max |x - ref| / max |ref| over a whole block (an all-zero reference block must be
# reproduced exactly: the error is then max |x| itself).
RTOL = 1e-10
# what the kernels actually achieve on these problems (regression guard)
RTOL_TIGHT = 1e-13


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def rel_err(x, ref):
    x, ref = np.asarray(x, dtype=float), np.asarray(ref, dtype=float)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(x - ref)))
    return err / scale if scale > 0.0 else err


def assert_close(x, ref, tol=RTOL, what=""):
    err = rel_err(x, ref)
    assert err <= tol, "%s: relative error %.3e > %.1e" % (what, err, tol)
    return err


def ranges_from_json(text):
    return {k: range(v[0], v[1]) for k, v in json.loads(str(text)).items()}


def lti_tracking_problem(api, rng, nx, nu, N, *, scaled=False, extra_unknown=False, given_input=False,
                  two_axis_limit=False, scheduled_cost=False, crossed_cost=False, plant=None):
    """A random LTI tracking problem (problems.random_lti) with the features the scan form of the
    tiled kernel has to tell apart: a cost on a multiple of a state (coefficient != 1), unknowns that
    are no input of the plant, an input that is GIVEN, a limit over two states (a row of G that is no
    single state row), a cost on part of the horizon (no scan form), a crossed cost of two states (rows A != rows
    B: P is not symmetric, every block pair is computed; no scan form).  ``plant``: the nominal ``(A, B)``
    (default: problems.random_lti_matrices)."""
    from mpcasm import problems

    A, B = problems.random_lti_matrices(rng, nx, nu) if plant is None else plant
    inputs = ["u%d" % j for j in range(nu)]
    states = ["s%d" % i for i in range(nx)]
    ext = api.ExtendedSystem.from_cotrol_system(api.ControlSystem(inputs, states, A, B), "x", N)
    form = api.Formulation()
    form.incorporate_dynamics("plant", ext)
    if extra_unknown:
        form.incorporate_dynamics("slack", api.DomainVariable("slack", N))
    if scaled:
        form.incorporate_definition("twice", api.LineCombo({"s1": 2.5}))
    for i, name in enumerate(states):
        var = "twice" if scaled and i == 1 else name
        form.incorporate_goal("track " + name, api.Cost(
            var, float(rng.uniform(0.1, 1)), aim=[float(rng.normal())],
            schedule=range(2, N) if scheduled_cost and i == 0 else range(0)))
    if crossed_cost:
        form.incorporate_goal("crossed", api.Cost("s0", 0.4, aim=[float(rng.normal())], cross="s1",
                                                  cross_aim=[float(rng.normal())]))
    form.incorporate_goal("effort", api.Cost(inputs[-1], 0.3))
    if extra_unknown:
        form.incorporate_goal("slack", api.Cost("slack", 0.2, aim=[0.1]))
    limits = [api.Constraint("s0", 4.0), api.Constraint("s0", 3.0, arrow=[-1]),
              api.Constraint("twice" if scaled else "s1", 2.0, schedule=range(N - 3, N))]
    form.incorporate_constraint("bounds", limits)
    if two_axis_limit:
        form.incorporate_definition("mix", api.LineCombo({"s0": 1.0, "s1": -0.5}))
        form.incorporate_constraint("mixed", [api.Constraint("mix", 1.5)])
    optim = inputs[1:] if given_input else inputs
    form.identify_qp_domain(optim + (["slack"] if extra_unknown else []))
    form.make_preview_matrices()
    return form, A, B


# --------------------------------------------------------------------------------------------------
# Componentwise check against extended precision.  The block measure above says nothing about the
# small elements of a block whose elements span many decades (a growing plant over a long horizon):
# here every element x is held to |x - x*| <= kappa (u M + 2^-1022), x* the oracle run in long double
# on the very fp64 inputs the kernel saw, M the same sums over the absolute values of every datum
# (rounding-error analysis' componentwise bound, independent of the order of association).
# --------------------------------------------------------------------------------------------------
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, \
    "the componentwise checks need an extended long double (64-bit mantissa), got eps %r" % np.finfo(LD).eps
U64 = 2.0 ** -53            # unit round-off of fp64
FLOOR = 2.0 ** -1022        # smallest normal: admits flush-to-zero where powers leave the normal range


def kappa(N, n):
    """The depth of the computation: N steps of n-term products, then an N-term sum."""
    return 2 * N * (n + 1)


def assert_cancellation_free(A, N, per_step=False):
    """|Phi(k, l)| = prod |A_j| over the horizon, in long double (so that M tracks the results): ``A`` of a batch,
    ``(batch, n, n)`` or per step ``(batch, N, n, n)``."""
    A = np.asarray(A, dtype=LD)
    batch, n = A.shape[0], A.shape[-1]
    eye = np.broadcast_to(np.eye(n, dtype=LD), (batch, n, n))
    if not per_step:
        P, Q = A.copy(), np.abs(A)
        for _ in range(N):
            assert np.array_equal(np.abs(P), Q), "the plant is not free of cancellation"
            P, Q = A @ P, np.abs(A) @ Q
        return
    R, Ra = np.zeros((batch, N, n, n), dtype=LD), np.zeros((batch, N, n, n), dtype=LD)
    for k in range(N):                               # R[:, l] = Phi(k, l + 1) = A_k ... A_{l+1}
        R[:, :k] = A[:, k, None] @ R[:, :k]
        Ra[:, :k] = np.abs(A[:, k, None]) @ Ra[:, :k]
        R[:, k], Ra[:, k] = eye, eye
        assert np.array_equal(np.abs(R[:, :k + 1]), Ra[:, :k + 1]), "the plant is not free of cancellation"


_premise = assert_cancellation_free


def cancellation_free_plants(rng, batch, n, m, rho, N, per_step=False, at_once=False):
    """``batch`` plants ``A = S D A+ D S^-1``, ``B = S normal diag(logspace(-2, 2, m))``: ``A+ >= 0``
    with an upper-triangular coupling (non-normal), Perron root ``rho``; ``D`` a random +-1 diagonal,
    ``S`` a permuted diagonal from 1e-3 to 1e3 -- mixed signs, bad scaling, growth, and still
    ``|A^k| = |A|^k``.  ``per_step``: ``(batch, N, n, n)`` / ``(batch, N, n, m)``, the same ``S``, ``D``
    at every step of an instance.  ``at_once`` (not per step): the same construction drawn for the whole batch
    in one go, for batches of thousands (another sequence of draws than instance by instance).  Asserts the
    premise over the horizon."""
    if at_once:
        assert not per_step
        d = rng.uniform(0.3, 1.0, (batch, n))
        Ap = np.triu(rng.uniform(0.0, 0.5, (batch, n, n)), 1)
        Ap[:, np.arange(n), np.arange(n)] = d
        Ap *= (rho / d.max(axis=1))[:, None, None]
        perm = rng.permuted(np.tile(np.arange(n), (batch, 1)), axis=1)
        Ap = np.take_along_axis(np.take_along_axis(Ap, perm[:, :, None], 1), perm[:, None, :], 2)
        sd = rng.choice([-1.0, 1.0], (batch, n)) * 10.0 ** rng.uniform(-3, 3, (batch, n))
        A = sd[:, :, None] * Ap / sd[:, None, :]
        B = np.abs(sd)[:, :, None] * rng.standard_normal((batch, n, m)) * np.logspace(-2, 2, m)[None, None, :]
        assert_cancellation_free(A, N)
        return A, B
    steps = N if per_step else 1
    A = np.empty((batch, steps, n, n))
    B = np.empty((batch, steps, n, m))
    cols = np.logspace(-2, 2, m)
    for b in range(batch):
        perm = rng.permutation(n)
        sd = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)
        for k in range(steps):
            Ap = np.diag(rng.uniform(0.3, 1.0, n)) + np.triu(rng.uniform(0.0, 0.5, (n, n)), 1)
            Ap *= rho / np.max(np.diag(Ap))                  # (triangular: the Perron root is the largest diagonal entry)
            Ap = Ap[np.ix_(perm, perm)]
            A[b, k] = sd[:, None] * Ap / sd[None, :]
            B[b, k] = np.abs(sd)[:, None] * rng.standard_normal((n, m)) * cols[None, :]
    if not per_step:
        A, B = A[:, 0], B[:, 0]
    _premise(A, N, per_step)
    return A, B


def precise_reference(form, name, A, B, given, ltv=False, optim=None, pm_rows=None):
    """``(x*, M)`` pairs in long double for one instance whose dynamics ``name`` is the plant ``(A, B)``
    (``A_k, B_k`` with ``ltv``): ``G, h, P, q`` of the formulation as it stands (its weights, aims,
    arrows, centres and extremes), ``S, U`` (``U`` stacked ``(m, N, N, n)``), and with ``optim`` and
    ``pm_rows`` (``plan.pm_rows``: definition -> first row, rows) the preview rows ``Mg given + Mo optim``."""
    from oracle import qp_oracle as orc

    dyn = form.dynamics[name]
    N = dyn.matrices[-1].shape[0]
    extend = orc.extend_matrices_ltv if ltv else orc.extend_matrices
    given = np.asarray(given, dtype=float).reshape(-1, 1)
    out, saved = {}, list(dyn.matrices)
    try:
        for magnitude in (False, True):
            S, U = extend(N, np.abs(A) if magnitude else A, np.abs(B) if magnitude else B, dtype=LD)
            dyn.matrices = list(U) + [S]
            dyn.update_definitions()
            PM = orc.preview_matrices(form, dtype=LD, magnitude=magnitude)
            G, h, P, q = orc.assemble(form, given, PM=PM, dtype=LD, magnitude=magnitude)
            res = {"S": S, "U": np.stack(U), "G": G, "h": h.ravel(), "P": P, "q": q.ravel()}
            if pm_rows is not None:
                x = np.asarray(optim, dtype=float).reshape(-1, 1)
                res["rows"] = np.zeros(max(r0 + rows for r0, rows in pm_rows.values()), dtype=LD)
                for var, (r0, rows) in pm_rows.items():
                    res["rows"][r0:r0 + rows] = orc.preview(PM, given, x, var, dtype=LD, magnitude=magnitude).ravel()
            for key, value in res.items():
                out.setdefault(key, []).append(value)
    finally:
        dyn.matrices = saved
        dyn.update_definitions()
    return {key: tuple(pair) for key, pair in out.items()}


def componentwise_units(x, ref, mag):
    """Error of every element in units of u M (the floor in the denominator)."""
    x = np.asarray(x, dtype=np.float64)
    assert x.shape == ref.shape == mag.shape, (x.shape, ref.shape, mag.shape)
    return np.abs(x.astype(LD) - ref) / (U64 * mag + LD(FLOOR))


def assert_componentwise(x, ref, mag, kappa, what=""):
    """Every element within ``kappa (u M + 2^-1022)`` of the long-double reference; where ``M == 0`` the
    element is exactly +-0.  Returns the worst error in units of u M."""
    x = np.asarray(x, dtype=np.float64)
    units = componentwise_units(x, ref, mag)
    zero = mag == 0
    bad = ~np.isfinite(x) | np.where(zero, x != 0, units > kappa)
    if bad.any():
        score = np.where(bad, np.where(zero | ~np.isfinite(units), np.inf, units), -1)
        i = np.unravel_index(int(np.argmax(score)), x.shape)
        raise AssertionError("%s: %d element(s) off; at %s: x = %r, x* = %r, M = %r, error %.3g u M > kappa = %d"
                             % (what, int(bad.sum()), tuple(int(v) for v in i), float(x[i]), float(ref[i]),
                                float(mag[i]), float(units[i]), kappa))
    return float(units.max()) if units.size else 0.0
