"""What the GPU tests of mpcasm_qp_sens and mpcasm_qp_sens_wide share  --  TEST INFRASTRUCTURE ONLY: the instances
they pose (numpy, built once, never changed) and the judge that holds one call to tests/sens_restatement.py.

The instances of a shape are strictly complementary QPs of tests/polish_restatement.py's construction (the stream of
tests/polish_wide_cases.py, seed ``[no, nc, na, 71]``); the iterate passed in is the CONSTRUCTED solution ``x*, y*,
z* = min(G x*, h)``, so that the active set is the constructed one, with ``y >= 0.5`` on it and a slack ``>= 0.5``
off it (asserted here), and no test leans on an ADMM iterate.  ``rx, ry`` are standard normal.  Seven instances:
three plain; one ``QP_NON_CVX`` by its status with NaN iterates; one ``QP_MAX_ITER`` by its status; one whose ``P``
is ``-I``; one with ``rx = ry = 0``.

The yardstick of a ``SENS_DONE`` instance, in the style of tests/test_gpu_qp_polish.py: the long-double residual
``|r - K t|_inf`` of the device's ``t = [u; w_A]`` is at most 8 times the plain fp64 restatement's on the same input
(the project's margin for another order of summation), or within the rounding magnitude
``(no + na + 2) u64 max_i (|K||t| + |r|)_i`` of that residual's own evaluation where that is larger; ``K`` is built
from the restated active set.  ``w`` is exactly 0 off the set, ``lres`` within that magnitude of the long-double
value.  ``gP`` and ``gG`` are products of the device's own ``u, w`` and the iterate: each element within
``4 u64 (|u_i x_j| + |x_i u_j|)`` (``4 u64 (|y_i u_j| + |w_i x_j|)``) of the long-double value -- two rounded products,
a rounded sum, the halving exact -- and inactive rows of ``gG`` exact zeros."""
import functools
import os

import numpy as np

import polish_restatement as pr
import sens_restatement as sn
from helpers import LD, U64
from mpcasm import capi

YARD = 8.0
PAD = 2                                     # rows of NaN (-99 for the verdicts) behind the batch
KEEP = -7.25                                # what every output holds before a call
PLAIN, NON_CVX, MAX_ITER, SINGULAR, ZERO = (0, 1, 2), 3, 4, 5, 6
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       "qp_sens_precision.txt")
HEAD = ("# mpcasm_qp_sens and mpcasm_qp_sens_wide, SENS_DONE instances: worst (device residual |r - K t|) / max(8 x the\n"
        "# fp64 restatement's, (no + na + 2) u64 max(|K||t| + |r|)), worst |lres - residual| over that magnitude, and the\n"
        "# worst elementwise error of gP and gG over 4 u64 (|u x| + |x u|), per shape; written by\n"
        "# tests/test_gpu_qp_sens.py, tests/test_gpu_qp_sens_wide.py\n")


def record(key, text):
    """One line per shape in profiles/qp_sens_precision.txt (a checkout that cannot be written is left alone)."""
    print("qp-sens-precision: %-26s %s" % (key, text))
    try:
        lines = {}
        if os.path.exists(PROFILE):
            for line in open(PROFILE):
                if not line.startswith("#") and line.strip():
                    lines[line[:26].strip()] = line.rstrip("\n")
        lines[key] = "%-26s %s" % (key, text)
        with open(PROFILE, "w") as f:
            f.write(HEAD + "".join(lines[k] + "\n" for k in sorted(lines)))
    except OSError:
        pass


@functools.lru_cache(maxsize=None)
def problem(no, nc, na, count=7):
    """``count`` instances of a shape: a dict of stacked numpy ``P, G, h, x, y, z, rx, ry, active`` (``P[SINGULAR]``
    is ``-I`` and ``rx, ry`` of ``ZERO`` are 0 when ``count`` is 7; the status marks are the caller's)."""
    rng = np.random.default_rng([no, nc, na, 71])
    qps = [pr.complementary_qp(rng, no, nc, na) for _ in range(count)]
    P, _q, G, h, x, y, active = (np.stack([qp[i] for qp in qps]) for i in range(7))
    z = np.stack([np.minimum(G[b] @ x[b], h[b]) for b in range(count)])
    for b in range(count):
        found, margin = sn.active_set(h[b], y[b], z[b])
        assert np.array_equal(found, active[b]) and margin >= 0.5, (no, nc, na, b, margin)
        assert (y[b][active[b]] >= 0.5).all() and ((h[b] - z[b])[~active[b]] >= 0.5).all()
    side = np.random.default_rng([no, nc, na, 73])
    rx, ry = side.standard_normal((count, no)), side.standard_normal((count, nc))
    if count == 7:
        P[SINGULAR] = -np.eye(no)
        rx[ZERO], ry[ZERO] = 0.0, 0.0
    out = dict(P=P, G=G, h=h, x=x, y=y, z=z, rx=rx, ry=ry, active=active)
    for a in out.values():
        a.setflags(write=False)
    return out


def seven_status():
    status = np.full(7, capi.QP_SOLVED, dtype=np.int32)
    status[NON_CVX], status[MAX_ITER] = capi.QP_NON_CVX, capi.QP_MAX_ITER
    return status


def with_nan_iterate(case):
    """The iterates of the seven with the NON_CVX instance's set to NaN (copies)."""
    x, y, z = (case[k].copy() for k in "xyz")
    x[NON_CVX], y[NON_CVX], z[NON_CVX] = np.nan, np.nan, np.nan
    return x, y, z


def padded(torch, shape, fill, dtype=None):
    """A device tensor of ``shape[0] + PAD`` rows: the first ``shape[0]`` hold KEEP (-99 for int32), the rows behind
    them ``fill``.  Returns ``(whole, view of the first rows)``."""
    dtype = dtype or torch.float64
    B = shape[0]
    whole = torch.full((B + PAD,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")
    whole[:B] = -99 if dtype == torch.int32 else KEEP
    return whole, whole[:B]


def same(a, c):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(c).view(np.int64))


def product_errors(dev, ref, bound):
    """The worst ``|dev - ref| / bound`` over the elements (0 / 0 is 0); a NaN must stand where the reference has
    one."""
    nan = np.isnan(ref.astype(np.float64))
    assert np.array_equal(np.isnan(dev), nan)
    err = np.abs(dev.astype(LD) - ref)[~nan]
    bound = bound[~nan]
    assert (err <= bound).all(), float((err - bound).max())
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    return float(ratio.max(initial=LD(0)))


def judge(P, G, h, xyz, rx, ry, status, dev, what, rhs_terms=None, margin=None):
    """One sensitivity call against the restatement.  ``P, G, h, rx, ry``: stacked numpy; ``xyz``: the iterates that
    went in; ``status``: numpy or None; ``dev``: what came back, numpy ``(u, w, gP, gG, verdict, lres)`` (``gP``,
    ``gG`` may be None), every output having held KEEP before the call.  ``rhs_terms``: per instance, the magnitude
    ``(m1 [no], m2 [nc])`` of the terms ``r`` was summed from, where it is itself a computed sum (it replaces ``|r|`` in
    the rounding magnitude).  ``margin``: judge only the instances whose restated active-set margin is at least this
    (None: every instance, and every margin must be at least 1e-6).  Returns the restatement's results (None where
    not judged) and the worst ratios ``[residual, lres, gP, gG]``."""
    x, y, z = xyz
    u, w, gP, gG, verdict, lres = dev
    no, nc = P.shape[1], G.shape[1]
    outs, worst = [], [0.0, 0.0, 0.0, 0.0]
    for b in range(P.shape[0]):
        st = None if status is None else status[b]
        out = sn.sens(P[b], G[b], h[b], x[b], y[b], z[b], rx[b], ry[b], status=st)
        if margin is not None and out.margin < margin:
            outs.append(None)
            continue
        outs.append(out)
        assert out.margin >= 1e-6, (what, b, out.margin)
        assert verdict[b] == out.verdict, (what, b, int(verdict[b]), out.verdict)
        if out.verdict != sn.DONE:                  # every output but the verdict keeps its bits
            for t in (u, w, gP, gG, lres):
                assert t is None or (t[b] == KEEP).all(), (what, b)
            continue
        active, na = out.active, int(out.active.sum())
        assert np.isfinite(u[b]).all() and np.isfinite(w[b]).all(), (what, b)
        assert not w[b][~active].any(), (what, b)                             # exactly 0 off the active set
        res, M = sn.kkt_residual(P[b], G[b], active, u[b], w[b], rx[b], ry[b])
        if rhs_terms is not None:
            m1, m2 = rhs_terms[b]
            M = sn.kkt_residual(P[b], G[b], active, u[b], w[b], m1, m2)[1]
        fres = sn.kkt_residual(P[b], G[b], active, out.u, out.w, rx[b], ry[b])[0]
        bound = (no + na + 2) * U64 * M
        limit = max(YARD * fres, bound)
        assert res <= limit, (what, b, res, fres, bound)
        worst[0] = max(worst[0], res / limit if res > 0.0 else 0.0)
        assert abs(lres[b] - res) <= bound, (what, b, lres[b], res, bound)
        worst[1] = max(worst[1], abs(lres[b] - res) / bound if bound > 0 else 0.0)
        if not rx[b].any() and not ry[b].any():
            assert not u[b].any() and not w[b].any() and lres[b] == 0.0, (what, b)
        c = lambda a: np.asarray(a, dtype=np.float64).astype(LD)
        ul, wl, xl, yl = c(u[b]), c(w[b]), c(x[b]), c(y[b])
        if gP is not None:
            ref = sn.gradients(ul, wl, xl, yl, active)[2]
            bound_p = 4 * U64 * (np.abs(np.outer(ul, xl)) + np.abs(np.outer(xl, ul)))
            worst[2] = max(worst[2], product_errors(gP[b], ref, bound_p))
            if np.isfinite(gP[b]).all():
                assert same(gP[b], gP[b].T), (what, b)                        # the same bits either side
        if gG is not None:
            ref = sn.gradients(ul, wl, xl, yl, active)[3]
            bound_g = 4 * U64 * (np.abs(np.outer(yl, ul)) + np.abs(np.outer(wl, xl)))
            bound_g[~active] = 0
            assert same(gG[b][~active], np.zeros_like(gG[b][~active])), (what, b)   # exact (positive) zeros
            worst[3] = max(worst[3], product_errors(gG[b][active], ref[active], bound_g[active]))
    return outs, worst


def run(torch, call, case, xyz, status, what, want=True, **judge_kw):
    """One call ``call(P, G, h, (x, y, z), rx, ry, status=, want_P=, want_G=, out=)`` on the stacked numpy ``case``
    with outputs that hold KEEP and carry PAD rows behind the batch, judged.  Returns :func:`judge`'s pair."""
    B, no, nc = case["P"].shape[0], case["P"].shape[1], case["G"].shape[1]
    dev = lambda a: torch.as_tensor(np.array(a), device="cuda")
    P, G, h, rx, ry = (dev(case[k]) for k in ("P", "G", "h", "rx", "ry"))
    x, y, z = (dev(a) for a in xyz)
    nan = float("nan")
    wu, u = padded(torch, (B, no), nan)
    ww, w = padded(torch, (B, nc), nan)
    wl, lres = padded(torch, (B,), nan)
    wv, verdict = padded(torch, (B,), -99, torch.int32)
    wP, gP = padded(torch, (B, no, no), nan) if want else (None, None)
    wG, gG = padded(torch, (B, nc, no), nan) if want else (None, None)
    before = [t.clone() for t in (P, G, h, x, y, z, rx, ry)]
    behind = [None if t is None else t[B:].clone() for t in (wu, ww, wl, wP, wG, wv)]
    st = None if status is None else dev(status)
    got = call(P, G, h, (x, y, z), rx, ry, status=st, want_P=want, want_G=want, out=(u, w, gP, gG, verdict, lres))
    torch.cuda.synchronize()
    assert got.u.data_ptr() == u.data_ptr() and got.verdict.data_ptr() == verdict.data_ptr()
    assert (got.gP is None) == (not want) and (got.gG is None) == (not want)
    bits = lambda t: t if t.dtype == torch.int32 else t.view(torch.int64)
    for whole, pad in zip((wu, ww, wl, wP, wG, wv), behind):        # the rows behind the batch keep their bits
        assert whole is None or torch.equal(bits(whole[B:]), bits(pad))
    assert wv[B:].tolist() == [-99] * PAD
    for a, c in zip(before, (P, G, h, x, y, z, rx, ry)):            # the inputs are only read
        assert torch.equal(a.view(torch.int64), c.view(torch.int64))
    host = tuple(None if t is None else t.cpu().numpy() for t in (u, w, gP, gG, verdict, lres))
    return judge(case["P"], case["G"], case["h"], xyz, case["rx"], case["ry"], status, host, what, **judge_kw)


def seven(torch, call, no, nc, na, label):
    """The seven instances of a shape with their status, then with status = NULL; the premises of each; the worst
    ratios recorded under ``label``."""
    case = problem(no, nc, na)
    xyz = with_nan_iterate(case)
    status = seven_status()
    worst = [0.0] * 4
    for what, st in (("with status", status), ("status NULL", None)):
        outs, w = run(torch, call, case, xyz, st, "%s %dx%d na %d, %s" % (label, no, nc, na, what))
        worst = [max(a, b) for a, b in zip(worst, w)]
        verdicts = [o.verdict for o in outs]
        for b in PLAIN + (ZERO,):
            assert verdicts[b] == sn.DONE and np.array_equal(outs[b].active, case["active"][b])
        assert verdicts[SINGULAR] == sn.SINGULAR
        if st is not None:
            assert verdicts[NON_CVX] == verdicts[MAX_ITER] == sn.SKIPPED
        else:
            # (the NaN iterate is read then: no comparison of the active-set test holds, the solve is P's alone)
            assert verdicts[MAX_ITER] == sn.DONE and verdicts[NON_CVX] == sn.DONE and not outs[NON_CVX].active.any()
    # ... and once without the dense gradients (d_gP = d_gG = NULL)
    run(torch, call, case, xyz, status, "%s %dx%d na %d, no dense gradients" % (label, no, nc, na), want=False)
    record("%s %dx%d-na%d" % (label, no, nc, na),
           "residual %.3f  lres %.3f  gP %.3f  gG %.3f" % tuple(worst))
