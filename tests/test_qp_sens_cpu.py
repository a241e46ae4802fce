"""CPU: the sensitivity solve restated (tests/sens_restatement.py) against central differences of the exact
active-set solution, in long double -- the signs of include/mpcasm.h and DESIGN.md -- and what mpcasm_qp_sens and
mpcasm_qp_sens_wide decide without a device: the argument errors, the size limits, and that neither takes more LDS
or workspace than the polish it shares its back-ends with."""
import ctypes

import numpy as np
import pytest

import polish_restatement as pr
import polish_wide_cases as cases
import sens_restatement as sn
from helpers import LD

EPS = 1e-6          # the offset of the central differences
BOUND = 1e-6        # relative; the worst measured here is 3.7e-9 ((7, 12, 7)): the margin is for other draws


def kkt_point(P, q, G, h, start):
    """``x, y`` (long double) with ``K [x; y_A] = [-q; h_A]`` on the active set of the iterate ``start``."""
    out = sn.exact(P, G, start[3], start[0], start[1], start[2], -q, h)
    assert out.verdict == sn.DONE
    return out.u, out.w


def same_active_set(G, h, x, y, active):
    """The point is the strictly complementary solution on ``active``: multipliers positive there, slack elsewhere."""
    return bool((y[active] > 0).all() and (G[~active] @ x < h[~active]).all() and not y[~active].any())


@pytest.mark.parametrize("no,nc,na", pr.SHAPES, ids=cases.IDS(pr.SHAPES))
def test_the_restatement_against_central_differences(no, nc, na):
    """(a) along a random ``(dq, dh, symmetric dP, dG)``: the forward derivative against ``(s(+eps) - s(-eps)) / 2 eps``
    of the exact active-set solution, and the adjoint's four gradients against it through ``<gx, dx> + <gy, dy>``."""
    rng = np.random.default_rng([no, nc, na, 71])
    P, q, G, h, xs, ys, active = pr.complementary_qp(rng, no, nc, na)
    dq, dh, dG = rng.standard_normal(no), rng.standard_normal(nc), rng.standard_normal((nc, no))
    dP = rng.standard_normal((no, no))
    dP = (dP + dP.T) / 2.0
    gx, gy = rng.standard_normal(no), rng.standard_normal(nc)
    start = (xs, ys, np.minimum(G @ xs, h), h)
    found, margin = sn.active_set(h, ys, start[2])
    assert np.array_equal(found, active) and margin >= 0.5
    c = lambda a: np.asarray(a, dtype=np.float64).astype(LD)
    x0, y0 = kkt_point(P, q, G, h, start)
    assert same_active_set(c(G), c(h), x0, y0, active)
    ends = []
    for sign in (1, -1):
        e = LD(sign * EPS)
        Pe, qe, Ge, he = c(P) + e * c(dP), c(q) + e * c(dq), c(G) + e * c(dG), c(h) + e * c(dh)
        # (long double operands: the restatement converts through fp64, so the solve is done here on its parts)
        ends.append(ld_kkt(Pe, qe, Ge, he, active))
        assert same_active_set(Ge, he, *ends[-1], active), "the active set changed at offset %+g" % float(e)
    fdx, fdy = ((ends[0][i] - ends[1][i]) / LD(2 * EPS) for i in (0, 1))
    rx, ry = sn.jvp_rhs(x0, y0, active, c(dq), c(dh), c(dP), c(dG))
    # (rx, ry are long double; the restatement's exact() takes fp64 operands, so the derivative is solved here too)
    dx, dy = ld_solve(c(P), c(G), active, rx, ry)
    top = lambda v: float(np.abs(v).max(initial=LD(0)))
    rel = max(top(fdx - dx) / top(dx), top(fdy - dy) / max(top(dy), 1e-300) if na else 0.0)
    # the adjoint through the restatement proper (fp64 operands gx, gy)
    adj = sn.exact(P, G, h, *start[:3], gx, gy)
    assert adj.verdict == sn.DONE and np.array_equal(adj.active, active)
    gq, gh, gP, gG = sn.gradients(adj.u, adj.w, x0, y0, active)
    lhs = c(gx) @ fdx + c(gy) @ fdy
    rhs = gq @ c(dq) + gh @ c(dh) + (gP * c(dP)).sum() + (gG * c(dG)).sum()
    rel_adj = float(abs(lhs - rhs) / abs(rhs))
    print("qp-sens-cpu: (%d, %d, %d)  forward %.1e  adjoint %.1e  cond(K) %.1e"
          % (no, nc, na, rel, rel_adj, np.linalg.cond(kkt(P, G, active))))
    assert rel <= BOUND and rel_adj <= BOUND, (rel, rel_adj)
    assert not adj.w[~active].any() and not gG[~active].any()
    # the restatement in fp64 agrees with the exact one to its own residual's size
    plain = sn.sens(P, G, h, *start[:3], gx, gy)
    assert plain.verdict == sn.DONE and plain.lres <= 1e-10 * max(1.0, top(gx), top(gy))
    assert top(c(plain.u) - adj.u) <= 1e-9 * top(adj.u)


def kkt(P, G, active):
    GA = G[active]
    na = GA.shape[0]
    return np.block([[P, GA.T], [GA, np.zeros((na, na), dtype=P.dtype)]])


def ld_solve(P, G, active, rx, ry):
    """``K^-1 [rx; ry_A]`` in long double for long-double operands: Gaussian elimination with partial pivoting and
    two steps of refinement (numpy's solvers stop at fp64)."""
    K = kkt(P, G, active)
    n, no = K.shape[0], P.shape[0]
    r = np.concatenate([rx, ry[active]]).astype(LD)
    A, piv = K.copy(), np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]], piv[[k, p]] = A[[p, k]], piv[[p, k]]
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])

    def lu_solve(b):
        v = b[piv].copy()
        for i in range(n):
            v[i] -= A[i, :i] @ v[:i]
        for i in range(n - 1, -1, -1):
            v[i] = (v[i] - A[i, i + 1:] @ v[i + 1:]) / A[i, i]
        return v

    t = lu_solve(r)
    for _ in range(2):
        t = t + lu_solve(r - K @ t)
    w = np.zeros(len(active), dtype=LD)
    w[active] = t[no:]
    return t[:no], w


def ld_kkt(P, q, G, h, active):
    return ld_solve(P, G, active, -q, h)


def test_the_two_exact_solves_agree():
    """The restatement's ``exact`` (block elimination, refined against K) and this file's elimination with pivoting
    give the same ``K^-1 r`` to long-double rounding times the condition number."""
    no, nc, na = 36, 76, 20
    rng = np.random.default_rng([no, nc, na, 71])
    P, q, G, h, xs, ys, active = pr.complementary_qp(rng, no, nc, na)
    rx, ry = rng.standard_normal(no), rng.standard_normal(nc)
    a = sn.exact(P, G, h, xs, ys, np.minimum(G @ xs, h), rx, ry)
    u, w = ld_solve(P.astype(LD), G.astype(LD), active, rx.astype(LD), ry.astype(LD))
    scale = float(np.finfo(LD).eps) * np.linalg.cond(kkt(P, G, active)) * 64
    assert float(np.abs(a.u - u).max()) <= scale * float(np.abs(u).max())
    assert float(np.abs(a.w - w).max()) <= scale * float(np.abs(w).max())
    assert a.lres <= 64 * float(np.finfo(LD).eps) * sn.kkt_residual(P, G, active, a.u, a.w, rx, ry)[1]


def test_the_restatements_verdict_paths():
    rng = np.random.default_rng(5)
    P, q, G, h, xs, ys, active = pr.complementary_qp(rng, 5, 12, 3)
    zs = np.minimum(G @ xs, h)
    rx, ry = rng.standard_normal(5), rng.standard_normal(12)
    nan = np.full(5, np.nan), np.full(12, np.nan), np.full(12, np.nan)
    for status in (-2, -3, -4, -7):
        out = sn.sens(P, G, h, *nan, rx, ry, status=status)
        assert out.verdict == sn.SKIPPED and out.u is None and out.active is None
    assert sn.sens(P, G, h, xs, (h - zs) + 1.0, zs, rx, ry).verdict == sn.SKIPPED           # na = 12 > no = 5
    assert sn.sens(-np.eye(5), G, h, xs, ys, zs, rx, ry).verdict == sn.SINGULAR
    zero = sn.sens(P, G, h, xs, ys, zs, 0 * rx, 0 * ry)
    assert zero.verdict == sn.DONE and not zero.u.any() and not zero.w.any() and zero.lres == 0


@pytest.mark.parametrize("no,nc,na", [(5, 3, 0), (7, 12, 7), (36, 76, 20), (130, 0, 0)])
def test_the_gpu_tests_judge_accepts_a_correct_implementation(no, nc, na):
    """tests/sens_cases.py's judge on the seven instances of a shape, with the plain fp64 restatement and fp64 numpy
    products standing in for the device: the premises of the GPU tests (verdicts, active sets) and a yardstick that a
    correct implementation meets."""
    import sens_cases as sc

    case = sc.problem(no, nc, na)
    xyz = sc.with_nan_iterate(case)
    for status in (sc.seven_status(), None):
        u, w = np.full((7, no), sc.KEEP), np.full((7, nc), sc.KEEP)
        gP, gG = np.full((7, no, no), sc.KEEP), np.full((7, nc, no), sc.KEEP)
        lres, verdict = np.full(7, sc.KEEP), np.full(7, -99, dtype=np.int32)
        for b in range(7):
            out = sn.sens(case["P"][b], case["G"][b], case["h"][b], xyz[0][b], xyz[1][b], xyz[2][b], case["rx"][b],
                          case["ry"][b], status=None if status is None else status[b])
            verdict[b] = out.verdict
            if out.verdict == sn.DONE:
                u[b], w[b], lres[b] = out.u, out.w, out.lres
                gP[b], gG[b] = sn.gradients(out.u, out.w, xyz[0][b], xyz[1][b], out.active)[2:]
        outs, worst = sc.judge(case["P"], case["G"], case["h"], xyz, case["rx"], case["ry"], status,
                               (u, w, gP, gG, verdict, lres), "the restatement itself")
        assert max(worst) <= 1.0
        expected = [sn.DONE] * 3 + ([sn.SKIPPED] * 2 if status is not None else [sn.DONE] * 2) + [sn.SINGULAR, sn.DONE]
        assert [o.verdict for o in outs] == expected


# ---- the library, without a device -------------------------------------------------------------------------------
SENS_ORDER = ("no", "nc", "P", "G", "h", "x", "y", "z", "status", "rx", "ry", "delta", "refine", "u", "w", "gP", "gG",
              "verdict", "lres", "batch")


def sens_args(**change):
    good = dict(no=5, nc=3, P=16, G=16, h=16, x=16, y=16, z=16, status=None, rx=16, ry=16, delta=1e-6, refine=3, u=16,
                w=16, gP=None, gG=None, verdict=16, lres=None, batch=1)
    good.update(change)
    return [good[k] for k in SENS_ORDER]


def refusals(call):
    """What both entries refuse alike, before any device call (the pointers are never read)."""
    from mpcasm import capi

    for delta in (0.0, -1e-6, float("nan"), float("inf")):
        assert call(delta=delta) == capi.ERR_ARG, delta
    assert call(refine=-1) == capi.ERR_ARG
    assert call(batch=-1) == capi.ERR_ARG
    assert call(no=0) == capi.ERR_ARG and call(nc=-1) == capi.ERR_ARG
    for name in ("P", "G", "h", "x", "y", "z", "rx", "ry", "u", "w", "verdict"):
        assert call(**{name: None}) == capi.ERR_ARG, name
    # without limits G, h, y, z, ry, w may be null: only then
    assert call(nc=0, G=None, h=None, y=None, z=None, ry=None, w=None, batch=0) == capi.OK
    # batch == 0 answers ok, whatever the pointers, and without a device
    assert call(batch=0) == capi.OK
    assert call(batch=0, P=None, rx=None, u=None, verdict=None) == capi.OK


def test_argument_errors_are_decided_before_any_device_call():
    from mpcasm import capi

    lib = capi.load()
    refusals(lambda **change: lib.mpcasm_qp_sens(*sens_args(**change), None))
    out = ctypes.c_int64()
    assert lib.mpcasm_qp_sens_lds_bytes(0, 3, ctypes.byref(out)) == capi.ERR_ARG
    assert lib.mpcasm_qp_sens_lds_bytes(5, -1, ctypes.byref(out)) == capi.ERR_ARG
    assert lib.mpcasm_qp_sens_lds_bytes(5, 3, None) == capi.ERR_ARG


def test_argument_errors_of_the_wide_entry():
    from mpcasm import capi, engine

    lib = capi.load()
    need = engine.qp_sens_wide_info(96, 196, 5)[1]

    def call(work=4096, bytes=need, **change):
        args = dict(no=96, nc=196, batch=5)
        args.update(change)
        return lib.mpcasm_qp_sens_wide(*sens_args(**args), work, bytes, None)

    refusals(call)
    # the workspace: null, not on 16 bytes, a byte short, five instances' for six
    assert call(work=None) == capi.ERR_ARG
    for work in (4096 + 8, 4096 + 1, 4096 + 4):
        assert call(work=work) == capi.ERR_ARG, work
    assert call(bytes=need - 1) == capi.ERR_ARG and call(bytes=0) == capi.ERR_ARG
    assert call(batch=6) == capi.ERR_ARG
    assert call(batch=0, work=None, bytes=0) == capi.OK
    out64, out32 = ctypes.c_int64(), ctypes.c_int32()
    a, b, c = ctypes.byref(out64), ctypes.byref(out64), ctypes.byref(out32)
    assert lib.mpcasm_qp_sens_wide_info(0, 3, 1, a, b, c) == capi.ERR_ARG
    assert lib.mpcasm_qp_sens_wide_info(5, -1, 1, a, b, c) == capi.ERR_ARG
    assert lib.mpcasm_qp_sens_wide_info(5, 3, -1, a, b, c) == capi.ERR_ARG
    for hole in range(3):
        args = [a, b, c]
        args[hole] = None
        assert lib.mpcasm_qp_sens_wide_info(5, 3, 1, *args) == capi.ERR_ARG


@pytest.mark.parametrize("no,nc,na", pr.SHAPES, ids=cases.IDS(pr.SHAPES))
def test_no_more_lds_than_the_polish(no, nc, na):
    """(c) on every shape of the polish's tests."""
    from mpcasm import engine

    assert engine.qp_sens_lds_bytes(no, nc) <= engine.qp_polish_lds_bytes(no, nc)


@pytest.mark.parametrize("no,nc", [(96, 196), (70, 70), (68, 100), (69, 1), (68, 67), (68, 66), (68, 1), (1, 0)])
def test_err_limit_exactly_where_the_polish_gives_it(no, nc):
    from mpcasm import capi

    lib = capi.load()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    rc = lib.mpcasm_qp_polish_lds_bytes(no, nc, ctypes.byref(a))
    assert lib.mpcasm_qp_sens_lds_bytes(no, nc, ctypes.byref(b)) == rc and b.value <= a.value
    assert rc in (capi.OK, capi.ERR_LIMIT)
    if rc == capi.ERR_LIMIT:
        # ... and the call itself refuses before it touches a device (the pointers are never read)
        assert lib.mpcasm_qp_sens(*sens_args(no=no, nc=nc), None) == capi.ERR_LIMIT


WIDE = cases.SHAPES + [cases.LARGEST]


@pytest.mark.parametrize("no,nc,na", WIDE, ids=cases.IDS(WIDE))
def test_the_wide_entry_takes_no_more_than_the_wide_polish(no, nc, na):
    from mpcasm import engine

    for batch in (1, 7, 512, 4096):
        sens, polish = engine.qp_sens_wide_info(no, nc, batch), engine.qp_polish_wide_info(no, nc, batch)
        assert sens[0] <= polish[0] and sens[1] <= polish[1] and sens[2] == polish[2]


@pytest.mark.parametrize("no,nc", [(513, 4), (513, 0), (512, 3133), (96, 4641), (1, 4985), (512, 3132), (96, 4640)])
def test_the_wide_limit_is_the_wide_polishs(no, nc):
    from mpcasm import capi

    lib = capi.load()
    outs = [(ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()) for _ in range(2)]
    rc = lib.mpcasm_qp_polish_wide_info(no, nc, 4, *(ctypes.byref(v) for v in outs[0]))
    assert lib.mpcasm_qp_sens_wide_info(no, nc, 4, *(ctypes.byref(v) for v in outs[1])) == rc
    assert [v.value for v in outs[0]] == [v.value for v in outs[1]]
    assert rc in (capi.OK, capi.ERR_LIMIT)
    if rc == capi.ERR_LIMIT:
        assert lib.mpcasm_qp_sens_wide(*sens_args(no=no, nc=nc, batch=4), 16, 1 << 40, None) == capi.ERR_LIMIT


@pytest.mark.parametrize("backward", [False, True], ids=["forward only", "after backward"])
def test_a_differentiable_solution_is_freed_with_its_last_reference(monkeypatch, backward):
    """solve_qp_diff's autograd node must not keep its own outputs alive: with the solve and the sensitivity
    replaced by stand-ins on CPU tensors (the Function and what it keeps on ctx are the shipped ones), the result,
    its x, its solution's tensors and the saved P die with ``del`` and one ``gc.collect()`` -- a cycle through the
    autograd graph would keep all of them, on the device, for every call."""
    import gc
    import weakref

    import torch

    from mpcasm import diff, engine

    def solve(P, q, G, h, polish=False, **kw):
        B, nc = G.shape[0], G.shape[1]
        return engine.PolishedQpSolution(-q.clone(), torch.ones(B, nc, dtype=q.dtype), torch.zeros(B, nc, dtype=q.dtype),
                                         torch.ones(B, dtype=torch.int32), torch.ones(B, dtype=torch.int32),
                                         torch.zeros(B, 2), torch.ones(B), torch.ones(B, dtype=torch.int32))

    def sens(P, G, h, xyz, rx, ry, status=None, want_P=False, want_G=False, stream=None, **kw):
        return engine.QpSensitivity(rx.clone(), ry.clone(), torch.zeros_like(P) if want_P else None,
                                    torch.zeros_like(G) if want_G else None, torch.ones(P.shape[0], dtype=torch.int32),
                                    torch.zeros(P.shape[0], dtype=P.dtype))

    monkeypatch.setattr(diff, "require_device", lambda: torch)
    monkeypatch.setattr(engine, "solve_qp", solve)
    monkeypatch.setattr(engine, "qp_sensitivity", sens)
    P, q = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1).requires_grad_(), torch.ones(2, 3, dtype=torch.float64)
    G, h = torch.ones(2, 4, 3, dtype=torch.float64), torch.ones(2, 4, dtype=torch.float64).requires_grad_()
    q.requires_grad_()
    res = diff.solve_qp_diff(P, q, G, h)
    assert res.verdict is None and res.lres is None and res.sol.x.data_ptr() == res.x.data_ptr()
    if backward:
        (res.x.sum() + 2 * res.y.sum()).backward()
        assert res.verdict.tolist() == [1, 1] and res.lres is not None
        assert torch.equal(q.grad, -torch.ones(2, 3, dtype=torch.float64)) and torch.equal(h.grad, 2 * torch.ones_like(h))
        assert P.grad is not None and G.grad is None
    alive = [weakref.ref(o) for o in (res, res.x, res.y, res.sol.x, res.sol.z, res.x.grad_fn)]
    del res
    gc.collect()
    assert [r() is None for r in alive] == [True] * len(alive)


def test_the_binding_and_the_python_entry_points():
    from mpcasm import capi, diff, engine

    assert (capi.SENS_DONE, capi.SENS_SKIPPED, capi.SENS_SINGULAR) == (sn.DONE, sn.SKIPPED, sn.SINGULAR) == (1, 0, -1)
    assert (engine.SENS_DONE, engine.SENS_SKIPPED, engine.SENS_SINGULAR) == (1, 0, -1)
    assert engine.QpSensitivity._fields == ("u", "w", "gP", "gG", "verdict", "lres")
    assert engine.QpVjp._fields == ("gq", "gh", "gP", "gG", "verdict")
    assert engine.QpJvp._fields == ("dx", "dy", "verdict")
    for name in ("qp_sensitivity", "qp_sensitivity_wide", "qp_sens_lds_bytes", "qp_sens_wide_info", "qp_vjp", "qp_jvp"):
        assert callable(getattr(engine, name))
    assert callable(diff.solve_qp_diff)
    assert capi.load().mpcasm_abi_version() == 1004
    # soft= is refused before anything else is looked at
    with pytest.raises(ValueError):
        diff.solve_qp_diff(None, None, None, None, soft=(1.0, 0.0))
