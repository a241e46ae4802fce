"""GPU: every route of the assembly element by element against extended precision (tests/helpers.py:
precise_reference, assert_componentwise) on plants that grow, shrink and span many decades inside one
block while staying free of cancellation (helpers.cancellation_free_plants), so that the componentwise
magnitude M tracks the results.  Each element x is held to |x - x*| <= kappa (u M + 2^-1022) with
kappa = 2 N (n + 1).  Every instance has a plant of its own; result buffers hold NaN before the call;
the kernel a route reaches is asserted where the library names it."""
import contextlib

import numpy as np
import pytest

from helpers import (LD, assert_componentwise, cancellation_free_plants, kappa, lti_tracking_problem,
                     precise_reference)
import tiled_cases as tc
from mpcasm import problems
from mpcasm.plan import _H
from oracle import qp_oracle as orc

pytestmark = pytest.mark.gpu

SAMPLES = (0, 1, 63, 64, 255, 256)


def _samples(B, few=False):
    return (0, B - 1) if few else sorted({b for b in SAMPLES if b < B} | {B - 1})


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _nan_out(torch, asm):
    f = dict(dtype=torch.float64, device="cuda")
    B, no, nc = asm.batch, asm.no, asm.nc
    return tuple(torch.full(s, float("nan"), **f) for s in ((B, no, no), (B, no), (B, nc, no), (B, nc)))


def _check(results, b, ref, kap, what):
    """The worst error of instance ``b`` over ``results`` (key -> batched array) in units of u M."""
    return max(assert_componentwise(x[b], *ref[key], kap, "%s, instance %d, %s" % (what, b, key))
               for key, x in results.items())


def _report(what, worst, kap):
    print("componentwise %-60s worst %8.3g u M   kappa %d" % (what, worst, kap))


# ---------------------------------------------------------------------------------------------------
# K1: mpcasm_fill_su.  Shapes picked from the dispatch of launch_fill_su (csrc/fill.hip): the id names
# the kernel the shape reaches at a batch of 300.
# ---------------------------------------------------------------------------------------------------
FILL = [
    (4, 2, 100, 1.3, False, "lti-quad"),
    (4, 2, 100, 1e-4, False, "lti-quad-underflow"),
    (3, 1, 33, 1.3, False, "lti-tiny"),              # (N n odd: no 16-byte rows, no quad kernel)
    (5, 1, 16, 1.3, False, "lti-tiny"),
    (5, 3, 48, 1.3, False, "lti-small"),
    (12, 6, 64, 1.25, False, "lti-workgroup"),
    (4, 2, 100, 1.3, True, "ltv-row"),
    (4, 2, 100, 1e-4, True, "ltv-row-underflow"),
    (3, 1, 33, 1.3, True, "ltv-block"),
    (5, 2, 24, 1.3, True, "ltv-block"),
    (5, 1, 100, 1.3, True, "ltv-wave"),
    (8, 2, 40, 1.3, True, "ltv-wave"),
]


@pytest.mark.parametrize("n,m,N,rho,ltv,kernel", FILL, ids=["%s-n%d-m%d-N%d" % (k, n, m, N) for n, m, N, _, _, k in FILL])
def test_fill_su(torch_gpu, n, m, N, rho, ltv, kernel):
    torch = torch_gpu
    from mpcasm import engine

    B = 300
    rng = np.random.default_rng(n * 1000 + m * 100 + N + (7 if ltv else 0))
    A, Bm = cancellation_free_plants(rng, B, n, m, rho, N, per_step=ltv)
    S = torch.full((B, N, n, n), float("nan"), dtype=torch.float64, device="cuda")
    U = torch.full((B, m, N, N, n), float("nan"), dtype=torch.float64, device="cuda")
    S, U = engine.fill_su(torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"), N, ltv=ltv,
                          out=(S, U))
    S, U = S.cpu().numpy(), U.cpu().numpy()
    extend = orc.extend_matrices_ltv if ltv else orc.extend_matrices
    kap, worst = kappa(N, n), 0.0
    for b in _samples(B):
        S0, U0 = extend(N, A[b], Bm[b], dtype=LD)
        S1, U1 = extend(N, np.abs(A[b]), np.abs(Bm[b]), dtype=LD)
        ref = {"S": (S0, S1), "U": (np.stack(U0), np.stack(U1))}
        worst = max(worst, _check({"S": S, "U": U}, b, ref, kap, kernel))
    _report("fill %s (%d, %d, %d, rho %g)" % (kernel, n, m, N, rho), worst, kap)


# ---------------------------------------------------------------------------------------------------
# The persistent kernel with its horizon tables built on chip (lti=), its four variants; the per-instance
# fused kernel and the staged pipeline fed the K1 fill's S, U of the same plants.
# ---------------------------------------------------------------------------------------------------
PATHS = {"resident": (0, 2, 1), "resident-jit": (0, 1, 1), "resident-lds": (0, 2, 2),
         "resident-jit-lds": (0, 1, 2), "fused": (1, 2, 0), "staged": (2, 2, 0)}
KERNEL = {"resident": "resident_assemble_kernel", "resident-jit": "resident_spec_kernel",
          "resident-lds": "resident_assemble_kernel", "resident-jit-lds": "resident_spec_kernel",
          "fused": "fused_assemble_kernel", "staged": "staged pipeline"}


@contextlib.contextmanager
def _path(name):
    from mpcasm import capi

    lib = capi.load()
    path, jit, direct = PATHS[name]
    assert lib.mpcasm_set_option(capi.OPT_PATH, path) == 0
    assert lib.mpcasm_set_option(capi.OPT_JIT, jit) == 0
    assert lib.mpcasm_set_option(capi.OPT_P_DIRECT, direct) == 0
    try:
        yield
    finally:
        lib.mpcasm_set_option(capi.OPT_PATH, 0)
        lib.mpcasm_set_option(capi.OPT_JIT, 0)
        lib.mpcasm_set_option(capi.OPT_P_DIRECT, 0)


def _persistent_problem(api, which, rng):
    if which.startswith("biped"):
        conf = problems.BipedConfig(step_samples=8 if which == "biped16" else 12)
        form = problems.biped(api, conf)
        form.update(step_times=np.array([6, 14] if which == "biped16" else [10, 22]), step_count=0)
        return form, "LIP", 3, 1, conf.horizon_lenght
    nx, nu, N = {"lti-4-1-9": (4, 1, 9), "lti-6-3-7": (6, 3, 7)}[which]
    return problems.random_lti(api, rng, nx=nx, nu=nu, N=N), "plant", nx, nu, N


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which", ["biped16", "biped24", "lti-4-1-9", "lti-6-3-7"])
def test_persistent_fused_and_staged(gpu_api, torch_gpu, which, path):
    torch = torch_gpu
    from mpcasm import engine

    rng = np.random.default_rng(len(which) * 100 + len(path))
    form, name, n, m, N = _persistent_problem(gpu_api, which, rng)
    B = 300
    A, Bm = cancellation_free_plants(rng, B, n, m, 1.3, N)
    At, Bt = torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda")
    given = rng.normal(0, 0.1, [B, form.given_len])
    with _path(path):
        if path.startswith("resident"):
            asm = engine.Assembler(form, batch=B, lti=[name])
            assert asm.plan.resident["ok"]
            asm.bind_lti(name, At, Bt)
        else:
            asm = engine.Assembler(form, batch=B)
            S, U = engine.fill_su(At, Bt, N)
            for j in range(m):
                asm.bind_source((name, j), U[:, j])
            asm.bind_source((name, m), S)
        out = asm.assemble(torch.as_tensor(given, device="cuda"), out=_nan_out(torch, asm))
        assert asm.last_kernel().startswith(KERNEL[path]), asm.last_kernel()
    res = dict(zip("PqGh", (t.cpu().numpy() for t in out)))
    kap, worst = kappa(N, n), 0.0
    for b in _samples(B):
        worst = max(worst, _check(res, b, precise_reference(form, name, A[b], Bm[b], given[b]), kap, path))
    _report("%s %s" % (path, which), worst, kap)


# ---------------------------------------------------------------------------------------------------
# The tiled kernel on generated horizon tables: the scan form with the set-up fused (MPCASM_OPT_PATH 0) and
# with pre-passes (1), the Toeplitz form (4), the general form (3).
# ---------------------------------------------------------------------------------------------------
TILED = [
    (5, 3, 48, 1.3, {}, 300), (12, 6, 64, 1.25, {}, 24), (4, 2, 100, 1.3, {}, 300),
    (5, 3, 48, 1.3, dict(scaled=True), 70), (5, 3, 48, 1.3, dict(extra_unknown=True), 70),
    (5, 4, 48, 1.3, dict(given_input=True), 70),        # (one input given: 4 inputs keep no >= 128, the tiled kernel's)
    (5, 3, 48, 1.3, dict(two_axis_limit=True), 70),
    # the only shape here whose plan has T_SCAN_FUSED (tiled_cases.py's builder: no row but the costs' own): on the
    # others "scan" and "scan-prepass" are one and the same launch
    (8, 4, 32, 1.3, dict(fused=True), 70),
]


@pytest.mark.parametrize("path", [0, 1, 4, 3], ids=["scan", "scan-prepass", "toeplitz", "general"])
@pytest.mark.parametrize("nx,nu,N,rho,kw,B", TILED,
                         ids=["5-3-48", "c4-shape", "4-2-100", "scaled", "extra-unknown", "given-input", "two-axis-limit",
                              "fused-8-4-32"])
def test_tiled(gpu_api, torch_gpu, nx, nu, N, rho, kw, B, path):
    torch = torch_gpu
    from mpcasm import capi, engine

    rng = np.random.default_rng(nx * 1000 + N + len(kw))
    A, Bm = cancellation_free_plants(rng, B, nx, nu, rho, N)
    if kw.get("fused"):
        form = tc.build(gpu_api, rng, tc.Shape("fused", "fused", nx, nu, N, nx, ()), (A[0], Bm[0]))
    else:
        form, _, _ = lti_tracking_problem(gpu_api, rng, nx, nu, N, plant=(A[0], Bm[0]), **kw)
    given = rng.normal(0, 0.3, [B, form.given_len])
    asm = engine.Assembler(form, batch=B, lti=["plant"])
    asm.set_option(capi.OPT_PATH, path)
    # the set-up fused into the scan kernel only where the plan allows it and the path option is 0
    fused = int(asm.plan.itab[_H["T_SCAN_FUSED"]])
    assert fused == (1 if kw.get("fused") else 0)
    asm.bind_lti("plant", torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"))
    out = asm.assemble(torch.as_tensor(given, device="cuda"), out=_nan_out(torch, asm))
    kernel = asm.last_kernel()
    assert "tiled" in kernel, kernel
    assert ("scan" in kernel) == (path in (0, 1) and N <= 64), kernel
    route = asm.tiled_route()
    assert route.form == {0: capi.TILED_SCAN if N <= 64 else capi.TILED_TOEPLITZ, 1: capi.TILED_SCAN if N <= 64
                          else capi.TILED_TOEPLITZ, 4: capi.TILED_TOEPLITZ, 3: capi.TILED_GENERAL}[path], route
    assert route.fused == (1 if fused and path == 0 else 0), route
    res = dict(zip("PqGh", (t.cpu().numpy() for t in out)))
    kap, worst = kappa(N, nx), 0.0
    for b in _samples(B, few=nx == 12):
        worst = max(worst, _check(res, b, precise_reference(form, "plant", A[b], Bm[b], given[b]), kap, kernel))
    _report("tiled path %d (%d, %d, %d) %s" % (path, nx, nu, N, ",".join(kw)), worst, kap)


@pytest.mark.parametrize("nx,nu,N,B", [(5, 3, 48, 67), (12, 6, 64, 40)], ids=["5-3-48", "c4-shape"])
def test_shared_model(gpu_api, torch_gpu, nx, nu, N, B):
    """One system for the batch, every parameter an instance's own: the shared-model form of the tiled kernel."""
    torch = torch_gpu
    from mpcasm import engine

    rng = np.random.default_rng(nx * 10 + N)
    A, Bm = cancellation_free_plants(rng, 1, nx, nu, 1.3, N)
    form, _, _ = lti_tracking_problem(gpu_api, rng, nx, nu, N, plant=(A[0], Bm[0]))
    asm = engine.Assembler(form, batch=B)
    given = rng.normal(0, 0.3, [B, form.given_len])
    host = asm.params.cpu().numpy().copy()
    for (kind, name, field), (start, rows, cols) in asm.plan.param_slots.items():
        block = host[:, start:start + rows * cols]
        if field == "weight":
            block *= rng.uniform(0.5, 2.0, [B, 1])
        elif field == "arrow":
            block *= rng.uniform(0.5, 1.5, [B, 1])
        else:
            block += rng.normal(0, 0.2, block.shape)
    asm.params.copy_(torch.as_tensor(host, device="cuda"))
    out = asm.assemble(torch.as_tensor(given, device="cuda"), out=_nan_out(torch, asm))
    assert "shared" in asm.last_kernel(), asm.last_kernel()
    res = dict(zip("PqGh", (t.cpu().numpy() for t in out)))
    limits = orc.all_limits(form)
    saved = {(k, n, f): np.array(getattr(form.goals[n] if k == "cost" else limits[n], f))
             for (k, n, f) in asm.plan.param_slots}
    kap, worst = kappa(N, nx), 0.0
    try:
        for b in _samples(B, few=nx == 12):
            for (kind, name, field), (start, rows, cols) in asm.plan.param_slots.items():
                obj = form.goals[name] if kind == "cost" else limits[name]
                value = host[b, start:start + rows * cols].reshape(rows, cols)
                obj.update(**{field: float(value[0, 0]) if field == "weight" else value})
            ref = precise_reference(form, "plant", A[0], Bm[0], given[b])
            worst = max(worst, _check(res, b, ref, kap, "shared"))
    finally:
        for (kind, name, field), value in saved.items():
            obj = form.goals[name] if kind == "cost" else limits[name]
            obj.update(**{field: float(value.ravel()[0]) if field == "weight" else value})
    _report("shared model (%d, %d, %d)" % (nx, nu, N), worst, kap)


# ---------------------------------------------------------------------------------------------------
# The sweep kernel (ltv=): C5 at its per-GPU batch, and a per-step growing plant.
# ---------------------------------------------------------------------------------------------------
def test_sweep_c5(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine
    from test_gpu_sweep import _ltv_batch

    B, N = 2048, 100
    rng = np.random.default_rng(20264)
    form = problems.lipm_ltv(gpu_api, N=N)
    A, Bm = _ltv_batch(gpu_api, B, N, rng)
    asm = engine.Assembler(form, batch=B, ltv=["LIP"])
    asm.bind_ltv("LIP", torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"))
    given = rng.normal(0, 0.05, [B, form.given_len])
    out = asm.assemble(torch.as_tensor(given, device="cuda"), out=_nan_out(torch, asm))
    assert "sweep" in asm.last_kernel(), asm.last_kernel()
    res = dict(zip("PqGh", (t.cpu().numpy() for t in out)))
    kap, worst = kappa(N, 3), 0.0
    for b in _samples(B):
        worst = max(worst, _check(res, b, precise_reference(form, "LIP", A[b], Bm[b], given[b], ltv=True), kap, "sweep C5"))
    _report("sweep C5", worst, kap)


def test_sweep_per_step_growing_plant(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine

    B, N, n, m = 300, 100, 4, 2
    rng = np.random.default_rng(4242)
    A, Bm = cancellation_free_plants(rng, B, n, m, 1.3, N, per_step=True)
    form, _, _ = lti_tracking_problem(gpu_api, rng, n, m, N, plant=(A[0, 0], Bm[0, 0]), scaled=True,
                                      two_axis_limit=True)
    asm = engine.Assembler(form, batch=B, ltv=["plant"])
    asm.bind_ltv("plant", torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"))
    given = rng.normal(0, 0.3, [B, form.given_len])
    out = asm.assemble(torch.as_tensor(given, device="cuda"), out=_nan_out(torch, asm))
    assert "sweep" in asm.last_kernel(), asm.last_kernel()
    res = dict(zip("PqGh", (t.cpu().numpy() for t in out)))
    kap, worst = kappa(N, n), 0.0
    for b in _samples(B):
        worst = max(worst, _check(res, b, precise_reference(form, "plant", A[b], Bm[b], given[b], ltv=True), kap,
                                  "sweep"))
    _report("sweep per-step (4, 2, 100)", worst, kap)


# ---------------------------------------------------------------------------------------------------
# Preview rows (mpcasm_preview_direct) on generated tables: three shapes on the direct kernel (n + m N > 32) and
# one on the staged kernel; every instantiation of the two fast kernels: test_gpu_preview_variants.py.
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu,N,rho,B,route",
                         [(5, 3, 48, 1.3, 300, "direct"), (12, 6, 64, 1.25, 24, "direct"), (4, 2, 100, 1.3, 300, "direct"),
                          (4, 2, 14, 1.3, 300, "staged")],
                         ids=["5-3-48", "c4-shape", "4-2-100", "staged-4-2-14"])
def test_preview_rows(gpu_api, torch_gpu, nx, nu, N, rho, B, route):
    torch = torch_gpu
    from mpcasm import capi, engine
    from preview_cases import generated_rows_reference

    rng = np.random.default_rng(nx + N)
    A, Bm = cancellation_free_plants(rng, B, nx, nu, rho, N)
    form = problems.random_lti(gpu_api, rng, nx=nx, nu=nu, N=N)
    asm = engine.Assembler(form, batch=B, lti=["plant"])
    asm.bind_lti("plant", torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"))
    assert capi.PREVIEW_ROUTES[asm.preview_route()[0]] == route, asm.preview_route()
    given = rng.normal(0, 0.3, [B, form.given_len])
    optim = rng.normal(0, 0.5, [B, form.optim_len])
    out = torch.full((B, asm.plan.pmrows), float("nan"), dtype=torch.float64, device="cuda")
    rows = asm.preview_rows(given, optim, out=out).cpu().numpy()
    kap, worst = kappa(N, nx), 0.0
    for b in _samples(B, few=nx == 12):
        ref = {"rows": generated_rows_reference(form, "plant", A[b], Bm[b], given[b], optim[b], asm.plan)}
        worst = max(worst, _check({"rows": rows}, b, ref, kap, "preview rows"))
    _report("preview rows (%d, %d, %d)" % (nx, nu, N), worst, kap)
