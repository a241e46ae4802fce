"""GPU: every variant of the staged pipeline (csrc/assemble.hip) and of the per-instance fused kernel
(csrc/fused.hip) against extended precision.  The family of staged_cases.py spans what staged_choose can select and
what the kernels' branches tell apart (test_staged_routes_cpu.py holds it to that); here each case first asserts that
the library takes the route its entry pins (Assembler.staged_route, the launch's own decision; engine.assemble_route
for the kernel family; last_kernel), then assembles into NaN-filled buffers -- every instance its own plant(s) (A, B),
whose horizon matrices S, U come from engine.fill_su, its own given and, where the case says so, its own weights,
aims, arrows, centres and extremes -- and holds P, q, G, h of the sampled instances element by element to
|x - x*| <= kappa (u M + 2^-1022), kappa = 2 N (n + 1) (helpers.py), x* the oracle in long double on the very fp64
plants, given and parameters.  Cases marked ``halves`` then launch one half at a time: the wanted half bit for bit the
full call's, the other buffers untouched.  ``zero_weight``: cost weights of exactly 0 in every other instance -- where
M == 0 the element is an exact zero (assert_componentwise), and the instances between them are held as ever."""
import numpy as np
import pytest

import staged_cases as sc
import sweep_cases
from helpers import assert_componentwise, kappa

pytestmark = pytest.mark.gpu

KERNEL = {sc.FUSED: "fused_assemble_kernel", sc.STAGED: "staged pipeline"}
# the long-double references, by the inputs they belong to (the seed follows from the shape alone)
_REFERENCES = {}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _nan_out(torch, asm):
    f = dict(dtype=torch.float64, device="cuda")
    n, no, nc = asm.batch, asm.no, asm.nc
    return tuple(torch.full(s, float("nan"), **f) for s in ((n, no, no), (n, no), (n, nc, no), (n, nc)))


def _set_up(api, torch, case):
    """The assembler of ``case`` with the horizon matrices of every instance's plants bound, its parameters, given."""
    from mpcasm import capi, engine

    shape, batch = case.shape, case.batch
    rng = np.random.default_rng(9000 + 1000 * shape.n + 10 * shape.N + shape.m + 7 * len(shape.kw))
    plant = sc.plants(rng, batch, shape)
    form = sc.build(api, rng, shape, sc.instance(plant, 0))
    given = rng.normal(0, 0.3, [batch, form.given_len])
    asm = engine.Assembler(form, batch=batch)
    for name, (A, Bm) in plant.items():
        S, U = engine.fill_su(torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"), shape.N)
        for j in range(Bm.shape[2]):
            asm.bind_source((name, j), U[:, j])
        asm.bind_source((name, Bm.shape[2]), S)
    params = asm.params.cpu().numpy().copy()
    if case.own_params:
        params = sweep_cases.perturb_params(asm.plan, params, rng)
    if case.zero_weight:
        for slot in sc.zero_weight_slots(asm.plan, shape):
            params[1::2, slot] = 0.0
    asm.params.copy_(torch.as_tensor(params, device="cuda"))
    asm.set_option(capi.OPT_PATH, case.path)
    return form, asm, plant, params, given


def _assert_route(asm, case, **want):
    from mpcasm import capi, engine

    kernel = engine.assemble_route(asm.plan, asm.batch, path=case.path)
    assert kernel.kernel == case.route.kernel, kernel
    if case.route.lds is not None:
        assert kernel.lds == case.route.lds
    r = asm.staged_route(**want)
    expect = case.route
    if want.get("want_cost") is False:
        expect = expect._replace(hessian=capi.STAGED_NONE, sym=0, nb=0, npairs=0, nbr=0, nbc=0)
    if want.get("want_constraints") is False:
        expect = expect._replace(whole_lines=0)
    assert sc.Route(case.route.kernel, r.hessian, r.sym, r.nb, r.npairs, r.nbr, r.nbc, r.whole_lines, r.max_axes,
                    case.route.lds) == expect, r


@pytest.mark.parametrize("case", sc.GPU_CASES, ids=[c.shape.name for c in sc.GPU_CASES])
def test_variant(gpu_api, torch_gpu, case):
    torch = torch_gpu
    shape, batch = case.shape, case.batch
    form, asm, plant, params, given = _set_up(gpu_api, torch, case)
    _assert_route(asm, case)
    g = torch.as_tensor(given, device="cuda")
    full = _nan_out(torch, asm)
    asm.assemble(g, out=full)
    assert asm.last_kernel().startswith(KERNEL[case.route.kernel]), asm.last_kernel()
    res = {key: t.cpu().numpy() for key, t in zip("PqGh", full)}
    kap, worst = kappa(shape.N, shape.n), 0.0
    samples = sorted({0, batch - 1} if batch < 8 else {0, 7, 8, batch - 1})
    refs = _REFERENCES.setdefault((shape[1:], batch, case.own_params, case.zero_weight), {})
    with sweep_cases.instance_params(form, asm.plan) as objects:
        for b in samples:
            if b not in refs:
                objects.set(params[b])
                refs[b] = sc.reference(form, sc.instance(plant, b), given[b])
            for key, x in res.items():
                worst = max(worst, assert_componentwise(x[b], *refs[b][key], kap,
                                                        "%s, instance %d, %s" % (shape.name, b, key)))
    if case.zero_weight:
        # the instances with the weights at 0 have whole blocks of exact zeros: the test is not vacuous
        assert all((refs[b]["P"][1] == 0).any() and (refs[b]["q"][1] == 0).any() for b in samples if b % 2)
    if case.halves:
        # one half at a time, into fresh NaN buffers: the wanted half bit for bit, the other one untouched
        for want in (dict(want_constraints=False), dict(want_cost=False)):
            _assert_route(asm, case, **want)
            out = _nan_out(torch, asm)
            asm.assemble(g, out=out, **want)
            assert asm.last_kernel().startswith(KERNEL[case.route.kernel]), asm.last_kernel()
            cost_half = "want_constraints" in want
            for i, (mine, ref) in enumerate(zip(out, full)):
                if (i < 2) == cost_half:
                    assert torch.equal(mine, ref), "%s %s" % ("PqGh"[i], want)
                else:
                    assert bool(torch.isnan(mine).all()), "%s written with %s" % ("PqGh"[i], want)
    r = case.route
    what = "fused kernel" if r.kernel == sc.FUSED else "staged " + \
        ("gemm nb %d %s" % (r.nb, "sym" if r.sym else "all pairs") if r.hessian == sc.GEMM else "block %dx%d" % (r.nbr, r.nbc))
    print("componentwise %-60s worst %8.3g u M   kappa %d" % ("%s %s" % (what, shape.name), worst, kap))


def test_a_refused_launch_writes_nothing(gpu_api, torch_gpu):
    """A limit of 9 axes, more than K4 holds: MPCASM_ERR_LIMIT from the launch as from staged_route, and -- the
    refusal comes before the first kernel -- P, q, G, h still hold their NaN.  With the constraints not wanted the same
    plan assembles P and q."""
    torch = torch_gpu
    from mpcasm import capi

    case = sc.BY_NAME["axes-9"]
    form, asm, plant, params, given = _set_up(gpu_api, torch, case)
    with pytest.raises(capi.MpcasmError) as refusal:
        asm.staged_route()
    assert refusal.value.status == capi.ERR_LIMIT
    g = torch.as_tensor(given, device="cuda")
    out = _nan_out(torch, asm)
    with pytest.raises(capi.MpcasmError) as refusal:
        asm.assemble(g, out=out)
    assert refusal.value.status == capi.ERR_LIMIT
    torch.cuda.synchronize()
    for key, t in zip("PqGh", out):
        assert bool(torch.isnan(t).all()), "%s written by a refused launch" % key
    asm.assemble(g, out=out, want_constraints=False)
    assert asm.last_kernel().startswith(KERNEL[sc.STAGED])
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all())
    assert bool(torch.isnan(out[2]).all()) and bool(torch.isnan(out[3]).all())
    ref = sc.reference(form, sc.instance(plant, 3), given[3])
    kap = kappa(case.shape.N, case.shape.n)
    for key, t in zip("Pq", out):
        assert_componentwise(t[3].cpu().numpy(), *ref[key], kap, "axes-9, cost half, %s" % key)
