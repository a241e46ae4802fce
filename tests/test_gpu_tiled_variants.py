"""GPU: every variant of the tiled path (csrc/tiled.hip) against extended precision.  The family of tiled_cases.py
spans what tiled_choose can select (test_tiled_routes_cpu.py holds it to that); here each case first asserts that
the library takes the route its entry pins (Assembler.tiled_route, the launch's own decision, and last_kernel), then
assembles into NaN-filled buffers -- every instance its own plant (A, B) and its own given; the shared-model cases
one system for the batch and every instance its own weights, aims, arrows, centres and extremes -- and holds P, q,
G, h of sampled instances element by element to |x - x*| <= kappa (u M + 2^-1022), kappa = 2 N (n + 1) (helpers.py),
x* the oracle in long double on the very fp64 inputs.  Cases marked ``halves`` then launch one half at a time: the
wanted half bit for bit the full call's, the other buffers untouched."""
import numpy as np
import pytest

import sweep_cases as sc
import tiled_cases as tc
from helpers import assert_componentwise, kappa, precise_reference

pytestmark = pytest.mark.gpu

KERNEL = {tc.SCAN: "toeplitz_scan_kernel", tc.TOEPLITZ: "tiled_assemble_kernel", tc.SHARED: "shared_p_kernel",
          tc.GENERAL: "tiled_assemble_kernel"}
# the long-double references, by the inputs they belong to: a shape's fused, pre-pass, Toeplitz and general cases
# run on the same plants, formulation and given (the seed follows from the shape alone)
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


def _inputs_key(case):
    s = case.shape
    return (s.kind, s.n, s.m, s.N, s.tracked, s.kw, case.batch)


def _set_up(api, torch, case):
    """The assembler of ``case`` with its sources bound, its parameters and its given."""
    from mpcasm import capi, engine

    shape, batch = case.shape, case.batch
    shared = shape.kind == "shared"
    rng = np.random.default_rng(7000 + 1000 * shape.n + 10 * shape.N + shape.m + len(shape.kw) + (500 if shared else 0))
    A, Bm = tc.plants(rng, 1 if shared else batch, shape)
    form = tc.build(api, rng, shape, (A[0], Bm[0]))
    given = rng.normal(0, 0.3, [batch, form.given_len])
    if shared:
        asm = engine.Assembler(form, batch=batch)
        params = sc.perturb_params(asm.plan, asm.params.cpu().numpy().copy(), rng)
        asm.params.copy_(torch.as_tensor(params, device="cuda"))
        A, Bm = np.broadcast_to(A[0], (batch,) + A[0].shape), np.broadcast_to(Bm[0], (batch,) + Bm[0].shape)
    else:
        asm = engine.Assembler(form, batch=batch, lti=["plant"])
        asm.bind_lti("plant", torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"))
        params = asm.params.cpu().numpy().copy()
    asm.set_option(capi.OPT_PATH, case.path)
    return form, asm, A, Bm, params, given


def _assert_route(asm, case, **want):
    r = asm.tiled_route(**want)
    pinned = tc.Route(r.form, r.fused, r.kp, r.cb, r.rows_in_lds, r.whole_lines, r.whole_lds, r.tables, r.tg, r.sym, None)
    expect = case.route._replace(lds=None)
    if want.get("want_cost") is False:
        expect = expect._replace(tg=0)
    assert pinned == expect, r
    if case.route.lds is not None:
        assert r.lds == case.route.lds


@pytest.mark.parametrize("case", tc.GPU_CASES, ids=[c.shape.name for c in tc.GPU_CASES])
def test_variant(gpu_api, torch_gpu, case):
    torch = torch_gpu
    shape, batch = case.shape, case.batch
    form, asm, A, Bm, params, given = _set_up(gpu_api, torch, case)
    _assert_route(asm, case)
    g = torch.as_tensor(given, device="cuda")
    full = _nan_out(torch, asm)
    asm.assemble(g, out=full)
    assert asm.last_kernel().startswith(KERNEL[case.route.form]), asm.last_kernel()
    res = {key: t.cpu().numpy() for key, t in zip("PqGh", full)}
    kap, worst = kappa(shape.N, shape.n), 0.0
    samples = (0, batch - 1) if asm.no >= 384 else (0, batch // 2, batch - 1)
    refs = _REFERENCES.setdefault(_inputs_key(case), {})
    with sc.instance_params(form, asm.plan) as objects:
        for b in samples:
            if b not in refs:
                objects.set(params[b])
                refs[b] = precise_reference(form, "plant", A[b], Bm[b], given[b])
            for key, x in res.items():
                worst = max(worst, assert_componentwise(x[b], *refs[b][key], kap,
                                                        "%s, instance %d, %s" % (shape.name, b, key)))
    if case.halves:
        # one half at a time, into fresh NaN buffers: the wanted half bit for bit, the other one untouched
        for want in (dict(want_constraints=False), dict(want_cost=False)):
            _assert_route(asm, case, **want)
            out = _nan_out(torch, asm)
            asm.assemble(g, out=out, **want)
            assert asm.last_kernel().startswith(KERNEL[case.route.form]), asm.last_kernel()
            cost_half = "want_constraints" in want
            for i, (mine, ref) in enumerate(zip(out, full)):
                if (i < 2) == cost_half:
                    assert torch.equal(mine, ref), "%s %s" % ("PqGh"[i], want)
                else:
                    assert bool(torch.isnan(mine).all()), "%s written with %s" % ("PqGh"[i], want)
    r = case.route
    what = {tc.SCAN: "scan <%d,%d> %s" % (r.kp, r.cb, "fused" if r.fused else "pre-pass"), tc.TOEPLITZ: "toeplitz",
            tc.SHARED: "shared TG %d" % r.tg, tc.GENERAL: "general"}[r.form]
    print("componentwise %-60s worst %8.3g u M   kappa %d" % ("tiled %s %s" % (what, shape.name), worst, kap))
