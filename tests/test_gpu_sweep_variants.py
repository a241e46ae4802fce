"""GPU: every instantiation of the sweep kernel (csrc/sweep.hip) and every path of its lines of G against
extended precision.  The family of sweep_cases.py spans what sweep_choose can select (test_sweep_routes_cpu.py holds
it to that); here each case first asserts that the library takes the route its entry pins (Assembler.sweep_route,
the launch's own decision), then assembles into NaN-filled buffers -- every instance its own per-step plant, its own
weights, aims, arrows, centres and extremes, its own initial state -- and holds P, q, G, h element by element to
|x - x*| <= kappa (u M + 2^-1022), kappa = 2 N (n + 1) (helpers.py), x* the oracle in long double on the very fp64
inputs.  Then one half at a time: the wanted half bit for bit the full call's, the other buffers untouched."""
import numpy as np
import pytest

import sweep_cases as sc
from helpers import RTOL_TIGHT, assert_componentwise, kappa

pytestmark = pytest.mark.gpu

B = 5
CHECK_ALL_UP_TO = 130       # unknowns up to which every instance is checked (the reference: under 0.2 s each)
CASES = [c for c in sc.CASES if c.shape.name not in ("four-full", "over")]
SHARED_A = ["one-4-4-63", "desc", "two-n1", "four-a4-n4"]      # one case per CPT: 1, 2 PAIR, 2, 4


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _rel(x, ref):
    scale = ref.abs().max()
    err = (x - ref).abs().max()
    return float(err / scale) if float(scale) > 0 else float(err)


def _nan_out(torch, asm):
    f = dict(dtype=torch.float64, device="cuda")
    n, no, nc = asm.batch, asm.no, asm.nc
    return tuple(torch.full(s, float("nan"), **f) for s in ((n, no, no), (n, no), (n, nc, no), (n, nc)))


def _report(what, worst, kap):
    print("componentwise %-60s worst %8.3g u M   kappa %d" % (what, worst, kap))


def _set_up(api, torch, case, batch, seed, shared_a=False):
    """The assembler of ``case`` with every instance's own plant, parameters and initial state."""
    from mpcasm import engine

    rng = np.random.default_rng(seed)
    A, Bm = sc.plants(rng, batch, case.shape)
    form = sc.build(api, rng, case.shape, plant=(A[0, 0], Bm[0, 0]))
    name = sc.dynamics_name(case.shape)
    asm = engine.Assembler(form, batch=batch, ltv=[name])
    if shared_a:                # (one A_k for the batch beside a B_k per instance: stride 0 beside a stride)
        A = np.broadcast_to(A[0], A.shape).copy()
    asm.bind_ltv(name, torch.as_tensor(A[0] if shared_a else A, device="cuda"), torch.as_tensor(Bm, device="cuda"))
    params = sc.perturb_params(asm.plan, asm.params.cpu().numpy().copy(), rng)
    asm.params.copy_(torch.as_tensor(params, device="cuda"))
    given = rng.normal(0, 0.3, [batch, form.given_len])
    return form, name, asm, A, Bm, params, given


def _assemble_and_check(api, torch, case, shared_a=False):
    shape = case.shape
    form, name, asm, A, Bm, params, given = _set_up(api, torch, case, B, 1000 + len(shape.name) + shape.N, shared_a)
    assert sc.Route(*asm.sweep_route()[:6]) == case.route, asm.sweep_route()
    g = torch.as_tensor(given, device="cuda")
    full = _nan_out(torch, asm)
    asm.assemble(g, out=full)
    assert "sweep" in asm.last_kernel(), asm.last_kernel()
    res = {key: t.cpu().numpy() for key, t in zip("PqGh", full) if asm.nc or key in "Pq"}
    kap, worst = kappa(shape.N, shape.n), 0.0
    with sc.instance_params(form, asm.plan) as objects:
        for b in (range(B) if case.no <= CHECK_ALL_UP_TO else (0, B - 1)):
            objects.set(params[b])
            ref = sc.reference(form, name, A[b], Bm[b], given[b])
            assert set(ref) >= set(res)
            for key, x in res.items():
                worst = max(worst, assert_componentwise(x[b], *ref[key], kap,
                                                        "%s, instance %d, %s" % (shape.name, b, key)))
    return asm, g, full, worst, kap


@pytest.mark.parametrize("case", CASES, ids=[c.shape.name for c in CASES])
def test_variant(gpu_api, torch_gpu, case):
    torch = torch_gpu
    asm, g, full, worst, kap = _assemble_and_check(gpu_api, torch, case)
    # one half at a time, into fresh NaN buffers: the wanted half bit for bit, the other one untouched
    halves = [dict(want_constraints=False)] + ([dict(want_cost=False)] if asm.nc else [])   # (no limit: no other half)
    for want in halves:
        out = _nan_out(torch, asm)
        asm.assemble(g, out=out, **want)
        assert "sweep" in asm.last_kernel()
        cost_half = "want_constraints" in want
        for i, (mine, ref) in enumerate(zip(out, full)):
            if (i < 2) == cost_half:
                assert torch.equal(mine, ref), "%s %s" % ("PqGh"[i], want)
            else:
                assert bool(torch.isnan(mine).all()), "%s written with %s" % ("PqGh"[i], want)
    r = case.route
    _report("sweep <%d,%s%s> %s %s" % (r.cpt, "3,1,2" if r.specialised else "0,0,0", ",PAIR" if r.pair else "",
                                       sc.mode_of(r), case.shape.name), worst, kap)


@pytest.mark.parametrize("name", SHARED_A)
def test_a_shared_by_the_batch(gpu_api, torch_gpu, name):
    """(A_k) bound once for the batch, (B_k) per instance: a stride of 0 beside one that is not."""
    case = sc.BY_NAME[name]
    asm, _, _, worst, kap = _assemble_and_check(gpu_api, torch_gpu, case, shared_a=True)
    name_id = asm.plan.ltv[0]["ids"]
    assert asm._src_stride[name_id[0]] == 0 and asm._src_stride[name_id[1]] > 0
    _report("sweep CPT %d%s shared A %s" % (case.route.cpt, " PAIR" if case.route.pair else "", name), worst, kap)


def test_the_widest_plan(gpu_api, torch_gpu):
    """1024 unknowns, every thread four live columns.  The long-double reference of P takes a minute per instance:
    P and every other block against the device's fill + staged-assembly route (as test_gpu_sweep.py's random
    systems), q and h (no limit here: q) element by element against extended precision from S, U alone."""
    torch = torch_gpu
    from mpcasm import capi, engine

    case, batch = sc.BY_NAME["four-full"], 3
    shape = case.shape
    form, name, asm, A, Bm, params, given = _set_up(gpu_api, torch, case, batch, 77)
    assert sc.Route(*asm.sweep_route()[:6]) == case.route and asm.no == 1024
    g = torch.as_tensor(given, device="cuda")
    mine = _nan_out(torch, asm)
    asm.assemble(g, out=mine)
    assert "sweep" in asm.last_kernel()
    live = [t for t in mine if t.numel()]
    assert not any(torch.isnan(t).any().item() for t in live)
    assert _rel(mine[0].transpose(1, 2), mine[0]) <= RTOL_TIGHT
    ref = engine.Assembler(form, batch=batch)
    assert ref.plan.param_slots == asm.plan.param_slots
    ref.params.copy_(asm.params)
    ref.set_option(capi.OPT_PATH, 2)
    S, U = engine.fill_su(torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"), shape.N, ltv=True)
    for j in range(shape.m):
        ref.bind_source((name, j), U[:, j])
    ref.bind_source((name, shape.m), S)
    for x, y in zip(mine, ref.assemble(g)):
        if y is not None and y.numel():
            assert _rel(x, y) <= 1e-12
    kap, worst = kappa(shape.N, shape.n), 0.0
    q = mine[1].cpu().numpy()
    with sc.instance_params(form, asm.plan) as objects:
        for b in (0, batch - 1):
            objects.set(params[b])
            pair = sc.reference(form, name, A[b], Bm[b], given[b], want_P=False)
            assert set(pair) == {"q"}
            worst = max(worst, assert_componentwise(q[b], *pair["q"], kap, "four-full, instance %d, q" % b))
    _report("sweep <4,0,0,0> four-full (q; P against fill + staged)", worst, kap)


def test_more_than_1024_unknowns_are_refused(gpu_api, torch_gpu):
    """The launch's refusal, MPCASM_ERR_LIMIT, from whichever call makes it: nothing is written."""
    torch = torch_gpu
    from mpcasm import capi, engine
    from mpcasm.plan import compile_plan

    case = sc.BY_NAME["over"]
    rng = np.random.default_rng(5)
    form = sc.build(gpu_api, rng, case.shape)
    with pytest.raises(capi.MpcasmError) as refusal:
        engine.sweep_route(compile_plan(form, ltv=["plant"]))
    assert refusal.value.status == capi.ERR_LIMIT
    try:
        asm = engine.Assembler(form, batch=2, ltv=["plant"])
    except capi.MpcasmError as refusal:
        assert refusal.status == capi.ERR_LIMIT
        return
    assert asm.no == 1028
    out = _nan_out(torch, asm)
    with pytest.raises(capi.MpcasmError) as refusal:
        asm.assemble(torch.zeros(2, form.given_len, dtype=torch.float64, device="cuda"), out=out)
    assert refusal.value.status == capi.ERR_LIMIT
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in out)
    with pytest.raises(capi.MpcasmError) as refusal:
        asm.sweep_route()
    assert refusal.value.status == capi.ERR_LIMIT
