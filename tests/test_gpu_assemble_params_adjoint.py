"""GPU: the derivative of the assembly with respect to the parameters -- Assembler.params_vjp
(mpcasm_assemble_params_vjp; csrc/adjoint.hip) and the layer on top (mpcasm.diff.mpc_solve_diff(params=)) -- against
the long-double Jacobian of tests/params_adjoint_reference.py on the cases of tests/adjoint_cases.py and the extra
limits of tests/params_adjoint_cases.py.  kappa is counted from the plan's tables (params_adjoint_cases.kappa).

The accuracy test prints ``assemble-params-adjoint-precision: ...`` lines (pytest -s) and keeps the worst units per case
in profiles/assemble_params_adjoint_precision.txt."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import adjoint_cases as ac
import params_adjoint_cases as pac
import params_adjoint_reference as pr
from helpers import LD, U64, assert_componentwise, cancellation_free_plants
from mpcasm import capi

pytestmark = pytest.mark.gpu
B = 5
PAD, KEEP = 2, -7.25
NAMES = ac.IDS + ["centres"]
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       "assemble_params_adjoint_precision.txt")
HEAD = ("# Assembler.params_vjp (mpcasm_assemble_params_vjp) at batch 5: the worst error of an element of gparams in units\n"
        "# of u64 M (M: the long-double magnitude of the contraction) and the kappa the test holds it to, counted from\n"
        "# the plan's tables; written by tests/test_gpu_assemble_params_adjoint.py\n")


def record(key, text):
    print("assemble-params-adjoint-precision: %-14s %s" % (key, text))
    try:
        lines = {}
        if os.path.exists(PROFILE):
            for line in open(PROFILE):
                if not line.startswith("#") and line.strip():
                    lines[line[:14].strip()] = line.rstrip("\n")
        lines[key] = "%-14s %s" % (key, text)
        with open(PROFILE, "w") as f:
            f.write(HEAD + "".join(lines[k] + "\n" for k in sorted(lines)))
    except OSError:
        pass


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _vectors(rng, plan, rows):
    """``given, x, u, y, w`` of ``rows`` instances; some rows of ``y`` and ``w`` zero (``w`` wherever ``y`` is)."""
    given, x, u = (rng.normal(size=(rows, n)) for n in (plan.ng, plan.no, plan.no))
    y, w = np.abs(rng.normal(size=(rows, plan.nc))), rng.normal(size=(rows, plan.nc))
    off = rng.random((rows, plan.nc)) < 0.4
    y[off], w[off] = 0.0, 0.0
    return given, x, u, y, w


@functools.lru_cache(maxsize=None)
def setup(name):
    """One case at batch B, computed once and left unchanged: the assembler with per-instance parameters (and
    sources, for the streams ``bound`` and ``lti``), the long-double Jacobian of every instance at its ``given``,
    random ``x, u, y, w`` and what the device made of them."""
    import torch

    from mpcasm import engine, problems

    api = problems.load_api("mpc_interface")
    rng = np.random.default_rng([len(name), NAMES.index(name), 43])
    if name == "centres":
        form, streams, kind = pac.build_centres(api, rng), "shared", "centres"
    else:
        case = ac.CASES[ac.IDS.index(name)]
        form, streams, kind = ac.build(api, rng, case.kind), case.streams, case.kind
    asm = engine.Assembler(form, batch=B, lti=["plant"] if streams == "lti" else ())
    plan = asm.plan
    given, x, u, y, w = _vectors(rng, plan, B)
    tables = A = Bm = None
    src = [{}] * B
    if streams != "shared":
        A, Bm = cancellation_free_plants(rng, B, ac.NS, ac.NI, 0.9, ac.N)
        if streams == "bound":
            S, U = engine.fill_su(A, Bm, ac.N)
            for j in range(ac.NI):
                asm.bind_source(("plant", j), U[:, j].contiguous())
            asm.bind_source(("plant", ac.NI), S)
            tables = (S, U)
            S, U = S.cpu().numpy(), U.cpu().numpy()
            src = [dict(name="plant", tables=(S[b], U[b])) for b in range(B)]
        else:
            asm.bind_lti("plant", torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"))
            src = [dict(name="plant", plant=(A[b], Bm[b])) for b in range(B)]
    params, J, fwd = [], [], []
    for b in range(B):
        ac.vary_params(form, rng)
        params.append(plan.current_params())
        J.append(pr.jacobian(form, plan, given[b], **src[b]))
        fwd.append(pr.forward_magnitude(form, given[b], **src[b]))
    asm.params.copy_(torch.as_tensor(np.stack(params), device="cuda"))
    dev = lambda a: torch.as_tensor(a, device="cuda")
    gp = asm.params_vjp(dev(given), dev(x), dev(u), dev(y), dev(w))
    torch.cuda.synchronize()
    return SimpleNamespace(name=name, form=form, streams=streams, kind=kind, asm=asm, plan=plan, given=given, x=x, u=u,
                           y=y, w=w, J=J, fwd=fwd, params=np.stack(params), src=src, gp=gp.cpu().numpy(),
                           kappa=pac.kappa(plan, generated=streams == "lti"), tables=tables, A=A, Bm=Bm)


def _call(torch, s, asm=None, rows=slice(None), **kw):
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a[rows]), device="cuda")
    return (asm or s.asm).params_vjp(dev(s.given), dev(s.x), dev(s.u), dev(s.y), dev(s.w), **kw)


@pytest.mark.parametrize("name", NAMES)
def test_accuracy(gpu_api, torch_gpu, name):
    """Every element of gparams within kappa u64 M of the long-double reference; exactly +-0 where M == 0 and in the
    slots no record names."""
    s = setup(name)
    worst = 0.0
    unnamed = pac.contributions(s.plan) == 0
    zeros = 0
    for b in range(B):
        ref, mag = pr.vjp_reference(s.J[b], s.x[b], s.u[b], s.y[b], s.w[b])
        worst = max(worst, assert_componentwise(s.gp[b], ref, mag, s.kappa, "%s gparams[%d]" % (name, b)))
        assert not s.gp[b][unnamed].any() and np.all(mag[unnamed] == 0)
        zeros += int(np.count_nonzero(mag == 0))
        assert np.count_nonzero(mag) > 0
    if name.startswith("mix"):
        assert zeros > 0, "an extreme of a line whose w is zero"
    # per-instance parameters and sources really differ between the instances
    assert len({row.tobytes() for row in s.params}) == B
    assert float(np.max(np.abs(s.J[0].dh - s.J[1].dh))) > 0
    record(name, "gparams %6.3f  kappa %d  slots %d" % (worst, s.kappa, s.params.shape[1]))


@pytest.mark.parametrize("name", ["mix-shared", "mix-bound", "mix-lti", "centres"])
def test_against_the_forward_kernels(gpu_api, torch_gpu, name):
    """For a slot of every kind, assemble(params + t e_j) - assemble(params), contracted on the host with the dense
    cotangents, agrees with t gparams[j] within the sum of the two yardsticks: kappa u64 t M_j for the operator and
    forward_kappa u64 times the magnitude of the two assemblies against the same cotangents for the forward kernels
    (M(params + t e_j) <= M(params) + t M_j).  t = fl(theta_j + 1) - theta_j: the difference is exact in t because
    P, q, G, h are affine in the slot."""
    torch = torch_gpu
    s = setup(name)
    slots = s.plan.param_slots
    picks = [("cost", "free", "weight"), ("cost", "free", "aim")]
    if name != "centres":
        picks += [("cost", "plain", "weight"), ("cost", "crossed", "weight"), ("cost", "crossed", "cross_aim"),
                  ("cost", "with L", "aim")]
    nlim = sum(1 for key in slots if key[0] == "limit" and key[2] == "arrow")
    picks += [("limit", nlim - 1, f) for f in ("arrow", "center", "extreme")]
    picks += [("limit", nlim - 2, f) for f in ("arrow", "center", "extreme")]
    kf = ac.forward_kappa(s.plan, generated=s.streams == "lti")
    given = torch.as_tensor(s.given, device="cuda")
    base = [t.clone().cpu().numpy().astype(LD) for t in s.asm.assemble(given)]
    for key in picks:
        start, rows, cols = slots[key]
        j = start + rows * cols - 1
        moved = s.asm.params.clone()
        moved[:, j] += 1.0
        there = [t.clone().cpu().numpy().astype(LD) for t in s.asm.assemble(given, params=moved)]
        t = moved[:, j].cpu().numpy().astype(LD) - s.params[:, j].astype(LD)
        seen = False
        for b in range(B):
            value, cot = pr.cotangents(s.x[b], s.u[b], s.y[b], s.w[b])
            dP, dq, dG, dh = (there[i][b] - base[i][b] for i in range(4))
            theirs = pr.contract(value, dP[None], dq[None], dG[None], dh[None])[0]
            _, mag = pr.vjp_reference(s.J[b], s.x[b], s.u[b], s.y[b], s.w[b])
            MG, Mh, MP, Mq = s.fwd[b]
            whole = pr.contract(cot, MP[None], Mq[None], MG[None], Mh[None])[0]
            bound = U64 * (s.kappa * t[b] * mag[j] + kf * (2 * whole + t[b] * mag[j]))
            assert abs(t[b] * LD(s.gp[b][j]) - theirs) <= bound, (name, key, b)
            seen = seen or mag[j] > 0
        assert seen, (name, key)


def _alone(torch, s, b, engine):
    """Instance ``b`` of the case in a batch of its own (another assembler: its parameters and sources at place 0)."""
    one = engine.Assembler(s.form, batch=1, lti=["plant"] if s.streams == "lti" else ())
    one.params.copy_(torch.as_tensor(s.params[b:b + 1], device="cuda"))
    if s.streams == "bound":
        S, U = s.tables
        for j in range(ac.NI):
            one.bind_source(("plant", j), U[b:b + 1, j].contiguous())
        one.bind_source(("plant", ac.NI), S[b:b + 1].contiguous())
    elif s.streams == "lti":
        one.bind_lti("plant", torch.as_tensor(s.A[b:b + 1], device="cuda"), torch.as_tensor(s.Bm[b:b + 1], device="cuda"))
    return _call(torch, s, one, slice(b, b + 1)).cpu().numpy()[0]


@pytest.mark.parametrize("name", ["mix-shared", "mix-bound", "mix-lti"])
def test_an_instance_does_not_depend_on_its_batch(gpu_api, torch_gpu, name):
    """Batch 5 against batch 1: instance b equals, bit for bit, the same instance run alone; two calls give the same
    bits; a tensor handed in as ``params=`` gives the bits of the assembler's own."""
    torch = torch_gpu
    from mpcasm import engine

    s = setup(name)
    assert same(_call(torch, s).cpu().numpy(), s.gp)
    assert same(_call(torch, s, params=s.asm.params.clone()).cpu().numpy(), s.gp)
    for b in (0, 3):
        assert same(_alone(torch, s, b, engine), s.gp[b]), b
    assert not same(s.gp[0], s.gp[3])


def test_more_instances_than_resident_workgroups(gpu_api, torch_gpu):
    """The smallest case at CUs x resident workgroups + 3 instances, every instance with parameters of its own: the
    grid-stride loop takes a second trip.  Instances on either side of the grid's edge equal the same instance run
    alone, bit for bit; two calls give identical bits."""
    torch = torch_gpu
    from mpcasm import engine, problems

    api = problems.load_api("mpc_interface")
    rng = np.random.default_rng(19)
    form = ac.build(api, rng, "diag")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    one = engine.Assembler(form, batch=1)
    grid = cus * one.params_adjoint_info().per_cu
    n = grid + 3
    asm = engine.Assembler(form, batch=n)
    assert asm.params_adjoint_info().per_cu * cus == grid
    gen = torch.Generator(device="cuda").manual_seed(3)
    f = dict(dtype=torch.float64, device="cuda", generator=gen)
    asm.params.mul_(0.5 + torch.rand(asm.params.shape, **f))
    given, x, u = (torch.randn((n, k), **f) for k in (asm.ng, asm.no, asm.no))
    y, w = torch.rand((n, asm.nc), **f), torch.randn((n, asm.nc), **f)
    gp = asm.params_vjp(given, x, u, y, w).clone()
    again = asm.params_vjp(given, x, u, y, w)
    assert torch.equal(gp.view(torch.int64), again.view(torch.int64))
    for b in (0, grid - 1, grid, n - 1):
        one.params.copy_(asm.params[b:b + 1])
        alone = one.params_vjp(*(t[b:b + 1] for t in (given, x, u, y, w)))
        assert torch.equal(gp[b].view(torch.int64), alone[0].view(torch.int64)), b
    assert not torch.equal(asm.params[0], asm.params[grid])
    assert bool(gp.abs().sum(dim=1).min() > 0)


def _padded(torch, rows, width):
    whole = torch.full((rows + 2 * PAD, width), float("nan"), dtype=torch.float64, device="cuda")
    whole[PAD:PAD + rows] = KEEP
    return whole


def test_nothing_outside_the_result_is_written(gpu_api, torch_gpu):
    """The result in a buffer with guard rows either side and a sentinel inside: a call on ``count`` instances writes
    their rows and nothing else; ``count == 0`` writes nothing; a null operand is refused."""
    torch = torch_gpu
    s = setup("mix-shared")
    asm, width = s.asm, s.params.shape[1]
    guards = lambda t: bool(torch.isnan(t[:PAD]).all()) and bool(torch.isnan(t[PAD + B:]).all())
    count = 3
    whole = _padded(torch, B, width)
    _call(torch, s, out=whole[PAD:PAD + B], count=count)
    torch.cuda.synchronize()
    assert same(whole[PAD:PAD + count].cpu().numpy(), s.gp[:count])
    assert bool((whole[PAD + count:PAD + B] == KEEP).all()) and guards(whole)
    whole = _padded(torch, B, width)
    _call(torch, s, out=whole[PAD:PAD + B])
    torch.cuda.synchronize()
    assert same(whole[PAD:PAD + B].cpu().numpy(), s.gp) and guards(whole)
    whole = _padded(torch, B, width)
    _call(torch, s, out=whole[PAD:PAD + B], count=0)
    torch.cuda.synchronize()
    assert bool((whole[PAD:PAD + B] == KEEP).all()) and guards(whole)
    lib, (ptrs, strides) = capi.load(), asm._src_args()
    dev = lambda a: torch.as_tensor(a, device="cuda")
    g, x, u, y, w = (dev(a) for a in (s.given, s.x, s.u, s.y, s.w))
    args = lambda **null: [None if k in null else t.data_ptr() for k, t in
                           (("g", g), ("x", x), ("u", u), ("y", y), ("w", w))]
    for null in ("g", "x", "u", "y", "w"):
        rc = lib.mpcasm_assemble_params_vjp(asm._handle, ptrs, strides, asm.params.data_ptr(), *args(**{null: 1}), None,
                                            whole[PAD:].data_ptr(), asm._workspace().data_ptr(), B, None)
        assert rc == capi.ERR_ARG, null
    rc = lib.mpcasm_assemble_params_vjp(asm._handle, ptrs, strides, asm.params.data_ptr(), *args(), None, None,
                                        asm._workspace().data_ptr(), B, None)
    assert rc == capi.ERR_ARG
    torch.cuda.synchronize()
    assert bool((whole[PAD:PAD + B] == KEEP).all()) and guards(whole)


def test_instances_that_are_not_done_get_a_zero_row(gpu_api, torch_gpu):
    """With ``verdict``: an instance that is not SENS_DONE comes out exactly zero although its ``x`` and ``y`` hold
    NaN (nothing of it is read); the others have the bits of the call without ``verdict``.  ``active`` zeroes ``y``
    off the set before the call."""
    torch = torch_gpu
    s = setup("mix-shared")
    verdict = torch.full((B,), capi.SENS_DONE, dtype=torch.int32, device="cuda")
    verdict[1], verdict[4] = 0, -3
    x, y = s.x.copy(), s.y.copy()
    x[1], y[4] = np.nan, np.nan
    dev = lambda a: torch.as_tensor(a, device="cuda")
    out = torch.full((B, s.params.shape[1]), KEEP, dtype=torch.float64, device="cuda")
    s.asm.params_vjp(dev(s.given), dev(x), dev(s.u), dev(y), dev(s.w), verdict=verdict, out=out)
    got = out.cpu().numpy()
    for b in range(B):
        if b in (1, 4):
            assert not got[b].any() and not np.signbit(got[b]).any(), b
        else:
            assert same(got[b], s.gp[b]), b
    # active: y with other numbers off the set gives the bits of y with zeros there
    active = dev(s.y != 0)
    noisy = np.where(s.y != 0, s.y, 3.5)
    got = s.asm.params_vjp(dev(s.given), dev(s.x), dev(s.u), dev(noisy), dev(s.w), active=active).cpu().numpy()
    assert same(got, s.gp)


def test_a_plan_compiled_as_ltv_is_refused(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine, problems

    api = problems.load_api("mpc_interface")
    swp = engine.Assembler(problems.lipm_ltv(api, N=12), batch=2, ltv=["LIP"])
    z = lambda n: torch.zeros((2, n), dtype=torch.float64, device="cuda")
    with pytest.raises(capi.MpcasmError):
        swp.params_vjp(z(swp.ng), z(swp.no), z(swp.no), z(swp.nc), z(swp.nc))
    with pytest.raises(capi.MpcasmError):
        swp.params_adjoint_info()


def _mix_loop(torch, engine, problems):
    """Solvable instances of the ``mix`` formulation at batch 5 with parameters of their own -- the plain cost's aims
    far out, so that seven of the twenty lines are active at the solution (tests/osqp_restatement.py on the host says
    so), the crossed cost at weight 0 (a product of two outputs is not convex; its gradient is checked all the same)
    --, the long-double Jacobian of each, and instance 2 made unsolvable (every extreme at -1e3)."""
    api = problems.load_api("mpc_interface")
    rng = np.random.default_rng(37)
    form = ac.build(api, rng, "mix")
    form.goals["plain"].update(aim=[[5.0, -4.0]])
    form.goals["crossed"].weight = 0.0
    asm = engine.Assembler(form, batch=B)
    given = rng.normal(0, 0.05, (B, asm.ng))
    params, J = [], []
    for b in range(B):
        for cost in form.goals.values():
            cost.weight = float(cost.weight * rng.uniform(0.8, 1.25))
        params.append(asm.plan.current_params())
        J.append(pr.jacobian(form, asm.plan, given[b]))
    p = torch.as_tensor(np.stack(params), device="cuda")
    for key in asm.plan.param_slots:
        if key[0] == "limit" and key[2] == "extreme":
            p[2, asm.param_slice(*key)[0]] = -1e3
    c, d = rng.normal(size=(B, asm.no)), rng.normal(size=(B, asm.nc))
    dev = lambda a: torch.as_tensor(a, device="cuda")
    return asm, dev(given), p, dev(c), dev(d), J


def test_the_layer(gpu_api, torch_gpu):
    """mpc_solve_diff(asm, given, params=p) with a loss on x and y: p.grad equals the host contraction of the
    long-double Jacobian with the (x, u, y . active, w) of the outcome within kappa u64 M (the sensitivity solve is
    shared with the call without params=: only the contraction is new); its ``active`` is (h - z) < y recomputed on
    the host; the instance that does not solve gets a zero row; given.grad is bit-identical to the call without
    params= when p is asm.params; param_grad reads a field."""
    torch = torch_gpu
    from mpcasm import diff, engine, problems

    asm, given, p, c, d, J = _mix_loop(torch, engine, problems)
    p.requires_grad_(True)
    g = given.clone().requires_grad_(True)
    res = diff.mpc_solve_diff(asm, g, params=p)
    assert res.verdict is None and res.active is None and res.x.requires_grad
    ((c * res.x).sum() + (d * res.y).sum()).backward()
    o = res._outcome
    s = engine.qp_sensitivity(o.P, o.G, o.h, res.sol, c, d, status=res.sol.status)
    assert torch.equal(res.verdict, s.verdict)
    verdict = s.verdict.tolist()
    assert verdict[2] != capi.SENS_DONE and verdict.count(capi.SENS_DONE) >= 3, verdict
    h, z, y = (t.cpu().numpy() for t in (o.h, res.sol.z, res.sol.y))
    active = (h - z) < y
    assert np.array_equal(res.active.cpu().numpy(), active)
    x, u, w = (t.cpu().numpy() for t in (res.sol.x, s.u, s.w))
    grad = p.grad.cpu().numpy()
    kappa = pac.kappa(asm.plan)
    some_active = False
    for b in range(B):
        if verdict[b] != capi.SENS_DONE:
            assert not grad[b].any(), b
            continue
        some_active = some_active or bool(active[b].any())
        ref, mag = pr.vjp_reference(J[b], x[b], u[b], np.where(active[b], y[b], 0.0), w[b])
        assert_componentwise(grad[b], ref, mag, kappa, "layer gparams[%d]" % b)
        assert grad[b].any(), b
    assert some_active, "no instance has an active line: the limits' gradients are not exercised"
    view = asm.param_grad(p.grad, "cost", "plain", "aim")
    start = asm.plan.param_slots[("cost", "plain", "aim")][0]
    assert tuple(view.shape) == (B, 1, 2) and torch.equal(view[:, 0], p.grad[:, start:start + 2])
    # given.grad: the same bits as the call without params= when p is asm.params
    asm.params.copy_(p.detach())
    g1, g2 = given.clone().requires_grad_(True), given.clone().requires_grad_(True)
    for gi, kw in ((g1, {}), (g2, dict(params=asm.params))):
        r = diff.mpc_solve_diff(asm, gi, **kw)
        ((c * r.x).sum() + (d * r.y).sum()).backward()
    assert torch.equal(g1.grad.view(torch.int64), g2.grad.view(torch.int64))
    assert torch.equal(g1.grad.view(torch.int64), g.grad.view(torch.int64))
    for kw in (dict(soft=(1.0, 0.0)), dict(polish=True)):
        with pytest.raises(ValueError):
            diff.mpc_solve_diff(asm, given, params=p.detach(), **kw)


def test_repeated_calls_do_not_grow_device_memory(gpu_api, torch_gpu):
    import gc

    torch = torch_gpu
    from mpcasm import diff, engine, problems

    asm, given, p, c, d, _ = _mix_loop(torch, engine, problems)

    def call():
        g, q = given.clone().requires_grad_(True), p.clone().requires_grad_(True)
        res = diff.mpc_solve_diff(asm, g, params=q)
        ((c * res.x).sum() + (d * res.y).sum()).backward()

    for _ in range(2):
        call()
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for _ in range(4):
        call()
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
