"""GPU: the derivative of the assembly with respect to ``given`` -- Assembler.given_jvp / given_vjp
(mpcasm_assemble_jvp, mpcasm_assemble_vjp; csrc/adjoint.hip) and the layer on top (mpcasm.diff.mpc_solve_diff,
tangent) -- against the long-double Jacobian of tests/adjoint_reference.py on the cases of tests/adjoint_cases.py,
problems.body_case and the reduced biped.  kappa is counted from the plan's tables (adjoint_cases.kappa).

The accuracy test prints ``assemble-adjoint-precision: ...`` lines (pytest -s) and keeps the worst units per case in
profiles/assemble_adjoint_precision.txt."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import adjoint_cases as ac
import adjoint_reference as ar
from helpers import LD, U64, assert_componentwise, cancellation_free_plants
from mpcasm import capi

pytestmark = pytest.mark.gpu
B = 5
PAD, KEEP = 2, -7.25
NAMES = ac.IDS + ["body", "biped"]
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       "assemble_adjoint_precision.txt")
HEAD = ("# Assembler.given_jvp / given_vjp (mpcasm_assemble_jvp, mpcasm_assemble_vjp) at batch 5: the worst error of an\n"
        "# element of dq, dh, ggiven in units of u64 M (M: the long-double magnitude |J||d|, |J|'|g|) and the kappa the\n"
        "# test holds it to, counted from the plan's tables; written by tests/test_gpu_assemble_adjoint.py\n")


def record(key, text):
    print("assemble-adjoint-precision: %-14s %s" % (key, text))
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


def _form(api, rng, name):
    from mpcasm import problems

    if name == "body":
        return problems.body_case(api), "shared", "mix"
    if name == "biped":
        form = problems.biped(api, problems.BipedConfig(step_samples=8), reduced=True)
        form.update(step_times=np.array([6, 14]), step_count=0)
        return form, "shared", "mix"
    case = ac.CASES[ac.IDS.index(name)]
    return ac.build(api, rng, case.kind), case.streams, case.kind


@functools.lru_cache(maxsize=None)
def setup(name):
    """One case at batch B, computed once and left unchanged: the assembler with per-instance parameters (and
    sources, for the streams ``bound`` and ``lti``), the long-double Jacobian of every instance, random ``d, gq, gh``
    and what the device made of them."""
    import torch

    from mpcasm import engine, problems

    api = problems.load_api("mpc_interface")
    rng = np.random.default_rng([len(name), NAMES.index(name), 41])
    form, streams, kind = _form(api, rng, name)
    asm = engine.Assembler(form, batch=B, lti=["plant"] if streams == "lti" else ())
    plan = asm.plan
    ng, no, nc = plan.ng, plan.no, plan.nc
    d, gq, gh = rng.normal(size=(B, ng)), rng.normal(size=(B, no)), rng.normal(size=(B, nc))
    src, tables = {}, None
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
    else:
        src = [{}] * B
    params, J, fwd = [], [], []
    for b in range(B):
        ac.vary_params(form, rng)
        params.append(plan.current_params())
        J.append(ar.jacobian(form, **src[b]))
        fwd.append([ar.forward_magnitude(form, g, **src[b]) for g in (d[b], np.zeros(ng))])
    asm.params.copy_(torch.as_tensor(np.stack(params), device="cuda"))
    dev = lambda a: torch.as_tensor(a, device="cuda")
    dq, dh = asm.given_jvp(dev(d))
    gg = asm.given_vjp(dev(gq), dev(gh))
    torch.cuda.synchronize()
    return SimpleNamespace(name=name, form=form, streams=streams, kind=kind, asm=asm, plan=plan, d=d, gq=gq, gh=gh, J=J,
                           fwd=fwd, params=np.stack(params), src=src, dq=dq.cpu().numpy(), dh=dh.cpu().numpy(),
                           gg=gg.cpu().numpy(), kappa=ac.kappa(plan, generated=streams == "lti"),
                           tables=tables, A=A if streams != "shared" else None, Bm=Bm if streams != "shared" else None)


@pytest.mark.parametrize("name", NAMES)
def test_accuracy(gpu_api, torch_gpu, name):
    """Every element of dq, dh, ggiven within kappa u64 M of the long-double reference; exactly +-0 where M == 0 (the
    given columns nothing reads; all of dq where every cost is on a free variable).  The NULL halves: ggiven of gq
    alone and of gh alone, each against its own reference."""
    torch = torch_gpu
    s = setup(name)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    only_q = s.asm.given_vjp(dev(s.gq), None).cpu().numpy()
    only_h = s.asm.given_vjp(None, dev(s.gh)).cpu().numpy() if s.plan.nc else None
    worst = dict(dq=0.0, dh=0.0, ggiven=0.0)
    for b in range(B):
        (dq_ref, dq_mag), (dh_ref, dh_mag) = ar.jvp_reference(s.J[b], s.d[b])
        worst["dq"] = max(worst["dq"], assert_componentwise(s.dq[b], dq_ref, dq_mag, s.kappa, "%s dq[%d]" % (name, b)))
        worst["dh"] = max(worst["dh"], assert_componentwise(s.dh[b], dh_ref, dh_mag, s.kappa, "%s dh[%d]" % (name, b)))
        for got, cq, ch in ((s.gg, s.gq[b], s.gh[b]), (only_q, s.gq[b], None), (only_h, None, s.gh[b])):
            if got is not None:
                units = assert_componentwise(got[b], *ar.vjp_reference(s.J[b], cq, ch), s.kappa,
                                             "%s ggiven[%d]" % (name, b))
                worst["ggiven"] = max(worst["ggiven"], units)
        if s.kind == "diag":
            assert not s.dq[b].any() and not only_q[b].any()
        if name in ac.IDS:
            idle = ac.unread_given_columns(s.form)
            assert not s.gg[b][idle].any() and np.all(ar.vjp_reference(s.J[b], s.gq[b], s.gh[b])[1][idle] == 0)
    # per-instance parameters and sources really differ between the instances
    assert len({row.tobytes() for row in s.params}) == B
    assert float(np.max(np.abs(s.J[0].Jh - s.J[1].Jh))) > 0
    record(name, "dq %6.3f  dh %6.3f  ggiven %6.3f  kappa %d" % (worst["dq"], worst["dh"], worst["ggiven"], s.kappa))


@pytest.mark.parametrize("name", NAMES)
def test_adjointness(gpu_api, torch_gpu, name):
    """<gq, dq> + <gh, dh> and <ggiven, d> differ by no more than kappa u64 times the sum of the two magnitudes."""
    s = setup(name)
    for b in range(B):
        (_, dq_mag), (_, dh_mag) = ar.jvp_reference(s.J[b], s.d[b])
        left = s.gq[b].astype(LD) @ s.dq[b].astype(LD) + s.gh[b].astype(LD) @ s.dh[b].astype(LD)
        right = s.gg[b].astype(LD) @ s.d[b].astype(LD)
        mag = np.abs(s.gq[b]) @ dq_mag + np.abs(s.gh[b]) @ dh_mag + \
            ar.vjp_reference(s.J[b], s.gq[b], s.gh[b])[1] @ np.abs(s.d[b])
        assert abs(left - right) <= s.kappa * U64 * mag, (name, b, float(abs(left - right) / (U64 * mag)))


@pytest.mark.parametrize("name", NAMES)
def test_against_the_forward_kernels(gpu_api, torch_gpu, name):
    """dq and dh agree with assemble(d) - assemble(0) within the sum of the two yardsticks: kappa u64 |J||d| for the
    operator, forward_kappa u64 (M(d) + M(0)) for the two assemblies (M: the oracle's magnitude of q, h)."""
    torch = torch_gpu
    s = setup(name)
    at = lambda g: [t.clone().cpu().numpy() for t in s.asm.assemble(torch.as_tensor(g, device="cuda"))]
    _, q1, _, h1 = at(s.d)
    _, q0, _, h0 = at(np.zeros_like(s.d))
    kf = ac.forward_kappa(s.plan, generated=s.streams == "lti")
    for b in range(B):
        (_, dq_mag), (_, dh_mag) = ar.jvp_reference(s.J[b], s.d[b])
        (mq1, mh1), (mq0, mh0) = s.fwd[b]
        pairs = [(s.dq[b], q1[b] - q0[b], dq_mag, mq1 + mq0)]
        if s.plan.nc:
            pairs.append((s.dh[b], h1[b] - h0[b], dh_mag, mh1 + mh0))
        for mine, theirs, mag, fmag in pairs:
            bound = U64 * (s.kappa * mag + kf * fmag)
            assert np.all(np.abs(mine.astype(LD) - theirs.astype(LD)) <= bound), (name, b)


def _alone(torch, s, b, engine):
    """Instance ``b`` of the case in a batch of its own (another assembler: its parameters and sources at place 0)."""
    one = engine.Assembler(s.form, batch=1, lti=["plant"] if s.streams == "lti" else ())
    one.params.copy_(torch.as_tensor(s.params[b:b + 1], device="cuda"))
    if s.streams == "bound":
        S, U = s.tables                    # (the very tables the batch read)
        for j in range(ac.NI):
            one.bind_source(("plant", j), U[b:b + 1, j].contiguous())
        one.bind_source(("plant", ac.NI), S[b:b + 1].contiguous())
    elif s.streams == "lti":
        one.bind_lti("plant", torch.as_tensor(s.A[b:b + 1], device="cuda"), torch.as_tensor(s.Bm[b:b + 1], device="cuda"))
    dev = lambda a: torch.as_tensor(a[b:b + 1], device="cuda")
    dq, dh = one.given_jvp(dev(s.d))
    gg = one.given_vjp(dev(s.gq), dev(s.gh))
    return dq.cpu().numpy()[0], dh.cpu().numpy()[0], gg.cpu().numpy()[0]


@pytest.mark.parametrize("name", ["mix-shared", "mix-bound", "mix-lti"])
def test_an_instance_does_not_depend_on_its_batch(gpu_api, torch_gpu, name):
    """Batch 5 against batch 1: instance b equals, bit for bit, the same instance run alone; two calls give the same
    bits."""
    torch = torch_gpu
    from mpcasm import engine

    s = setup(name)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    dq, dh = s.asm.given_jvp(dev(s.d))
    gg = s.asm.given_vjp(dev(s.gq), dev(s.gh))
    assert same(dq.cpu().numpy(), s.dq) and same(dh.cpu().numpy(), s.dh) and same(gg.cpu().numpy(), s.gg)
    for b in (0, 3):
        dq1, dh1, gg1 = _alone(torch, s, b, engine)
        assert same(dq1, s.dq[b]) and same(dh1, s.dh[b]) and same(gg1, s.gg[b]), b
    assert not same(s.dq[0], s.dq[3]) and not same(s.gg[0], s.gg[3])


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
    grid = cus * one.adjoint_info().per_cu
    n = grid + 3
    asm = engine.Assembler(form, batch=n)
    assert asm.adjoint_info().per_cu * cus == grid
    gen = torch.Generator(device="cuda").manual_seed(3)
    f = dict(dtype=torch.float64, device="cuda", generator=gen)
    asm.params.mul_(0.5 + torch.rand(asm.params.shape, **f))
    d, gq, gh = torch.randn((n, asm.ng), **f), torch.randn((n, asm.no), **f), torch.randn((n, asm.nc), **f)
    dq, dh = (t.clone() for t in asm.given_jvp(d))
    gg = asm.given_vjp(gq, gh).clone()
    again = asm.given_jvp(d) + (asm.given_vjp(gq, gh),)
    for a, c in zip((dq, dh, gg), again):
        assert torch.equal(a.view(torch.int64), c.view(torch.int64))
    for b in (0, grid - 1, grid, n - 1):
        one.params.copy_(asm.params[b:b + 1])
        dq1, dh1 = one.given_jvp(d[b:b + 1])
        gg1 = one.given_vjp(gq[b:b + 1], gh[b:b + 1])
        for a, c in ((dq[b], dq1[0]), (dh[b], dh1[0]), (gg[b], gg1[0])):
            assert torch.equal(a.view(torch.int64), c.view(torch.int64)), b
    assert not torch.equal(asm.params[0], asm.params[grid])
    assert bool(dh.abs().sum(dim=1).min() > 0) and bool(gg.abs().sum(dim=1).min() > 0)


def _padded(torch, rows, width):
    whole = torch.full((rows + PAD, width), float("nan"), dtype=torch.float64, device="cuda")
    whole[:rows] = KEEP
    return whole


def test_nothing_outside_the_result_is_written(gpu_api, torch_gpu):
    """Outputs in padded buffers with a sentinel: a call on ``count`` instances writes their rows and nothing else;
    a skipped half is not touched; ``count == 0`` and ``ng == 0`` write nothing; both halves None is refused."""
    torch = torch_gpu
    from mpcasm import engine, problems

    s = setup("mix-shared")
    asm, (ng, no, nc) = s.asm, (s.plan.ng, s.plan.no, s.plan.nc)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    count = 3
    kept = lambda t, first: bool((t[first:B] == KEEP).all()) and bool(torch.isnan(t[B:]).all())
    dq, dh, gg = _padded(torch, B, no), _padded(torch, B, nc), _padded(torch, B, ng)
    asm.given_jvp(dev(s.d), out=(dq, dh), count=count)
    asm.given_vjp(dev(s.gq), dev(s.gh), out=gg, count=count)
    for t, ref in ((dq, s.dq), (dh, s.dh), (gg, s.gg)):
        assert same(t[:count].cpu().numpy(), ref[:count]) and kept(t, count)
    # a skipped output stays as it was, the other half is the full call's
    dq, dh = _padded(torch, B, no), _padded(torch, B, nc)
    asm.given_jvp(dev(s.d), out=(dq, None))
    asm.given_jvp(dev(s.d), out=(None, dh))
    assert same(dq[:B].cpu().numpy(), s.dq) and same(dh[:B].cpu().numpy(), s.dh) and kept(dq, B) and kept(dh, B)
    # count == 0
    dq, dh, gg = _padded(torch, B, no), _padded(torch, B, nc), _padded(torch, B, ng)
    asm.given_jvp(dev(s.d), out=(dq, dh), count=0)
    asm.given_vjp(dev(s.gq), dev(s.gh), out=gg, count=0)
    assert kept(dq, 0) and kept(dh, 0) and kept(gg, 0)
    with pytest.raises(ValueError):
        asm.given_jvp(dev(s.d), out=(None, None))
    with pytest.raises(ValueError):
        asm.given_vjp(None, None)
    lib, (ptrs, strides) = capi.load(), asm._src_args()
    none = lib.mpcasm_assemble_vjp(asm._handle, ptrs, strides, asm.params.data_ptr(), None, None, gg.data_ptr(),
                                   asm._workspace().data_ptr(), B, None)
    assert none == capi.ERR_ARG and kept(gg, 0)
    # ng == 0: MPCASM_OK, nothing written
    rng = np.random.default_rng(23)
    nog = engine.Assembler(ac.build_no_given(problems.load_api("mpc_interface"), rng), batch=B)
    assert nog.ng == 0
    dq, dh = _padded(torch, B, nog.no), _padded(torch, B, nog.nc)
    nog.given_jvp(None, out=(dq, dh))
    torch.cuda.synchronize()
    assert kept(dq, 0) and kept(dh, 0)
    assert tuple(nog.given_vjp(dev(rng.normal(size=(B, nog.no))), None).shape) == (B, 0)


def test_a_plan_compiled_as_ltv_is_refused(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine, problems

    api = problems.load_api("mpc_interface")
    swp = engine.Assembler(problems.lipm_ltv(api, N=12), batch=2, ltv=["LIP"])
    with pytest.raises(capi.MpcasmError):
        swp.given_jvp(torch.zeros((2, swp.ng), dtype=torch.float64, device="cuda"))
    with pytest.raises(capi.MpcasmError):
        swp.given_vjp(torch.zeros((2, swp.no), dtype=torch.float64, device="cuda"), None)
    with pytest.raises(capi.MpcasmError):
        swp.adjoint_info()


def _biped_loop(torch, engine, problems):
    api = problems.load_api("mpc_interface")
    form = problems.biped(api, problems.BipedConfig(step_samples=8), reduced=True)
    form.update(step_times=np.array([6, 14]), step_count=0)
    asm = engine.Assembler(form, batch=B)
    rng = np.random.default_rng(29)
    given = rng.normal(0, 0.01, (B, asm.ng))
    for key in asm.plan.param_slots:   # instance 2 cannot be solved: every facet of every box asks for less than -1e3
        if key[0] == "limit" and key[2] == "extreme":
            asm.params[2, asm.param_slice(*key)[0]] = -1e3
    c, d = rng.normal(size=(B, asm.no)), rng.normal(size=(B, asm.nc))
    dev = lambda a: torch.as_tensor(a, device="cuda")
    return asm, dev(given), dev(c), dev(d)


def test_the_layer(gpu_api, torch_gpu):
    """mpc_solve_diff on the reduced biped at batch 5: given.grad equals, bit for bit, given_vjp(-u, w) of a direct
    qp_sensitivity call on the same polished solution; the instance that does not solve gets an exactly zero row;
    tangent equals qp_jvp fed with given_jvp's outputs, bit for bit."""
    torch = torch_gpu
    from mpcasm import diff, engine, problems

    asm, given, c, d = _biped_loop(torch, engine, problems)
    given.requires_grad_(True)
    res = diff.mpc_solve_diff(asm, given)
    assert res.verdict is None and res.x.requires_grad
    ((c * res.x).sum() + (d * res.y).sum()).backward()
    o = res._outcome
    s = engine.qp_sensitivity(o.P, o.G, o.h, res.sol, c, d, status=res.sol.status)
    assert torch.equal(res.verdict, s.verdict)
    verdict, status = s.verdict.tolist(), res.sol.status.tolist()
    assert status[2] != capi.QP_SOLVED and verdict[2] != capi.SENS_DONE
    assert verdict.count(capi.SENS_DONE) >= 3, verdict
    direct = asm.given_vjp(-s.u, s.w)
    assert torch.equal(given.grad.view(torch.int64), direct.view(torch.int64))
    assert not bool(given.grad[2].any())
    for b in range(B):
        if verdict[b] == capi.SENS_DONE:
            assert bool(given.grad[b].any()), b
    # the tangential predictor
    dg = torch.as_tensor(np.random.default_rng(31).normal(0, 1e-3, tuple(given.shape)), device="cuda")
    dx, dy = diff.tangent(asm, res, dg)
    dq, dh = asm.given_jvp(dg)
    j = engine.qp_jvp(o.P, o.G, o.h, res.sol, dq, dh, status=res.sol.status)
    assert torch.equal(dx.view(torch.int64), j.dx.view(torch.int64))
    assert torch.equal(dy.view(torch.int64), j.dy.view(torch.int64))
    assert not bool(dx[2].any()) and bool(dx[0].any())
    for kw in (dict(soft=(1.0, 0.0)), dict(polish=True)):
        with pytest.raises(ValueError):
            diff.mpc_solve_diff(asm, given.detach(), **kw)


def test_repeated_calls_do_not_grow_device_memory(gpu_api, torch_gpu):
    """The autograd node holds the outcome, never the returned object: nothing of a call outlives it."""
    import gc

    torch = torch_gpu
    from mpcasm import diff, engine, problems

    asm, given, c, d = _biped_loop(torch, engine, problems)

    def call():
        g = given.detach().clone().requires_grad_(True)
        res = diff.mpc_solve_diff(asm, g)
        ((c * res.x).sum() + (d * res.y).sum()).backward()
        diff.tangent(asm, res, g.detach())

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
