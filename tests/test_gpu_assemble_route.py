"""GPU: the launch agrees with the route.  mpcasm_assemble decides its kernel family with the function
mpcasm_assemble_route reports (csrc/dispatch.hip assemble_route; the table of tests/test_assemble_route_cpu.py),
under the options of ITS plan -- set on the plan or process-wide, from one thread or from two."""
import threading

import numpy as np
import pytest

import sweep_cases as sc
import tiled_cases as tc
from mpcasm import problems

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _biped(api):
    form = problems.biped(api, problems.BipedConfig(step_samples=8))
    form.update(step_times=np.array([6, 14]), step_count=0)
    return form


def _biped_case(api, torch):
    from mpcasm import engine

    form = _biped(api)
    given = torch.as_tensor(np.random.default_rng(5).normal(0, 0.1, [67, form.given_len]), device="cuda")
    return (lambda: engine.Assembler(form, batch=67)), given


def _lipm3d_case(api, torch):
    from mpcasm import engine

    form = problems.lipm3d(api, N=32)
    given = torch.as_tensor(np.random.default_rng(6).normal(0, 0.1, [40, form.given_len]), device="cuda")
    return (lambda: engine.Assembler(form, batch=40, lti=["LIP"])), given


def _tiled_case(api, torch):
    from mpcasm import engine

    case = tc.BY_NAME["fused-4-4-32"]          # (128 unknowns, the fewest the tiled path takes)
    assert case.shape.m * case.shape.N == min(c.shape.m * c.shape.N for c in tc.GPU_CASES)
    rng = np.random.default_rng(7)
    A, B = tc.plants(rng, case.batch, case.shape)
    form = tc.build(api, rng, case.shape, (A[0], B[0]))
    At, Bt = torch.as_tensor(A, device="cuda"), torch.as_tensor(B, device="cuda")

    def make():
        asm = engine.Assembler(form, batch=case.batch, lti=["plant"])
        asm.bind_lti("plant", At, Bt)
        return asm

    return make, torch.as_tensor(rng.normal(0, 0.3, [case.batch, form.given_len]), device="cuda")


def _sweep_case(api, torch):
    from mpcasm import engine

    case, batch = sc.BY_NAME["one-1-1-1"], 5     # (one unknown)
    rng = np.random.default_rng(8)
    A, B = sc.plants(rng, batch, case.shape)
    form = sc.build(api, rng, case.shape, plant=(A[0, 0], B[0, 0]))
    At, Bt = torch.as_tensor(A, device="cuda"), torch.as_tensor(B, device="cuda")

    def make():
        asm = engine.Assembler(form, batch=batch, ltv=["plant"])
        asm.bind_ltv("plant", At, Bt)
        return asm

    return make, torch.as_tensor(rng.normal(0, 0.3, [batch, form.given_len]), device="cuda")


# name -> (builder, MPCASM_OPT_PATH, the family the route is to name)
CASES = {
    "biped": (_biped_case, 0, "KERNEL_RESIDENT"),
    "lipm3d-32": (_lipm3d_case, 0, "KERNEL_RESIDENT"),
    "biped, path 1": (_biped_case, 1, "KERNEL_FUSED"),
    "biped, path 2": (_biped_case, 2, "KERNEL_STAGED"),
    "tiled": (_tiled_case, 0, "KERNEL_TILED"),
    "sweep": (_sweep_case, 0, "KERNEL_SWEEP"),
}


def _family(capi, asm):
    """The family of the kernel the latest launch of ``asm`` ran, in the route's terms."""
    k = capi.load().mpcasm_plan_last_kernel(asm._handle)
    return {capi.KERNEL_RESIDENT_JIT: capi.KERNEL_RESIDENT, capi.KERNEL_TILED_SCAN: capi.KERNEL_TILED,
            capi.KERNEL_TILED_SHARED: capi.KERNEL_TILED}.get(k, k)


def _run(torch, asm, given):
    out = tuple(t.clone() for t in asm.assemble(given) if t is not None)
    torch.cuda.synchronize()
    return out


def _same(torch, a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(CASES))
def test_the_launch_takes_the_route(gpu_api, torch_gpu, name):
    """One launch per way of setting the path -- on the plan, and process-wide on assemblers created before any
    option was set -- runs the family the route names and gives the same bits.  (The reference launch runs under
    the same path: the families agree to the last bit or two, not bit for bit -- on the 36-wide biped the fused
    kernel's P, q, h and all of the staged pipeline's differ from the persistent kernel's by at most 8.9e-16,
    profiles/assemble_routes.txt -- so equality across paths is no property of the kernels to pin here.)"""
    from mpcasm import capi, engine

    torch, lib = torch_gpu, capi.load()
    builder, path, family = CASES[name]
    family = getattr(capi, family)
    make, given = builder(gpu_api, torch)
    first, own, wide = make(), make(), make()             # (all three before any option is set)
    route = engine.assemble_route(first.plan, first.batch, path)
    assert route.kernel == family
    if name == "lipm3d-32":
        assert route.lds > 64 * 1024
    # the option on the plan
    own.set_option(capi.OPT_PATH, path)
    mine = _run(torch, own, given)
    assert _family(capi, own) == route.kernel, own.last_kernel()
    # ... and process-wide: the assemblers that were there before follow it, at their next launch
    try:
        capi.check(lib.mpcasm_set_option(capi.OPT_PATH, path), "mpcasm_set_option")
        theirs = _run(torch, wide, given)
        assert _family(capi, wide) == route.kernel, wide.last_kernel()
        ref = _run(torch, first, given)
        assert _family(capi, first) == route.kernel, first.last_kernel()
    finally:
        lib.mpcasm_set_option(capi.OPT_PATH, 0)
    assert _same(torch, mine, ref) and _same(torch, theirs, ref)
    # with the process-wide value back, the plan's own option still holds
    assert _same(torch, _run(torch, own, given), ref) and _family(capi, own) == route.kernel
    if path == 2:
        _rows_by_index_launch_nothing(torch, make(), given)


def _rows_by_index_launch_nothing(torch, asm, given):
    """mpcasm_assemble_indexed off the persistent kernel: MPCASM_ERR_LIMIT, as the route says, and no kernel ran."""
    from mpcasm import capi, engine

    lib = capi.load()
    asm.set_option(capi.OPT_PATH, 2)
    with pytest.raises(capi.MpcasmError) as refusal:
        engine.assemble_route(asm.plan, asm.batch, 2, indexed=True)
    assert refusal.value.status == capi.ERR_LIMIT
    f = dict(dtype=torch.float64, device="cuda")
    n, no, nc = asm.batch, asm.no, asm.nc
    out = tuple(torch.full(s, float("nan"), **f) for s in ((n, no, no), (n, no), (n, nc, no), (n, nc)))
    index = torch.arange(n, dtype=torch.int32, device="cuda")
    ptrs, strides = asm._src_args()
    rc = lib.mpcasm_assemble_indexed(asm._handle, ptrs, strides, asm.params.data_ptr(), given.data_ptr(),
                                     index.data_ptr(), *(t.data_ptr() for t in out), asm._workspace().data_ptr(), n,
                                     None)
    torch.cuda.synchronize()
    assert rc == capi.ERR_LIMIT
    assert lib.mpcasm_plan_last_kernel(asm._handle) == capi.KERNEL_NONE
    assert all(bool(torch.isnan(t).all()) for t in out)


def test_options_stay_with_the_plan_across_threads(gpu_api, torch_gpu):
    """Two host threads, a stream each, 20 launches each, on two assemblers of the same biped plan -- one with
    MPCASM_OPT_PATH 2 of its own, one with the default: every result bit-equal to the single-threaded one, each
    plan's last kernel its own."""
    from mpcasm import capi

    torch = torch_gpu
    make, given = _biped_case(gpu_api, torch)
    asms = {"staged": make(), "default": make()}
    asms["staged"].set_option(capi.OPT_PATH, 2)
    ref = {k: _run(torch, a, given) for k, a in asms.items()}
    names = {k: a.last_kernel() for k, a in asms.items()}
    assert names["staged"].startswith("staged") and "persistent" in names["default"], names
    errors = []

    def run(key):
        try:
            stream = torch.cuda.Stream()
            outs = tuple(torch.empty_like(t) for t in ref[key])
            for i in range(20):
                got = asms[key].assemble(given, out=outs, stream=stream)
                stream.synchronize()
                if not _same(torch, got, ref[key]):
                    errors.append("%s, launch %d: results differ" % (key, i))
        except Exception as exc:                       # (a failed launch: MpcasmError)
            errors.append(repr(exc))

    threads = [threading.Thread(target=run, args=(key,)) for key in asms]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
    assert {k: a.last_kernel() for k, a in asms.items()} == names
