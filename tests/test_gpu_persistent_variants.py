"""GPU: every variant of the persistent kernel (csrc/resident.hip) against extended precision.  The family of
persistent_cases.py spans what a plan can select inside the kernel (test_persistent_variants_cpu.py holds it to
that); here every case runs on four builds -- the ahead-of-time kernel and the kernel compiled for the plan, P
written straight to memory and through LDS -- with every instance its own plant(s) (A, B), its own given and its
own weights, aims, arrows, centres and extremes; the plans compiled without ``lti=`` read the fill kernel's S, U of
those plants.  Each test asserts the variant and the kernel that ran, assembles 67 instances into NaN-filled
buffers and holds P, q, G, h of instances 0, 33 and 66 element by element to |x - x*| <= kappa (u M + 2^-1022)
(helpers.py; kappa: persistent_cases.kappa_of), x* the oracle in long double on the very fp64 inputs.  Then the
walk: on a grid of 3 workgroups (runs of four instances, more than twenty a workgroup, a tail of three) and of 5
(runs of one) every instance must come out bit for bit as on the full grid -- an instance is assembled by one
workgroup alone, whatever it assembled before.  Flagged cases launch one half at a time (the wanted half bit for
bit, the other buffers untouched), a part of the batch through an index into a longer ``given``, and the per-plan
kernel with its first fetch by arithmetic for none and for some of the chunks."""
import contextlib

import numpy as np
import pytest

import persistent_cases as pc
import sweep_cases as sc
from helpers import assert_componentwise

pytestmark = pytest.mark.gpu

BATCH = pc.BATCH
COUNT = 41                                             # instances of the launch through an index
# MPCASM_OPT_JIT (2 ahead of time, 1 per plan), MPCASM_OPT_P_DIRECT (1 straight to memory, 2 through LDS)
BUILDS = {"aot-direct": (2, 1), "aot-lds": (2, 2), "per-plan-direct": (1, 1), "per-plan-lds": (1, 2)}
KERNEL = {2: "resident_assemble_kernel", 1: "resident_spec_kernel"}
# by the formulation (persistent_cases.seed_of): the inputs, and the long-double references of the sampled
# instances -- the four builds of a case, and its lti, -mem, CSC and compact plans, share them
_INPUTS, _REFERENCES = {}, {}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@contextlib.contextmanager
def _build(jit, direct, fetch_runs=None):
    """The process-wide options a plan reads when it is created, set and put back."""
    from mpcasm import capi

    lib = capi.load()
    assert lib.mpcasm_set_option(capi.OPT_PATH, 0) == 0
    assert lib.mpcasm_set_option(capi.OPT_JIT, jit) == 0
    assert lib.mpcasm_set_option(capi.OPT_P_DIRECT, direct) == 0
    if fetch_runs is not None:
        assert lib.mpcasm_set_option(capi.OPT_JIT_FETCH_RUNS, fetch_runs) == 0
    try:
        yield
    finally:
        lib.mpcasm_set_option(capi.OPT_JIT, 0)
        lib.mpcasm_set_option(capi.OPT_P_DIRECT, 0)
        lib.mpcasm_set_option(capi.OPT_JIT_FETCH_RUNS, 8)


def _nan_out(torch, asm):
    f = dict(dtype=torch.float64, device="cuda")
    n, no, nc = asm.batch, asm.no, asm.nc
    pshape = (n, asm.csc["pnnz"]) if asm.csc else (n, no, no)
    gshape = (n, asm.csc["gnnz"]) if asm.csc else (n, nc, no)
    return tuple(torch.full(s, float("nan"), **f) for s in (pshape, (n, no), gshape, (n, nc)))


def _inputs(api, case):
    key = (case.make, case.stride0)
    if key not in _INPUTS:
        _, plants, form, given = pc.inputs(api, case, BATCH, given_rows=3)
        if case.stride0:        # one plant for the batch
            plants = {name: (np.broadcast_to(A[:1], A.shape), np.broadcast_to(B[:1], B.shape))
                      for name, (A, B) in plants.items()}
        _INPUTS[key] = (plants, form, given)
    return _INPUTS[key]


def _assembler(torch, case, plants, form):
    """The assembler of ``case`` with its systems bound -- (A, B) where the plan generates the horizon tables, the
    fill kernel's S, U where it fetches them -- and every instance its own parameters."""
    from mpcasm import engine

    asm = engine.Assembler(form, batch=BATCH, **case.kw)
    for name, n, m in case.systems:
        A, B = plants[name]
        if case.stride0:
            A, B = A[:1], B[:1]
        At, Bt = (torch.as_tensor(np.array(x), device="cuda") for x in (A, B))
        if "lti" in case.kw:
            asm.bind_lti(name, At[0] if case.stride0 else At, Bt[0] if case.stride0 else Bt)
        else:
            S, U = engine.fill_su(At, Bt, case.N)
            for j in range(m):
                asm.bind_source((name, j), U[0, j] if case.stride0 else U[:, j])
            asm.bind_source((name, m), S[0] if case.stride0 else S)
    params = pc.params_of(asm.plan, case, BATCH)
    asm.params.copy_(torch.as_tensor(params, device="cuda"))
    return asm, params


def _same(torch, mine, theirs, what):
    for key, a, b in zip("PqGh", mine, theirs):
        assert torch.equal(a, b), "%s: %s differs in instances %s" % (
            what, key, torch.nonzero((a != b).reshape(a.shape[0], -1).any(dim=1)).ravel().tolist()[:8])


CASE_BUILDS = [(c, b) for c in pc.CASES for b in BUILDS]


@pytest.mark.parametrize("case,build", CASE_BUILDS, ids=["%s-%s" % (c.name, b) for c, b in CASE_BUILDS])
def test_variant(gpu_api, torch_gpu, case, build):
    torch = torch_gpu
    from mpcasm import capi

    jit, direct = BUILDS[build]
    if direct == 2 and not case.p_in_lds:
        pytest.skip("P does not fit in LDS beside the workspace (pinned by test_persistent_variants_cpu.py)")
    plants, form, given = _inputs(gpu_api, case)
    with _build(jit, direct):
        asm, params = _assembler(torch, case, plants, form)
        assert asm.plan.resident["ok"]
        assert pc.variant_of(asm.plan) == case.variant
        g = torch.as_tensor(given[:BATCH], device="cuda")
        full = _nan_out(torch, asm)
        asm.assemble(g, out=full)
        assert asm.last_kernel().startswith(KERNEL[jit]), asm.last_kernel()
        assert not any(bool(torch.isnan(t).any()) for t in full), "an element was not written"
        # ---- P, q, G, h of the sampled instances, element by element
        res = {key: t.cpu().numpy() for key, t in zip("PqGh", full)}
        kap, worst = pc.kappa_of(case), 0.0
        refs = _REFERENCES.setdefault((case.make, case.stride0), {})
        with sc.instance_params(form, asm.plan) as objects:
            for b in case.sample:
                if b not in refs:
                    objects.set(params[b])
                    refs[b] = (params[b].copy(), pc.reference(form, case, plants, b, given[b]))
                assert np.array_equal(refs[b][0], params[b])      # (the plans of one formulation: the same slots)
                ref = pc.csc_reference(refs[b][1], asm.csc) if asm.csc else refs[b][1]
                for key, x in res.items():
                    worst = max(worst, assert_componentwise(x[b], *ref[key], kap,
                                                            "%s, instance %d, %s" % (case.name, b, key)))
        # ---- the walk: 3 workgroups (runs of four, a tail of three), 5 (runs of one): the same bits
        for grid in (3, 5):
            asm.set_option(capi.OPT_RESIDENT_GRID, grid)
            out = _nan_out(torch, asm)
            asm.assemble(g, out=out)
            assert asm.last_kernel().startswith(KERNEL[jit]), asm.last_kernel()
            _same(torch, out, full, "grid %d" % grid)
        asm.set_option(capi.OPT_RESIDENT_GRID, -1)
        if case.halves:
            # one half at a time, into fresh NaN buffers: the wanted half bit for bit, the other one untouched
            for want in (dict(want_constraints=False), dict(want_cost=False)):
                out = _nan_out(torch, asm)
                asm.assemble(g, out=out, **want)
                assert asm.last_kernel().startswith(KERNEL[jit]), asm.last_kernel()
                cost_half = "want_constraints" in want
                for i, (mine, theirs) in enumerate(zip(out, full)):
                    if (i < 2) == cost_half:
                        assert torch.equal(mine, theirs), "%s %s" % ("PqGh"[i], want)
                    else:
                        assert bool(torch.isnan(mine).all()), "%s written with %s" % ("PqGh"[i], want)
        if case.count_index:
            # the first COUNT instances, their rows of given picked through an index into 3 BATCH rows: bit for bit
            # what the gathered rows yield, the instances behind them untouched
            index = np.random.default_rng(pc.seed_of(case) + 2).permutation(3 * BATCH)[:BATCH].astype(np.int32)
            gathered = _nan_out(torch, asm)
            asm.assemble(torch.as_tensor(given[index], device="cuda"), out=gathered, count=COUNT)
            out = _nan_out(torch, asm)
            asm.assemble(torch.as_tensor(given, device="cuda"), out=out, count=COUNT,
                         index=torch.as_tensor(index, device="cuda"))
            assert asm.last_kernel().startswith(KERNEL[jit]), asm.last_kernel()
            for key, mine, theirs in zip("PqGh", out, gathered):
                assert not bool(torch.isnan(mine[:COUNT]).any()), key
                assert torch.equal(mine[:COUNT], theirs[:COUNT]), "%s through the index" % key
                assert bool(torch.isnan(mine[COUNT:]).all()) and bool(torch.isnan(theirs[COUNT:]).all()), \
                    "%s written behind instance %d" % (key, COUNT)
    if case.fetch_runs and build == "per-plan-direct":
        # the per-plan kernel's first fetch: no chunk by arithmetic, and chunks of both kinds -- builds of their own
        from test_fetch_segments_cpu import fetch_segments

        limit = pc.fetch_limit(asm.plan, fetch_segments)
        for runs in (0, limit):
            with _build(jit, direct, fetch_runs=runs):
                other, _ = _assembler(torch, case, plants, form)
                out = _nan_out(torch, other)
                other.assemble(g, out=out)
                assert other.last_kernel().startswith(KERNEL[jit]), other.last_kernel()
                _same(torch, out, full, "at most %d runs a chunk" % runs)
    v = case.variant
    what = "persistent %s JC %d %s mode %d %s" % (build, v.jc_inst, "gen" if v.gen else "mem", v.g_mode, case.name)
    print("componentwise %-60s worst %8.3g u M   kappa %d" % (what, worst, kap))
