"""The first requests of a persistent workgroup, asked for by arithmetic (GPU).

The kernel compiled for one plan works the addresses of its first requests -- the (A, B) of a
workgroup's first two instances, its whole first image -- out from the lane index and the runs
of the fetch tables (``jit.hip jit_fetch_segments``) instead of reading the tables first.  A wrong
run, a wrong stream or a wrong stride spoils exactly the first instances of a workgroup (later
ones are fetched through the tables' LDS copies, which the same runs write), so the first two
instances of every workgroup and the last instance of the batch are compared with the oracle, at
the tolerances of ``test_gpu_prologue.py``, on the per-plan and on the ahead-of-time kernel, for

(a) a launch of 4096 instances,
(b) launches smaller than the grid, and of one and a half grids: half the workgroups have a single
    instance, and no second (A, B) to ask for,
(c) ``assemble(index=...)`` with a permutation of the rows of ``given``,
(d) an (A, B) shared by the whole batch (a stream of stride 0),
(e) a plan with some chunks fetched by arithmetic and some through the table in ONE kernel: the
    reference's test_body problem, whose chunks have at most 4 runs, compiled with a limit of 3 runs
    per chunk (``MPCASM_OPT_JIT_FETCH_RUNS``; ``test_fetch_segments_cpu.py`` checks that this leaves both
    kinds and that the kernel compiles).

Every launch must have run the kernel its parametrisation names (``last_kernel()``).
"""
import numpy as np
import pytest

from helpers import RTOL_TIGHT, rel_err
from mpcasm import problems
from oracle import qp_oracle as orc
from test_gpu_prologue import launch_grid

pytestmark = pytest.mark.gpu

BUILDS = {"per-plan": 1, "ahead-of-time": 2}          # MPCASM_OPT_JIT
# ... and what `last_kernel()` must say then: a per-plan build that failed to compile falls back to the
# ahead-of-time kernel, which would pass these tests without running one line of the code they are for
RAN = {"per-plan": "resident_spec_kernel", "ahead-of-time": "resident_assemble_kernel"}
CASES = ["per-instance", "indexed", "shared"]


def instances_to_check(batch, grid):
    """First and second instance of every workgroup (the kernel's instance_at) and the batch's last."""
    wgs = min(grid, batch)
    shift = 2 if batch >= 16 * wgs else 0
    picked = {batch - 1}
    for n in (0, 1):
        for w in range(wgs):
            b = (((n >> shift) * wgs + w) << shift) + (n & ((1 << shift) - 1))
            if b < batch:
                picked.add(b)
    return sorted(picked)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("case", CASES)
def test_first_instances_c2(gpu_api, case, build):
    import torch
    from mpcasm import capi, engine

    conf = problems.BipedConfig(step_samples=8)
    form = problems.biped(gpu_api, conf)
    form.update(step_times=np.array([6, 14]), step_count=0)
    no, N = form.optim_len, conf.horizon_lenght
    lib = capi.load()
    assert lib.mpcasm_set_option(capi.OPT_PATH, 0) == 0
    assert lib.mpcasm_set_option(capi.OPT_JIT, BUILDS[build]) == 0
    lip = form.dynamics["LIP"]
    keep = list(lip.matrices)
    try:
        rng = np.random.default_rng(CASES.index(case))
        cap = 4096
        asm = engine.Assembler(form, batch=cap, lti=["LIP"])
        grid = launch_grid(asm, rng.normal(0, 0.1, [cap, form.given_len]))
        assert asm.last_kernel().startswith(RAN[build]), asm.last_kernel()
        assert 4 <= grid <= cap, grid
        nc = asm.nc
        get_A, get_B, _ = gpu_api.tools.get_system_matrices("J->CCC")
        shared = case == "shared"
        taus = np.full(cap, 0.1) if shared else rng.uniform(0.08, 0.12, cap)
        A = np.stack([get_A(tau=t) for t in taus])
        B = np.stack([get_B(tau=t) for t in taus])
        if shared:
            asm.bind_lti("LIP", A[0], B[0])                     # one (n, n), (n, m) for all: stride 0
        else:
            asm.bind_lti("LIP", A, B)
        given = rng.normal(0, 0.1, [cap, form.given_len])
        index = rng.permutation(cap).astype(np.int32) if case == "indexed" else np.arange(cap, dtype=np.int32)
        index_dev = torch.as_tensor(index, device="cuda")
        given_dev = torch.as_tensor(given, device="cuda")
        out = tuple(torch.empty(s, dtype=torch.float64, device="cuda")
                    for s in ((cap, no, no), (cap, no), (cap, nc, no), (cap, nc)))
        reference = {}

        def oracle(b):
            if b not in reference:
                Sb, Ub = orc.extend_matrices(N, A[b], B[b])
                lip.matrices = Ub + [Sb]
                lip.update_definitions()
                Ao, ho, Qo, qo = orc.assemble(form, given[index[b]].reshape(-1, 1))
                reference[b] = (np.array(Qo), qo.ravel().copy(), np.array(Ao), ho.ravel().copy())
            return reference[b]

        worst = 0.0
        for batch in (cap, grid // 2, grid + grid // 2):
            for t in out:
                t.fill_(float("nan"))
            res = asm.assemble(given_dev, out=out, count=batch, index=index_dev if case == "indexed" else None)
            assert asm.last_kernel().startswith(RAN[build]), asm.last_kernel()
            P, q, G, h = (t[:batch].cpu().numpy() for t in res)
            assert not any(np.isnan(t).any() for t in (P, q, G, h)), "batch %d: an instance was not written" % batch
            for b in instances_to_check(batch, grid):
                for name, mine, ref in zip("PqGh", (P[b], q[b], G[b], h[b]), oracle(b)):
                    err = rel_err(mine, ref)
                    worst = max(worst, err)
                    assert err <= RTOL_TIGHT, "%s of instance %d of %d (grid %d, %s, %s): %.3e" % (
                        name, b, batch, grid, case, build, err)
        print("%s, %s: grid %d, %d instances compared, worst relative error %.3e"
              % (case, build, grid, len(reference), worst))
    finally:
        lip.matrices = keep
        lip.update_definitions()
        lib.mpcasm_set_option(capi.OPT_PATH, 0)
        lib.mpcasm_set_option(capi.OPT_JIT, 0)


@pytest.mark.parametrize("build", list(BUILDS))
def test_first_instances_with_chunks_of_both_kinds(gpu_api, build):
    import torch
    from mpcasm import capi, engine

    form = problems.body_case(gpu_api)
    lib = capi.load()
    # (the limit is part of the generated constants, so this kernel is a build of its own)
    assert lib.mpcasm_set_option(capi.OPT_JIT_FETCH_RUNS, 3) == 0
    assert lib.mpcasm_set_option(capi.OPT_PATH, 0) == 0
    assert lib.mpcasm_set_option(capi.OPT_JIT, BUILDS[build]) == 0
    try:
        rng = np.random.default_rng(5)
        cap = 4096
        asm = engine.Assembler(form, batch=cap)
        given = rng.normal(0, 0.5, [cap, form.given_len])
        grid = launch_grid(asm, given)
        assert asm.last_kernel().startswith(RAN[build]), asm.last_kernel()
        assert 4 <= grid <= cap, grid
        given_dev = torch.as_tensor(given, device="cuda")
        no, nc = asm.no, asm.nc
        out = tuple(torch.empty(s, dtype=torch.float64, device="cuda")
                    for s in ((cap, no, no), (cap, no), (cap, nc, no), (cap, nc)))
        reference = {}
        worst = 0.0
        for batch in (cap, grid // 2, grid + grid // 2):
            for t in out:
                t.fill_(float("nan"))
            res = asm.assemble(given_dev, out=out, count=batch)
            assert asm.last_kernel().startswith(RAN[build]), asm.last_kernel()
            P, q, G, h = (t[:batch].cpu().numpy() for t in res)
            assert not any(np.isnan(t).any() for t in (P, q, G, h)), "batch %d: an instance was not written" % batch
            for b in instances_to_check(batch, grid):
                if b not in reference:
                    Ao, ho, Qo, qo = orc.assemble(form, given[b].reshape(-1, 1))
                    reference[b] = (np.array(Qo), qo.ravel().copy(), np.array(Ao), ho.ravel().copy())
                for name, mine, ref in zip("PqGh", (P[b], q[b], G[b], h[b]), reference[b]):
                    err = rel_err(mine, ref)
                    worst = max(worst, err)
                    assert err <= RTOL_TIGHT, "%s of instance %d of %d (grid %d, %s): %.3e" % (
                        name, b, batch, grid, build, err)
        print("body_case, %s: grid %d, %d instances compared, worst relative error %.3e"
              % (build, grid, len(reference), worst))
    finally:
        lib.mpcasm_set_option(capi.OPT_JIT_FETCH_RUNS, 8)
        lib.mpcasm_set_option(capi.OPT_PATH, 0)
        lib.mpcasm_set_option(capi.OPT_JIT, 0)
