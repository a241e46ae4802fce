"""The first instances of every workgroup of the persistent kernel (GPU).

A persistent workgroup sets itself up once -- fetch tables, compose program, structure tables,
the first (A, B) and the first input image -- and then walks its instances.  The order of that
set-up is what decides when the first instance starts, so the first and the second instance of
every workgroup are exactly the ones a mistake in it would spoil: a table read before it landed,
an image or an (A, B) composed before its load came back.  Here every one of them is compared
with the oracle, for launches of 1, 2, grid - 1, grid, grid + 1, 4096 and 4096 + 3 instances
(grid: the workgroups a full launch of this plan runs, as the stamped launch reports them) and one
of 16 grid + 3 (runs of four consecutive instances per workgroup), plus a seeded sample of the
later instances; on the kernel compiled for the plan and on the ahead-of-time one; for the C2
biped with per-instance (A, B) in its 36- and 34-wide phases, with the CSC hand-off, and with the
``given`` rows picked through an index.
"""
import numpy as np
import pytest

from helpers import RTOL_TIGHT, rel_err
from mpcasm import problems
from oracle import qp_oracle as orc

pytestmark = pytest.mark.gpu

BUILDS = {"per-plan": 1, "ahead-of-time": 2}          # MPCASM_OPT_JIT
PLANS = {"c2-36": ([6, 14], 36), "c2-34": ([7, 15], 34), "c2-36-csc": ([6, 14], 36),
         "c2-36-indexed": ([6, 14], 36)}
SAMPLE = 48                                            # later instances checked per launch
FLEET = 3                                              # rows of `given` per instance behind the index


def launch_grid(asm, given):
    """Workgroups of a launch of the whole batch: those that left their cycle stamps."""
    import torch
    from mpcasm import capi

    lib = capi.load()
    asm.assemble(given)
    assert lib.mpcasm_set_option(capi.OPT_PHASE_MASK, capi.PHASE_DEFAULT | capi.PHASE_STAMPS) == 0
    try:
        asm._work.zero_()
        asm.assemble(given)
        torch.cuda.synchronize()
    finally:
        lib.mpcasm_set_option(capi.OPT_PHASE_MASK, capi.PHASE_DEFAULT)
    raw = asm._work.view(torch.int64).cpu().numpy()
    rows = raw[:(raw.size // 64) * 64].reshape(-1, 64)
    # (per workgroup one row of phase sums and, behind those of all workgroups, one of set-up stations)
    return int((rows != 0).any(axis=1).sum()) // 2


def instances_to_check(batch, grid, rng):
    """First and second instance of every workgroup of a launch of ``batch`` instances (the kernel's
    instance_at: round robin, in runs of four from 16 instances per workgroup on), and a sample of the rest."""
    wgs = min(grid, batch)
    shift = 2 if batch >= 16 * wgs else 0
    first = set()
    for n in (0, 1):
        for w in range(wgs):
            b = (((n >> shift) * wgs + w) << shift) + (n & ((1 << shift) - 1))
            if b < batch:
                first.add(b)
    rest = np.setdiff1d(np.arange(batch), np.fromiter(first, dtype=np.int64, count=len(first)))
    if rest.size > SAMPLE:
        rest = rng.choice(rest, SAMPLE, replace=False)
    return sorted(first), sorted(int(b) for b in rest)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("plan", list(PLANS))
def test_first_instances_of_every_workgroup(gpu_api, plan, build):
    import torch
    from mpcasm import capi, engine

    times, width = PLANS[plan]
    conf = problems.BipedConfig(step_samples=8)
    form = problems.biped(gpu_api, conf)
    form.update(step_times=np.array(times), step_count=0)
    assert form.optim_len == width
    no, N = form.optim_len, conf.horizon_lenght
    csc, indexed = plan.endswith("csc"), plan.endswith("indexed")
    lib = capi.load()
    assert lib.mpcasm_set_option(capi.OPT_PATH, 0) == 0
    assert lib.mpcasm_set_option(capi.OPT_JIT, BUILDS[build]) == 0
    lip = form.dynamics["LIP"]
    keep = list(lip.matrices)
    try:
        rng = np.random.default_rng(width + 100 * csc + 1000 * indexed)
        probe = engine.Assembler(form, batch=4096, lti=["LIP"])
        grid = launch_grid(probe, rng.normal(0, 0.1, [4096, form.given_len]))
        assert "persistent" in probe.last_kernel(), probe.last_kernel()
        assert 2 <= grid <= 4096, grid
        del probe
        batches = [1, 2, grid - 1, grid, grid + 1, 4096, 4096 + 3, 16 * grid + 3]
        cap = max(batches)
        asm = engine.Assembler(form, batch=cap, lti=["LIP"], **(dict(csc="upper") if csc else {}))
        nc = asm.nc
        get_A, get_B, _ = gpu_api.tools.get_system_matrices("J->CCC")
        taus = rng.uniform(0.08, 0.12, cap)
        A = np.stack([get_A(tau=t) for t in taus])
        B = np.stack([get_B(tau=t) for t in taus])
        asm.bind_lti("LIP", A, B)
        given = rng.normal(0, 0.1, [cap * (FLEET if indexed else 1), form.given_len])
        index = rng.integers(0, given.shape[0], cap).astype(np.int32) if indexed else np.arange(cap, dtype=np.int32)
        index_dev = torch.as_tensor(index, device="cuda")
        given_dev = torch.as_tensor(given, device="cuda")
        pshape = (cap, asm.csc["pnnz"]) if csc else (cap, no, no)
        gshape = (cap, asm.csc["gnnz"]) if csc else (cap, nc, no)
        out = tuple(torch.empty(s, dtype=torch.float64, device="cuda") for s in (pshape, (cap, no), gshape, (cap, nc)))

        reference = {}

        def oracle(b):
            if b not in reference:
                Sb, Ub = orc.extend_matrices(N, A[b], B[b])
                lip.matrices = Ub + [Sb]
                lip.update_definitions()
                Ao, ho, Qo, qo = orc.assemble(form, given[index[b]].reshape(-1, 1))
                if csc:
                    Qo, Ao = Qo.reshape(-1)[asm.csc["p_flat"]], Ao.reshape(-1)[asm.csc["g_flat"]]
                reference[b] = (np.array(Qo), qo.ravel().copy(), np.array(Ao), ho.ravel().copy())
            return reference[b]

        worst = 0.0
        for batch in batches:
            for t in out:
                t.fill_(float("nan"))
            res = asm.assemble(given_dev, out=out, count=batch, index=index_dev if indexed else None)
            assert "persistent" in asm.last_kernel(), asm.last_kernel()
            P, q, G, h = (t[:batch].cpu().numpy() for t in res)
            assert not any(np.isnan(t).any() for t in (P, q, G, h)), "batch %d: an instance was not written" % batch
            first, rest = instances_to_check(batch, grid, rng)
            for b in first + rest:
                for name, mine, ref in zip("PqGh", (P[b], q[b], G[b], h[b]), oracle(b)):
                    err = rel_err(mine, ref)
                    worst = max(worst, err)
                    assert err <= RTOL_TIGHT, "%s of instance %d of %d (grid %d, %s, %s): %.3e" % (
                        name, b, batch, grid, plan, build, err)
        print("%s, %s: grid %d, %d instances compared, worst relative error %.3e"
              % (plan, build, grid, len(reference), worst))
    finally:
        lip.matrices = keep
        lip.update_definitions()
        lib.mpcasm_set_option(capi.OPT_PATH, 0)
        lib.mpcasm_set_option(capi.OPT_JIT, 0)
