"""GPU: every variant of the rollout kernel (csrc/rollout.hip: ``ltv_rollout_kernel`` behind ``Assembler.rollout``,
``Assembler.advance`` and ``LtvLoop``) and every edge of its launch geometry against extended precision, beside
test_gpu_ltv_rollout.py, which runs the seven shapes at 3 instances:

  (a) the sixteen ``roll_chain<NS, MS>`` (rollout_cases.NM_SHAPES) in workgroups of 8 and 3, rows and advance;
  (b) the group sizes and tails of rollout_cases.GEOMETRY: full, partial and single workgroups behind full ones;
  (c) ``out`` and ``optim`` starting on an odd double (the peeled 8-byte store, the staging from inside a block);
  (d) instances whose device index points outside ``given``, beside ones that are there, aligned and 8 bytes off;
  (e) the advance over several workgroups under a status mask, and a plant shared by the batch (stride 0);
  (f) the closed loop at 20 instances, teacher-forced tick by tick.

Every launch writes into NaN-filled buffers, and every test first holds ``Assembler.rollout_info`` -- the function
the launch takes its geometry from -- to the workgroups its case claims.  The rows of EVERY instance below ``count``
stay within ``kappa_rollout(N, n, m) (u M + 2^-1022)`` of rollout_cases.reference_rows (long double, on the very
fp64 inputs); a next ``given`` within ``kappa_rollout(1, n, m)`` of first_step_reference: one step is one inner
product of length n + m.  The worst ratio per case is kept in profiles/rollout_variants.txt."""
import os
import types

import numpy as np
import pytest

import rollout_cases as rc
import sweep_cases as sc
from helpers import assert_componentwise

pytestmark = pytest.mark.gpu
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       "rollout_variants.txt")
HEAD = ("# ltv_rollout_kernel (csrc/rollout.hip), every variant: worst error in u M over every instance of a case\n"
        "# (u = 2^-53) and its bound -- kappa_rollout(N, n, m) for the rows, kappa_rollout(1, n, m) for the next given;\n"
        "# written by tests/test_gpu_ltv_rollout_variants.py\n")
KEY = 30
NAN = float("nan")


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def record(key, text):
    """One line per case in profiles/rollout_variants.txt (a checkout that cannot be written is left alone)."""
    print("rollout-variants: %-*s %s" % (KEY, key, text))
    try:
        lines = {}
        if os.path.exists(PROFILE):
            for line in open(PROFILE):
                if not line.startswith("#") and line.strip():
                    lines[line[:KEY].strip()] = line.rstrip("\n")
        lines[key] = "%-*s %s" % (KEY, key, text)
        with open(PROFILE, "w") as f:
            f.write(HEAD + "".join(lines[k] + "\n" for k in sorted(lines)))
    except OSError:
        pass


_CASES = {}


def case(api, torch, name, batch):
    """The inputs of ``batch`` instances of shape ``name`` -- every instance its own per-step plant, initial state and
    solution -- with their assembler, made once and never changed; ``ref(b)``: the long-double rows of instance b,
    computed once."""
    if (name, batch) in _CASES:
        return _CASES[(name, batch)]
    from mpcasm import engine

    shape = rc.shape_of(name)
    rng = np.random.default_rng([batch, 500] + [ord(ch) for ch in name])
    A, Bm = sc.plants(rng, batch, shape)
    form = sc.build(api, rng, shape, plant=(A[0, 0], Bm[0, 0]))
    dyn = sc.dynamics_name(shape)
    asm = engine.Assembler(form, batch=batch, ltv=[dyn])
    c = types.SimpleNamespace(name=name, shape=shape, batch=batch, form=form, dyn=dyn, asm=asm, plan=asm.plan, A=A,
                              B=Bm, pmrows=asm.plan.pmrows, rng=rng,
                              given=rng.normal(0, 0.3, [batch, asm.ng]), optim=rng.normal(0, 0.5, [batch, asm.no]),
                              kap=rc.kappa_rollout(shape.N, shape.n, shape.m),
                              kap1=rc.kappa_rollout(1, shape.n, shape.m))
    c.dA, c.dB = torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda")
    asm.bind_ltv(dyn, c.dA, c.dB)
    c.g, c.x = torch.as_tensor(c.given, device="cuda"), torch.as_tensor(c.optim, device="cuda")
    refs = {}

    def ref(b):
        if b not in refs:
            refs[b] = rc.reference_rows(form, dyn, A[b], Bm[b], c.given[b], c.optim[b], asm.plan)
        return refs[b]

    c.ref = ref
    _CASES[(name, batch)] = c
    return c


def split_of(asm, rows, count):
    """The live instances of every workgroup, from what the launch itself would choose."""
    group, _, workgroups = asm.rollout_info(rows=rows, count=count)
    split = tuple(min(group, count - first) for first in range(0, count, group))
    assert len(split) == workgroups
    return split


def nan_rows(torch, c, odd=False):
    """``(whole, out)``: a NaN-filled ``(batch, pmrows)`` buffer with a double in front and one behind; ``odd``:
    ``out`` starts on that first double (8 bytes off a 16-byte boundary), else two doubles in."""
    whole = torch.full((c.batch * c.pmrows + 4,), NAN, dtype=torch.float64, device="cuda")
    first = 1 if odd else 2
    out = whole[first:first + c.batch * c.pmrows].view(c.batch, c.pmrows)
    assert out.is_contiguous() and out.data_ptr() % 16 == (8 if odd else 0)
    return whole, out


def guards_kept(torch, whole, out, count):
    """Nothing in front of ``out``, behind it, or from row ``count`` on is written."""
    first = (out.data_ptr() - whole.data_ptr()) // 8
    used = first + count * out.shape[1]
    return bool(torch.isnan(whole[:first]).all()) and bool(torch.isnan(whole[used:]).all())


def rows_against_reference(c, rows, count, what):
    """Every instance below ``count`` within the bound, the copies of given and optim bit for bit; the worst u M."""
    from mpcasm import capi, engine

    assert rows.shape[0] == count
    worst = max(assert_componentwise(rows[b], *c.ref(b), c.kap, "%s, instance %d" % (what, b)) for b in range(count))
    copies = 0
    for kind, row0, n, axis, k0, kstep, cv, _ in engine.rollout_rows(c.plan)[0]:
        src = {capi.ROLL_GIVEN: c.given, capi.ROLL_OPTIM: c.optim}.get(int(kind))
        if src is not None:
            assert kstep == 1 or n == 1
            assert np.array_equal(rows[:, row0:row0 + n], src[:count, k0:k0 + n]), (what, kind, row0)
            copies += n
    assert copies == c.asm.ng + c.asm.no
    return worst


def run_rows(torch, c, count, odd=False, **kw):
    """One rollout of ``count`` instances into NaN: the rows below count on the host, guards checked."""
    whole, out = nan_rows(torch, c, odd)
    given = kw.pop("given", c.g)
    assert c.asm.rollout(given, kw.pop("optim", c.x), out=out, count=count, **kw) is out
    assert guards_kept(torch, whole, out, count), (c.name, count, "written outside the rows of the launch")
    return out[:count].clone()


# ---- (a) every instantiation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.NM_SHAPES)
def test_every_chain_instantiation(gpu_api, torch_gpu, name):
    """n, m in 1 .. 4, 11 instances: workgroups of 8 and 3 for the rows and for the advance."""
    torch = torch_gpu
    c = case(gpu_api, torch, name, rc.NM_BATCH)
    asm, count = c.asm, rc.NM_BATCH
    assert (c.plan.sweep["n"], c.plan.sweep["m"]) == (c.shape.n, c.shape.m)
    assert split_of(asm, True, count) == (8, 3) and split_of(asm, False, count) == (8, 3)
    rows = run_rows(torch, c, count).cpu().numpy()
    worst = rows_against_reference(c, rows, count, name)
    # the next given by a permuted index into 14 rows: every named row against x_1 in long double, the others kept
    big = torch.as_tensor(c.rng.normal(0, 1.0, [rc.NM_GIVEN_ROWS, asm.ng]), device="cuda")
    perm = np.random.default_rng(count).permutation(rc.NM_GIVEN_ROWS)[:count]
    big[torch.as_tensor(perm, device="cuda")] = c.g
    before = big.cpu().numpy()
    assert asm.advance(big, c.x, index=torch.as_tensor(perm.astype(np.int32), device="cuda"), count=count) is big
    after = big.cpu().numpy()
    others = np.setdiff1d(np.arange(rc.NM_GIVEN_ROWS), perm)
    assert others.size == 3 and np.array_equal(after[others], before[others])
    worst1 = 0.0
    for b in range(count):
        ref = rc.first_step_reference(c.plan, c.A[b, 0], c.B[b, 0], c.given[b], c.optim[b])
        worst1 = max(worst1, assert_componentwise(after[perm[b]], *ref, c.kap1, "%s, next given of %d" % (name, b)))
        # ... and it is the first sample of the states the rows hold, bit for bit
        assert np.array_equal(after[perm[b]], rc.next_given_reference(c.plan, (rows[b], rows[b]))[0]), (name, b)
    record("a %s" % name, "rows %6.3f of %3d   next given %6.3f of %2d" % (worst, c.kap, worst1, c.kap1))


# ---- (b) group sizes and tails -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch,counts", rc.GEOMETRY, ids=[g[0] for g in rc.GEOMETRY])
def test_group_sizes_and_tails(gpu_api, torch_gpu, name, batch, counts):
    torch = torch_gpu
    c = case(gpu_api, torch, name, batch)
    worst = 0.0
    for count, split in counts.items():
        assert split_of(c.asm, True, count) == split, (name, count)
        rows = run_rows(torch, c, count).cpu().numpy()
        worst = max(worst, rows_against_reference(c, rows, count, "%s, %d of %d" % (name, count, batch)))
    record("b %s" % name, "rows %6.3f of %4d   counts %s" % (worst, c.kap, " ".join(str(k) for k in counts)))


# ---- (c) out and optim on an odd double ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch,count", rc.ODD_START, ids=[g[0] for g in rc.ODD_START])
def test_out_and_optim_on_an_odd_double(gpu_api, torch_gpu, name, batch, count):
    torch = torch_gpu
    c = case(gpu_api, torch, name, batch)
    assert split_of(c.asm, True, count) == dict((g[0], g[2]) for g in rc.GEOMETRY)[name][count]
    aligned = run_rows(torch, c, count)
    assert not bool(torch.isnan(aligned).any())
    # out 8 bytes off (run_rows holds the doubles in front of it, behind it and from row count on to NaN)
    assert torch.equal(run_rows(torch, c, count, odd=True), aligned)
    # optim 8 bytes off: staged from the 16-byte boundary inside every block
    flat = torch.full((batch * c.asm.no + 2,), NAN, dtype=torch.float64, device="cuda")
    x = flat[1:1 + batch * c.asm.no].view(batch, c.asm.no)
    x.copy_(c.x)
    assert x.is_contiguous() and x.data_ptr() % 16 == 8 and c.x.data_ptr() % 16 == 0
    assert torch.equal(run_rows(torch, c, count, optim=x), aligned)
    assert torch.equal(run_rows(torch, c, count, odd=True, optim=x), aligned)
    # ... and read from there by the single step of the advance
    assert torch.equal(c.asm.advance(c.g.clone(), x, count=count), c.asm.advance(c.g.clone(), c.x, count=count))


# ---- (d) a row that is not there, beside ones that are -----------------------------------------------------------------
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd-double"])
def test_a_missing_row_beside_valid_neighbours(gpu_api, torch_gpu, odd):
    """lipm-33, 17 instances in workgroups of 8, 8, 1: the index of instance 8 (the second workgroup's first), of 9
    (inside it) and of 16 (the last, alone in its workgroup) points outside ``given``.  Their rows stay NaN; every
    other element is what the valid index gives -- with ``out`` on an odd double also those that share a 16-byte
    pair with a missing neighbour's (pmrows = 402 is even: aligned, no pair straddles two instances)."""
    torch = torch_gpu
    name, batch, count, given_rows, missing = rc.MISSING
    c = case(gpu_api, torch, name, batch)
    assert split_of(c.asm, True, count) == (8, 8, 1) and c.pmrows % 2 == 0
    big = torch.as_tensor(np.random.default_rng(61).normal(0, 1.0, [given_rows, c.asm.ng]), device="cuda")
    perm = np.random.default_rng(62).permutation(given_rows)[:count]
    big[torch.as_tensor(perm, device="cuda")] = c.g[:count]
    dev = lambda v: torch.as_tensor(np.asarray(v, dtype=np.int32), device="cuda")
    valid = run_rows(torch, c, count, odd=odd, given=big, index=dev(perm))
    assert torch.equal(valid, run_rows(torch, c, count))            # (the rows of the plain run, from the index)
    wild = perm.copy()
    wild[list(missing)] = [given_rows, -1, given_rows + 5]
    rows = run_rows(torch, c, count, odd=odd, given=big, index=dev(wild))
    there = np.setdiff1d(np.arange(count), missing)
    assert bool(torch.isnan(rows[list(missing)]).all())
    assert torch.equal(rows[there.tolist()], valid[there.tolist()])
    # the advance: the rows the valid entries name move as with the whole index, every other row keeps its bits
    full, part = big.clone(), big.clone()
    c.asm.advance(full, c.x, index=dev(perm), count=count)
    c.asm.advance(part, c.x, index=dev(wild), count=count)
    moved = torch.as_tensor(perm[there], device="cuda")
    kept = torch.as_tensor(np.setdiff1d(np.arange(given_rows), perm[there]), device="cuda")
    assert torch.equal(part[moved], full[moved]) and torch.equal(part[kept], big[kept])
    assert not torch.equal(full[kept], big[kept])                   # (the whole index does move three of them)


# ---- (e) the advance across workgroups -----------------------------------------------------------------------------
def test_the_advance_across_workgroups(gpu_api, torch_gpu):
    """lipm-33, a permuted index into 25 rows, 20 / 17 / 9 instances: every workgroup of more than one instance holds
    applied and held ones.  Which apply is worked out here from the mask's bits, not read back."""
    torch = torch_gpu
    from mpcasm import capi, engine

    name, batch, given_rows, counts = rc.ADVANCE
    c = case(gpu_api, torch, name, batch)
    asm = c.asm
    cycle = [capi.QP_SOLVED, capi.QP_MAX_ITER, capi.QP_PRIMAL_INFEASIBLE, capi.QP_NON_CVX, 40, -40]
    status = np.array([cycle[b % len(cycle)] for b in range(batch)], dtype=np.int32)
    dstatus = torch.as_tensor(status, device="cuda")
    big0 = torch.as_tensor(np.random.default_rng(71).normal(0, 1.0, [given_rows, asm.ng]), device="cuda")
    perm = np.random.default_rng(72).permutation(given_rows)[:batch]
    big0[torch.as_tensor(perm, device="cuda")] = c.g
    index = torch.as_tensor(perm.astype(np.int32), device="cuda")
    before = big0.cpu().numpy()
    refs = [rc.first_step_reference(c.plan, c.A[b, 0], c.B[b, 0], c.given[b], c.optim[b]) for b in range(batch)]
    worst = 0.0
    for count, split in counts.items():
        assert split_of(asm, False, count) == split
        for mask, stat in ((engine.APPLY_SOLVED, dstatus), (engine.APPLY_ALL, dstatus), (None, None)):
            if stat is None:
                applies = np.ones(count, dtype=bool)
            else:
                applies = np.array([abs(int(s)) <= 31 and bool((mask >> abs(int(s))) & 1) for s in status[:count]])
                first = 0
                for live in split:                      # (a workgroup of one instance cannot hold both kinds)
                    mine = applies[first:first + live]
                    assert live == 1 or (mine.any() and not mine.all()), (count, first)
                    first += live
            big = big0.clone()
            kw = {} if stat is None else dict(status=stat, apply_mask=mask)
            assert asm.advance(big, c.x, index=index, count=count, **kw) is big
            after = big.cpu().numpy()
            moved = perm[:count][applies]
            kept = np.setdiff1d(np.arange(given_rows), moved)
            assert np.array_equal(after[kept], before[kept]), (count, mask)
            for b in np.flatnonzero(applies):
                worst = max(worst, assert_componentwise(after[perm[b]], *refs[b], c.kap1,
                                                        "count %d, mask %r, instance %d" % (count, mask, b)))
                assert not np.array_equal(after[perm[b]], before[perm[b]])
    record("e advance lipm-33", "next given %6.3f of %2d   counts %s" % (worst, c.kap1, " ".join(map(str, counts))))

    # one plant shared by the batch (stride 0) against every instance's own copy of it, rows and advance, 20 instances
    try:
        own = np.broadcast_to(c.A[:1], c.A.shape).copy(), np.broadcast_to(c.B[:1], c.B.shape).copy()
        asm.bind_ltv(c.dyn, torch.as_tensor(own[0], device="cuda"), torch.as_tensor(own[1], device="cuda"))
        each, each_next = run_rows(torch, c, batch), asm.advance(big0.clone(), c.x, index=index)
        asm.bind_ltv(c.dyn, c.dA[0].contiguous(), c.dB[0].contiguous())
        ids = c.plan.ltv[0]["ids"]
        assert asm._src_stride[ids[0]] == 0 and asm._src_stride[ids[1]] == 0
        assert split_of(asm, True, batch) == (8, 8, 4) and split_of(asm, False, batch) == (8, 8, 4)
        assert torch.equal(run_rows(torch, c, batch), each)
        assert torch.equal(asm.advance(big0.clone(), c.x, index=index), each_next)
        assert not torch.equal(each_next, big0)
    finally:
        asm.bind_ltv(c.dyn, c.dA, c.dB)
    assert torch.equal(run_rows(torch, c, 1)[0], each[0])           # (instance 0 reads plant 0 either way)


# ---- (f) the loop over several workgroups, teacher-forced -----------------------------------------------------------
@pytest.mark.parametrize("on_unsolved", ["hold", "apply"])
def test_the_loop_tick_by_tick_over_three_workgroups(gpu_api, torch_gpu, on_unsolved):
    """test_gpu_ltv_loop.test_the_loop_tick_by_tick's check at 20 instances: rollout_cases.loop_inputs five times
    over, so the advance runs workgroups of 8, 8, 4 and each holds a primal infeasible instance (1, 5, 9, 13, 17)."""
    torch = torch_gpu
    from mpcasm.ltv_loop import LtvLoop

    reps = 5
    batch = reps * rc.LOOP_BATCH
    form, A, B, given0 = rc.loop_inputs(gpu_api)
    A, B, given0 = np.tile(A, (reps, 1, 1, 1)), np.tile(B, (reps, 1, 1, 1)), np.tile(given0, (reps, 1))
    loop = LtvLoop(form, "LIP", batch, torch.as_tensor(A, device="cuda"), torch.as_tensor(B, device="cuda"),
                   on_unsolved=on_unsolved)
    split = split_of(loop.asm, False, batch)
    assert split == (8, 8, 4)
    loop.given.copy_(torch.as_tensor(given0, device="cuda"))
    plan = loop.asm.plan
    kap1 = rc.kappa_rollout(1, 3, 1)
    group_of = np.repeat(np.arange(len(split)), split)
    applied, held = np.zeros(len(split), dtype=np.int64), np.zeros(len(split), dtype=np.int64)
    seen = np.zeros((rc.LOOP_TICKS, batch), dtype=np.int64)
    worst = 0.0
    for t in range(rc.LOOP_TICKS):
        pre = loop.given.cpu().numpy()
        out = loop.step()
        x, status, post = out["x"].cpu().numpy(), out["status"].cpu().numpy(), loop.given.cpu().numpy()
        seen[t] = status
        for b in range(batch):
            if rc.applies(int(status[b]), on_unsolved):
                assert np.isfinite(x[b]).all()
                ref = rc.first_step_reference(plan, A[b, t], B[b, t], pre[b], x[b])
                worst = max(worst, assert_componentwise(post[b], *ref, kap1, "tick %d, instance %d" % (t, b)))
                applied[group_of[b]] += 1
            else:
                assert np.array_equal(post[b], pre[b]), (t, b)
                held[group_of[b]] += 1
    if on_unsolved == "hold":
        assert (applied > 0).all() and (held > 0).all(), seen.tolist()
    else:
        assert applied.sum() == rc.LOOP_TICKS * batch and not held.any(), seen.tolist()
    record("f loop %s" % on_unsolved, "next given %6.3f of %2d   applied %s held %s per workgroup"
           % (worst, kap1, applied.tolist(), held.tolist()))
