"""GPU: every variant of the pre-stabilisation kernels (csrc/feedback.hip: ``mpcasm_ltv_true_inputs``,
``mpcasm_ltv_lqr``, ``mpcasm_ltv_close``, ``mpcasm_ltv_augment``) and every edge of their launch geometry against
extended precision, beside test_gpu_ltv_feedback.py and test_gpu_ltv_augment.py, which run the pendulum and a few
shapes more (feedback_cases.py holds the cases, test_ltv_feedback_cpu.py their premises):

  (a) the sixteen ``ltv_true_inputs_kernel<NS, MS>`` on two axes, at two windows, per-instance and shared gains;
  (b) the true inputs' lanes: partial, full and further workgroups on one to four axes, an instance whose axes lie
      in two workgroups, fewer instances than the batch, indices that name no row of ``given``;
  (c) the sixteen ``ltv_lqr_kernel<NS, MS>`` one step at a time -- the residual of each gain under a terminal weight
      that is not Q -- and a chain for the eleven that had none;
  (d) the sweep's failure paths: a later pivot, the first and the last step, a later workgroup, no ``A_cl``, T = 0;
  (e) ``ltv_augment`` at its six (n, m) and ``ltv_close`` at the ten it had not run at, regions and totals that end
      exactly on a workgroup and ones that do not;
  (f) ``LtvLoop(feedback=)`` on a plant with two inputs, teacher-forced tick by tick.

Every launch whose output the test can allocate writes into NaN-filled buffers (-99 for ``info``) with guard
elements in front and behind -- where the engine allocates the output itself, the C entry is called directly.  The
worst ratio of every case is kept in profiles/ltv_feedback_variants.txt."""
import os
import types

import numpy as np
import pytest

import augment_cases as ac
import feedback_cases as fc
import feedback_restatement as fr
import rollout_cases as rc
import sweep_cases as sc
from helpers import LD, assert_componentwise

pytestmark = pytest.mark.gpu
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       "ltv_feedback_variants.txt")
HEAD = ("# the pre-stabilisation kernels (csrc/feedback.hip), every variant: the worst of every case over all its\n"
        "# instances -- errors in u M (u = 2^-53) beside their bound, residuals as a fraction of theirs;\n"
        "# written by tests/test_gpu_ltv_feedback_variants.py\n")
KEY = 30
NAN = float("nan")
FRONT = 16              # guard elements in front of every carved output


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def record(key, text):
    """One line per case in profiles/ltv_feedback_variants.txt (a checkout that cannot be written is left alone)."""
    print("ltv-feedback-variants: %-*s %s" % (KEY, key, text))
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


def _dev(torch, v):
    return torch.as_tensor(np.array(v, order="C"), device="cuda")      # (a copy: the shared cases are read-only)


def _bits(v):
    return np.ascontiguousarray(v).view(np.int64)


def carve(torch, shape, behind, dtype=None, fill=NAN):
    """``(whole, view)``: ``view`` of ``shape`` inside a filled buffer, FRONT elements in front, ``behind`` behind."""
    size = int(np.prod(shape))
    whole = torch.full((FRONT + size + behind,), fill, dtype=dtype or torch.float64, device="cuda")
    return whole, whole[FRONT:FRONT + size].view(*shape)


def untouched(torch, whole, used, fill=NAN):
    """Nothing in front of the view or from ``used`` elements into it on has been written."""
    outside = torch.cat([whole[:FRONT], whole[FRONT + used:]])
    return bool(torch.isnan(outside).all()) if fill != fill else bool((outside == fill).all())


def same(torch, a, b):
    """Equal bit for bit where finite, NaN in the same places."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) \
        and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


# ---- the true inputs ---------------------------------------------------------------------------------------------
_CASES = {}


def case(api, torch, name, batch):
    """``batch`` instances of shape ``name``, made once and never changed: per-step plants of N + 2 steps, random
    gains, the closed loop ``engine.ltv_close`` builds of them, initial states and unknowns; ``ref(b, t, row)``: the
    long-double true inputs of instance b over the window at t from ``row`` of given, computed once."""
    if (name, batch) in _CASES:
        return _CASES[(name, batch)]
    from mpcasm import engine

    shape = fc.shape_of(name)
    rng = np.random.default_rng([batch, 700] + [ord(ch) for ch in name])
    A, B, K = fc.plants_and_gains(rng, batch, shape)
    form = sc.build(api, rng, shape, plant=(A[0, 0].copy(), B[0, 0].copy()))    # (copies: the case is read-only)
    dyn = sc.dynamics_name(shape)
    asm = engine.Assembler(form, batch=batch, ltv=[dyn])
    sw = asm.plan.sweep
    assert (sw["n"], sw["m"], sw["N"], sw["axes"].shape[0]) == (shape.n, shape.m, shape.N, shape.axes)
    c = types.SimpleNamespace(name=name, shape=shape, batch=batch, dyn=dyn, asm=asm, plan=asm.plan, A=A, B=B, K=K,
                              axes=shape.axes, N=shape.N, T=A.shape[1],
                              given=rng.normal(0, 0.3, [batch, asm.ng]), optim=rng.normal(0, 0.5, [batch, asm.no]),
                              kap=rc.kappa_rollout(shape.N, shape.n, shape.m))
    c.dA, c.dB, c.dK = _dev(torch, A), _dev(torch, B), _dev(torch, K)
    c.dAcl = engine.ltv_close(c.dA, c.dB, c.dK)
    c.Acl = c.dAcl.cpu().numpy()
    c.g, c.x = _dev(torch, c.given), _dev(torch, c.optim)
    for v in (c.given, c.optim, c.Acl):
        v.setflags(write=False)
    refs = {}

    def ref(b, t, given=None, gains=None):
        key = (b, t, None if given is None else given.tobytes(), None if gains is None else gains.tobytes())
        if key not in refs:
            w = slice(t, t + c.N)
            refs[key] = fr.true_inputs(c.plan, c.Acl[b, w], B[b, w], (K[b] if gains is None else gains)[w],
                                       c.given[b] if given is None else given, c.optim[b], dtype=LD)
        return refs[key]

    c.ref = ref
    _CASES[(name, batch)] = c
    return c


def run_true(torch, c, t, count, given=None, index=None, gains=None):
    """One launch of ``count`` instances over the window at ``t`` into NaN: ``(count, axes, N, m)`` on the host.  The
    buffer holds the whole batch's rows and a workgroup's worth of lanes behind them; everything from row ``count`` on,
    and both guards, must keep their NaN."""
    c.asm.bind_ltv_window(c.dyn, c.dAcl, c.dB, t)
    m = c.shape.m
    whole, out = carve(torch, (c.batch, c.axes, c.N, m), fc.FB_BLOCK * c.N * m)
    got = c.asm.true_inputs(c.dK if gains is None else gains, t, c.g if given is None else given, c.x, index=index,
                            out=out, count=count)
    assert got is out
    assert untouched(torch, whole, count * c.axes * c.N * m), (c.name, count, "written outside the launch's rows")
    return out[:count].cpu().numpy()


def against_reference(c, got, t, instances, what, given_of=None):
    """Every listed instance within kappa_rollout(N, n, m) (u M + 2^-1022) of the long-double restatement on the
    device's own A_cl; the worst error in u M."""
    worst = 0.0
    for b in instances:
        ref = c.ref(b, t, None if given_of is None else given_of(b))
        worst = max(worst, assert_componentwise(got[b], *ref, c.kap, "%s, window %d, instance %d" % (what, t, b)))
    return worst


# ---- (a) every instantiation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.TRUE_SHAPES)
def test_every_true_input_instantiation(gpu_api, torch_gpu, name):
    """n, m in 1 .. 4, N = 5 on two axes (the second axis' unknowns start behind the first's: ``ucol`` is not 0), 11
    instances, windows at t = 0 and t = 2 of sequences of 7 steps; and one gain sequence for the whole batch
    (k_stride = 0) bit for bit what the replicated one gives."""
    torch = torch_gpu
    c = case(gpu_api, torch, name, fc.TRUE_BATCH)
    count, m = fc.TRUE_BATCH, c.shape.m
    assert c.T == c.N + 2 == 7 and c.axes == 2 and fc.true_lanes(count, c.axes) == (1, 22)
    ucol = np.asarray(c.plan.sweep["axes"])[:, 1:1 + m]
    assert (ucol[1] > 0).all() and len(set(ucol.ravel().tolist())) == 2 * m
    worst = 0.0
    for t in fc.TRUE_TICKS:
        got = run_true(torch, c, t, count)
        worst = max(worst, against_reference(c, got, t, range(count), name))
    shared = c.dK[1].contiguous()
    one = run_true(torch, c, 2, count, gains=shared)
    each = run_true(torch, c, 2, count, gains=shared[None].expand(count, -1, -1, -1).contiguous())
    assert np.array_equal(_bits(one), _bits(each)) and np.array_equal(_bits(one[1]), _bits(got[1]))
    assert not np.array_equal(one[0], got[0])
    # ... and it is held to the reference on those gains too
    for b in range(count):
        assert_componentwise(one[b], *c.ref(b, 2, gains=c.K[1]), c.kap, "%s, shared gains, instance %d" % (name, b))
    record("a true_inputs<%d,%d>" % (c.shape.n, m), "%6.3f of %3d u M   windows %s, %d instances"
           % (worst, c.kap, " ".join(map(str, fc.TRUE_TICKS)), count))


# ---- (b) lanes, workgroups and guards ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,axes,counts", fc.TRUE_GEOMETRY, ids=[g[0] for g in fc.TRUE_GEOMETRY])
def test_true_input_lanes_and_workgroups(gpu_api, torch_gpu, name, axes, counts):
    """Every count of the case in an assembler of the largest: the lane arithmetic the case claims first, then every
    instance below ``count`` within the bound -- the one whose axes lie in two workgroups among them -- and, where
    the batch is larger than ``count``, nothing written from row ``count`` on (run_true)."""
    torch = torch_gpu
    batch = max(counts)
    c = case(gpu_api, torch, name, batch)
    assert c.axes == axes
    worst, t = 0.0, fc.TRUE_WINDOW
    for count, claim in counts.items():
        assert fc.true_lanes(count, axes) == claim
        split = fc.straddlers(count, axes)
        assert split == fc.STRADDLERS.get((name, count), ())
        got = run_true(torch, c, t, count)
        worst = max(worst, against_reference(c, got, t, range(count), "%s, %d of %d" % (name, count, batch)))
        for b in split:     # (named: the instance of lanes 63, 64, 65)
            assert np.isfinite(got[b]).all() and b * axes // 64 + 1 == (b * axes + axes - 1) // 64
    record("b lanes %s" % name, "%6.3f of %3d u M   axes %d, counts %s" % (worst, c.kap, axes,
                                                                           " ".join(str(k) for k in counts)))


def test_true_inputs_of_rows_that_are_not_there(gpu_api, torch_gpu):
    """nm-2-2, 33 of 70 instances by a device index into 23 rows of ``given``; instances 5, 31 (its second axis is lane
    63, the first workgroup's last) and 32 (the second workgroup's first) name row -1, row 23 and row 2^31 - 1.  Their
    blocks of ``out`` keep their NaN; every other instance is within the bound, and bit for bit what the index
    without those three gives."""
    torch = torch_gpu
    name, batch, count, rows, wild = fc.MISSING
    c = case(gpu_api, torch, name, batch)
    assert fc.true_lanes(count, c.axes) == (2, 2) and (31 * c.axes + 1) % fc.FB_BLOCK == fc.FB_BLOCK - 1
    rng = np.random.default_rng(77)
    big = rng.normal(0, 0.3, [rows, c.asm.ng])
    valid = rng.integers(0, rows, count).astype(np.int32)
    index = valid.copy()
    for b, row in wild.items():
        index[b] = row
    assert index.dtype == np.int32 and sorted(index[list(wild)].tolist()) == [-1, rows, 2 ** 31 - 1]
    t, dbig = fc.TRUE_WINDOW, _dev(torch, big)
    full = run_true(torch, c, t, count, given=dbig, index=_dev(torch, valid))
    got = run_true(torch, c, t, count, given=dbig, index=_dev(torch, index))
    there = [b for b in range(count) if b not in wild]
    assert np.isnan(got[list(wild)]).all() and np.isfinite(full).all()
    assert np.array_equal(_bits(got[there]), _bits(full[there]))
    worst = against_reference(c, got, t, there, "an index with three rows missing", given_of=lambda b: big[index[b]])
    record("b missing rows %s" % name, "%6.3f of %3d u M   %d of %d, rows %s of %d missing"
           % (worst, c.kap, count, batch, " ".join(str(wild[b]) for b in sorted(wild)), rows))


# ---- the Riccati sweep through the C entry, into guarded buffers ------------------------------------------------------
def lqr_guarded(torch, A, B, Q, R, terminal=None, want_closed=True, steps=None):
    """``mpcasm_ltv_lqr`` on host arrays ``A (batch, T, n, n), B (batch, T, n, m)`` with ``K``, ``A_cl`` and ``info``
    carved out of padded buffers (NaN, -99): a workgroup's worth of instances behind each, FRONT elements in front.
    Asserts that nothing outside the ``batch`` instances' own elements is written; returns device views ``(K, A_cl
    or None, info)``.  ``steps``: the T the entry is told (0: no step at all)."""
    from mpcasm import capi

    batch, T, n, m = A.shape[0], A.shape[1], A.shape[2], B.shape[3]
    told = T if steps is None else steps
    dA, dB, dQ, dR = (_dev(torch, v) for v in (A, B, Q, R))
    dP = None if terminal is None else _dev(torch, terminal)
    Kw, K = carve(torch, (batch, told, m, n), fc.FB_BLOCK * max(told, 1) * m * n)
    Cw, C = carve(torch, (batch, told, n, n), fc.FB_BLOCK * max(told, 1) * n * n) if want_closed else (None, None)
    Iw, info = carve(torch, (batch,), fc.FB_BLOCK, dtype=torch.int32, fill=-99)
    code = capi.load().mpcasm_ltv_lqr(n, m, told, batch, dA.data_ptr(), T * n * n, dB.data_ptr(), T * n * m,
                                      dQ.data_ptr(), dR.data_ptr(), None if dP is None else dP.data_ptr(),
                                      Kw.data_ptr() + 8 * FRONT, None if C is None else Cw.data_ptr() + 8 * FRONT,
                                      Iw.data_ptr() + 4 * FRONT, None)
    assert code == capi.OK
    torch.cuda.synchronize()
    assert untouched(torch, Kw, K.numel()), "K written outside the batch's instances"
    assert C is None or untouched(torch, Cw, C.numel()), "A_cl written outside the batch's instances"
    assert untouched(torch, Iw, batch, fill=-99), "info written outside the batch's instances"
    return K, C, info


# ---- (c) every instantiation, one step at a time -------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", fc.NM, ids=["%d-%d" % nm for nm in fc.NM])
def test_every_riccati_instantiation_one_step_at_a_time(gpu_api, torch_gpu, n, m):
    """T = 2, 70 instances (two workgroups, the second of six lanes), a random SPD terminal weight that is not Q:
    the residual of K_1 within (2 n + 3 m + 2) u of its magnitudes, that of K_0 on the P_1 of the device's own K_1
    within the same plus (2 n + m + 2) u of P_1's (feedback_cases.step_residuals: the derivation; the fp64
    restatement reaches at most 0.23 and 0.13 of them, test_ltv_feedback_cpu.py), and A_cl at both steps within
    (m + 2) u (|A| + |B| |K|) -- a wrong element of a gain is off by orders of magnitude."""
    torch = torch_gpu
    from mpcasm import engine

    A, B, Q, R, terminal = fc.step_case(n, m)
    K, Acl, info = lqr_guarded(torch, A, B, Q, R, terminal)
    assert (info == -1).all()
    Kh, Ah = K.cpu().numpy(), Acl.cpu().numpy()
    r1, r0 = fc.step_ratios(A, B, Q, R, terminal, Kh)
    print("ltv-feedback-variants: lqr<%d,%d>: residual / bound %.3g at step 1, %.3g at step 0" % (n, m, r1, r0))
    assert np.isfinite(Kh).all() and r1 <= 1.0 and r0 <= 1.0, ((n, m), r1, r0)
    worst = assert_componentwise(Ah, fr.close(A, B, Kh, dtype=LD), fr.close(A, B, Kh, dtype=LD, magnitude=True), m + 2,
                                 "ltv_lqr's A_cl, (%d, %d)" % (n, m))
    # the Python layer's own buffers hold the same numbers, and the terminal weight is what made them
    K2, Acl2, info2 = engine.ltv_lqr(_dev(torch, A), _dev(torch, B), np.array(Q), np.array(R), terminal=np.array(terminal))
    assert torch.equal(K2, K) and torch.equal(Acl2, Acl) and torch.equal(info2, info)
    K3 = engine.ltv_lqr(_dev(torch, A), _dev(torch, B), np.array(Q), np.array(R), want_closed=False)[0]
    assert not torch.equal(K3[:, 1], K[:, 1])
    record("c lqr<%d,%d>" % (n, m), "step 1 %5.3f  step 0 %5.3f of their bounds   A_cl %5.3f of %d u M"
           % (r1, r0, worst, m + 2))


@pytest.mark.parametrize("shape", fc.CHAIN_SHAPES, ids=["-".join(map(str, s)) for s in fc.CHAIN_SHAPES])
def test_a_chain_for_the_other_eleven_instantiations(gpu_api, torch_gpu, shape):
    """test_gpu_ltv_feedback.test_the_gains_and_the_closed_loop_matrices' forward-error rule -- every step's K within
    max(8 x the fp64 restatement's own error on that instance, 16 (n + m) u) relative to the step's largest |K*| --
    at T = 7, three instances, for the (n, m) its five shapes leave out."""
    torch = torch_gpu
    n, m, T, batch = shape
    A, B, Q, R = fr.riccati_case(gpu_api, shape)
    K_ref = np.stack([fr.lqr(A[b], B[b], Q, R, dtype=LD)[0] for b in range(batch)])
    own = np.array([fr.gain_errors(fr.lqr(A[b], B[b], Q, R)[0], K_ref[b]).max() for b in range(batch)])
    K, Acl, info = lqr_guarded(torch, A, B, Q, R)
    assert (info == -1).all()
    Kh = K.cpu().numpy()
    err = fr.gain_errors(Kh, K_ref)
    bound = np.maximum(8.0 * own, 16.0 * (n + m))
    ratio = (err / bound[:, None, None, None]).max()
    print("ltv-feedback-variants: chain %s: worst error %.3g u, restatement's own %.3g u" % (shape, err.max(), own.max()))
    assert np.isfinite(Kh).all() and ratio <= 1.0, (shape, ratio)
    worst = assert_componentwise(Acl.cpu().numpy(), fr.close(A, B, Kh, dtype=LD),
                                 fr.close(A, B, Kh, dtype=LD, magnitude=True), m + 2, "A_cl, shape %s" % (shape,))
    record("c chain lqr<%d,%d>" % (n, m), "%6.3f of its bound (%.3g u, the restatement's own %.3g u)   A_cl %5.3f of %d"
           % (ratio, err.max(), own.max(), worst, m + 2))


# ---- (d) the failure paths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", fc.FAIL_SHAPES)
def test_a_later_pivot_at_the_first_the_last_and_a_middle_step(gpu_api, torch_gpu, n, m):
    """feedback_cases.failure_case: for instances 5, 64 and 69 of 70 the LAST pivot of S is exactly 0 at step T - 1
    (every row NaN), at step 0 (only step 0 NaN) and at step 2, every earlier pivot positive -- ``info`` and the NaN
    pattern are the restatement's; every other instance is bit for bit what the batch without those three gives;
    without ``A_cl`` (d_Acl = NULL) the same K and info."""
    torch = torch_gpu
    A, B, Q, R = fc.failure_case(n, m)
    T, batch = fc.FAIL_T, fc.FAIL_BATCH
    want = [fr.lqr(A[b], B[b], Q, R) for b in range(batch)]
    K, Acl, info = lqr_guarded(torch, A, B, Q, R)
    assert info.tolist() == [w[2] for w in want] == [fc.FAILS.get(b, -1) for b in range(batch)]
    Kh, Ah = K.cpu().numpy(), Acl.cpu().numpy()
    assert np.array_equal(np.isnan(Kh), np.isnan(np.stack([w[0] for w in want])))
    assert np.array_equal(np.isnan(Ah), np.isnan(np.stack([w[1] for w in want])))
    for b, k in fc.FAILS.items():       # (spelt out: the rows of step k and of every earlier one, and no later one)
        assert np.isnan(Kh[b, :k + 1]).all() and np.isnan(Ah[b, :k + 1]).all()
        assert np.isfinite(Kh[b, k + 1:]).all() and np.isfinite(Ah[b, k + 1:]).all()
    assert np.isnan(Kh[5]).all() and np.isfinite(Kh[64, 1:]).all()
    rest = [b for b in range(batch) if b not in fc.FAILS]
    K4, Acl4, info4 = lqr_guarded(torch, A[rest], B[rest], Q, R)
    assert (info4 == -1).all() and torch.isfinite(K4).all() and torch.isfinite(Acl4).all()
    assert torch.equal(K4, K[rest]) and torch.equal(Acl4, Acl[rest])
    K5, none, info5 = lqr_guarded(torch, A, B, Q, R, want_closed=False)
    assert none is None and same(torch, K5, K) and torch.equal(info5, info)
    record("d later pivot lqr<%d,%d>" % (n, m), "info %s of instances %s, the other %d bit for bit"
           % ([fc.FAILS[b] for b in sorted(fc.FAILS)], sorted(fc.FAILS), len(rest)))


def test_no_step_at_all(gpu_api, torch_gpu):
    """T = 0 with 70 instances through the C entry: ``info`` is -1 for every instance and for nothing behind them,
    ``K`` and ``A_cl`` (no element is theirs) are not touched."""
    torch = torch_gpu
    A, B, Q, R = fc.failure_case(3, 2)
    K, Acl, info = lqr_guarded(torch, A, B, Q, R, steps=0)
    assert K.numel() == 0 and Acl.numel() == 0 and info.shape == (fc.FAIL_BATCH,) and (info == -1).all()
    record("d T = 0", "info -1 for %d instances, K and A_cl untouched" % fc.FAIL_BATCH)


# ---- (e) close and augment -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(fc.AUGMENT_SIZES))
@pytest.mark.parametrize("n,m", fc.AUGMENT_NM, ids=["%d-%d" % nm for nm in fc.AUGMENT_NM])
def test_augment_at_every_shape_into_one_buffer(gpu_api, torch_gpu, n, m, size):
    """``At``, ``Bt``, ``Kt`` carved back to back out of one NaN buffer: test_gpu_ltv_augment's assertions -- the A + B
    K block within (m + 2) u (|A| + |B| |K|) of long double and ``engine.ltv_close``'s bit for bit, every other
    element the bits of what it copies, of +0.0 or of 1.0 -- with regions that end exactly on a workgroup (``exact``
    at n = m = 2: 512, 256, 256 elements) and ones that do not; then with d_Kt = NULL."""
    torch = torch_gpu
    from mpcasm import capi, engine

    T, batch = fc.AUGMENT_SIZES[size]
    A, B, K = fc.augment_case(n, m, size)
    (totA, totB, totK), blocks = fc.augment_blocks(n, m, T, batch)
    if (n, m, size) == (2, 2, "exact"):
        assert (totA, totB, totK) == (512, 256, 256) and blocks == (2, 1, 1)
    if size == "ragged":
        assert totA % fc.CLOSE_BLOCK and totB % fc.CLOSE_BLOCK and totK % fc.CLOSE_BLOCK
    nz = n + m
    dA, dB, dK = _dev(torch, A), _dev(torch, B), _dev(torch, K)
    results = []
    for want_gain in (True, False):
        whole, _ = carve(torch, (totA + totB + totK,), fc.CLOSE_BLOCK)
        p = whole.data_ptr() + 8 * FRONT
        code = capi.load().mpcasm_ltv_augment(n, m, T, batch, dA.data_ptr(), T * n * n, dB.data_ptr(), T * n * m,
                                              dK.data_ptr(), T * m * n, m * n, p, p + 8 * totA,
                                              p + 8 * (totA + totB) if want_gain else None, None)
        assert code == capi.OK
        torch.cuda.synchronize()
        assert untouched(torch, whole, totA + totB + (totK if want_gain else 0)), (n, m, size, want_gain)
        body = whole[FRONT:FRONT + totA + totB + totK].cpu().numpy()
        results.append((body[:totA].reshape(batch, T, nz, nz), body[totA:totA + totB].reshape(batch, T, nz, m),
                        body[totA + totB:].reshape(batch, T, m, nz)))
    (At, Bt, Kt), (At2, Bt2, Kt2) = results
    assert np.array_equal(_bits(At2), _bits(At)) and np.array_equal(_bits(Bt2), _bits(Bt)) and np.isnan(Kt2).all()
    closed = At[..., :n, :n].copy()
    worst = assert_componentwise(closed, fr.close(A, B, K, dtype=LD), fr.close(A, B, K, dtype=LD, magnitude=True), m + 2,
                                 "A + B K, (%d, %d), %s" % (n, m, size))
    assert np.array_equal(_bits(closed), _bits(engine.ltv_close(dA, dB, dK).cpu().numpy()))
    want_At, want_Bt, want_Kt = ac.augmented(A, B, K)
    At[..., :n, :n] = 0.0
    for what, got, want in (("At", At, want_At), ("Bt", Bt, want_Bt), ("Kt", Kt, want_Kt)):
        assert np.array_equal(_bits(got), _bits(want)), (what, n, m, size)
    record("e augment %d-%d %s" % (n, m, size), "A + B K %5.3f of %d u M   %d %d %d elements in %d %d %d workgroups"
           % ((worst, m + 2, totA, totB, totK) + blocks))


@pytest.mark.parametrize("n,m", fc.CLOSE_NM, ids=["%d-%d" % nm for nm in fc.CLOSE_NM])
def test_close_at_the_other_ten_shapes_into_a_guarded_buffer(gpu_api, torch_gpu, n, m):
    """``mpcasm_ltv_close`` at the (n, m) it had not run at, once with a total that is a multiple of 256 and once with
    one that is not: within (m + 2) u (|A| + |B| |K|) of long double, ``engine.ltv_close``'s numbers bit for bit, and
    not an element outside A_cl."""
    torch = torch_gpu
    from mpcasm import capi, engine

    worst = []
    for size, (T, batch) in fc.CLOSE_SIZES.items():
        A, B, K = fc.close_case(n, m, size)
        total, blocks = fc.close_blocks(n, T, batch)
        assert (total % fc.CLOSE_BLOCK == 0) == (size == "exact")
        dA, dB, dK = _dev(torch, A), _dev(torch, B), _dev(torch, K)
        whole, Acl = carve(torch, (batch, T, n, n), fc.CLOSE_BLOCK)
        code = capi.load().mpcasm_ltv_close(n, m, T, batch, dA.data_ptr(), T * n * n, dB.data_ptr(), T * n * m,
                                            dK.data_ptr(), T * m * n, m * n, whole.data_ptr() + 8 * FRONT, None)
        assert code == capi.OK
        torch.cuda.synchronize()
        assert untouched(torch, whole, total), (n, m, size)
        assert torch.equal(Acl, engine.ltv_close(dA, dB, dK))
        worst.append(assert_componentwise(Acl.cpu().numpy(), fr.close(A, B, K, dtype=LD),
                                          fr.close(A, B, K, dtype=LD, magnitude=True), m + 2,
                                          "ltv_close, (%d, %d), %s" % (n, m, size)))
    record("e close %d-%d" % (n, m), "%5.3f %5.3f of %d u M   exact, ragged" % (worst[0], worst[1], m + 2))


# ---- (f) a closed loop with two inputs ---------------------------------------------------------------------------------
def test_the_loop_on_a_plant_with_two_inputs(gpu_api, torch_gpu):
    """``LtvLoop(feedback={"Q": I, "R": I})`` on nm-2-2 (no limits: every instance solves), five instances, three
    ticks, teacher-forced: per tick ``u (B, 2, N, 2)`` within kappa_rollout(N, n, m) of the long-double true inputs
    on the tick's own ``given`` and the device's ``x``, and the advanced ``given`` within kappa_rollout(1, n, m) of
    the long-double first step on A_cl_t."""
    torch = torch_gpu
    from mpcasm import capi
    from mpcasm.ltv_loop import LtvLoop

    form, A, B, given0 = fc.loop_inputs(gpu_api)
    shape = fc.shape_of(fc.LOOP_SHAPE)
    n, m, N, batch = shape.n, shape.m, shape.N, fc.LOOP_BATCH
    loop = LtvLoop(form, sc.dynamics_name(shape), batch, _dev(torch, A), _dev(torch, B),
                   feedback={"Q": np.eye(n), "R": np.eye(m)})
    assert loop.asm.nc == 0 and loop.horizon == N and loop.ticks_possible == fc.LOOP_TICKS
    assert loop.K_seq.shape == (batch, A.shape[1], m, n) and loop.A_cl_seq.shape == A.shape
    loop.given.copy_(_dev(torch, given0))
    plan = loop.asm.plan
    Acl, Kh = loop.A_cl_seq.cpu().numpy(), loop.K_seq.cpu().numpy()
    kap, kap1 = rc.kappa_rollout(N, n, m), rc.kappa_rollout(1, n, m)
    worst, worst1 = 0.0, 0.0
    for t in range(fc.LOOP_TICKS):
        pre = loop.given.cpu().numpy()
        out = loop.step()
        assert set(out) == {"x", "status", "iters", "u"} and out["u"].shape == (batch, 2, N, 2)
        x, status, post, u = (v.cpu().numpy() for v in (out["x"], out["status"], loop.given, out["u"]))
        assert status.tolist() == [capi.QP_SOLVED] * batch, (t, status.tolist())
        for b in range(batch):
            w = slice(t, t + N)
            ref = fr.true_inputs(plan, Acl[b, w], B[b, w], Kh[b, w], pre[b], x[b], dtype=LD)
            worst = max(worst, assert_componentwise(u[b], *ref, kap, "u, tick %d, instance %d" % (t, b)))
            ref = rc.first_step_reference(plan, Acl[b, t], B[b, t], pre[b], x[b])
            worst1 = max(worst1, assert_componentwise(post[b], *ref, kap1, "given, tick %d, instance %d" % (t, b)))
            assert not np.array_equal(post[b], pre[b])
    record("f loop %s" % fc.LOOP_SHAPE, "u %6.3f of %3d   next given %6.3f of %2d u M   %d ticks, %d instances, all solved"
           % (worst, kap, worst1, kap1, fc.LOOP_TICKS, batch))
