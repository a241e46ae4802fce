"""What the tests of every variant of the pre-stabilisation kernels share (csrc/feedback.hip: ``ltv_lqr_kernel<NS, MS>``
and ``ltv_true_inputs_kernel<NS, MS>``, sixteen instantiations each, ``ltv_close_kernel`` and ``ltv_augment_kernel``):
the shapes, the launch geometries each case claims, the inputs, and the bounds a single step of the Riccati sweep is
held to -- all in numpy, built once and read-only; used by the CPU premises (test_ltv_feedback_cpu.py) and by the
GPU tests (test_gpu_ltv_feedback_variants.py)."""
import functools

import numpy as np

import augment_cases as ac
import feedback_restatement as fr
import rollout_cases as rc
import sweep_cases as sc
from helpers import LD, U64

FB_BLOCK = 64           # lanes of a workgroup of ltv_lqr_kernel and ltv_true_inputs_kernel (one wavefront)
CLOSE_BLOCK = 256       # lanes of a workgroup of ltv_close_kernel and ltv_augment_kernel
NM = [(n, m) for n in range(1, 5) for m in range(1, 5)]


def _frozen(*arrays):
    for v in arrays:
        v.setflags(write=False)
    return arrays


# --------------------------------------------------------------------------------------------------
# (a), (b) the true inputs: lane w = instance * axes + axis, 64 lanes to a workgroup
# --------------------------------------------------------------------------------------------------
# every instantiation: rollout_cases.NM_SHAPES (N = 5 on two axes: the second axis' columns of optim start behind
# the first's), 11 instances on sequences of N + 2 steps, windows at t = 0 and t = 2, random gains N(0, 0.3)
TRUE_SHAPES = rc.NM_SHAPES
TRUE_BATCH, TRUE_TICKS, GAIN_SIGMA = 11, (0, 2), 0.3
# three axes: an instance's lanes can lie in two workgroups (64 is no multiple of 3)
EXTRA = {"three-2-2": sc.Shape("three-2-2", None, 2, 2, 5, 3, 0, False, False, 0, ())}

# (shape, axes, {count: (workgroups, lanes of the last one)}): the claim of each case, written down from
# ``lanes = count * axes`` -- test_ltv_feedback_cpu.py holds true_lanes to it, the GPU test runs every count with
# the batch of the largest
TRUE_GEOMETRY = [
    ("nm-2-2", 2, {31: (1, 62), 32: (1, 64), 33: (2, 2), 70: (3, 12)}),       # one short, exactly one, one past, two full
    ("one-1-1-1", 1, {64: (1, 64), 65: (2, 1)}),                              # N = 1, ng = no = 1: odd everything
    ("four-a4-n4", 4, {16: (1, 64), 17: (2, 4)}),
    ("three-2-2", 3, {21: (1, 63), 22: (2, 2)}),
]
# the instances whose axes lie in two workgroups: at 22 instances on three axes, instance 21 has axis 0 on lane 63
# of the first workgroup and axes 1 and 2 on lanes 0 and 1 of the second; nowhere else
STRADDLERS = {("three-2-2", 22): (21,)}
TRUE_WINDOW = 1         # the tick of the geometry cases: the window starts one step into the sequences
# (shape, batch, count, rows of given, {instance: the row its index names}): -1, `rows` and 2^31 - 1 are not there.
# On two axes instance 31's second axis is lane 63, the last of the first workgroup; 32 is the second's first
MISSING = ("nm-2-2", 70, 33, 23, {5: -1, 31: 23, 32: 2 ** 31 - 1})


def shape_of(name):
    return EXTRA[name] if name in EXTRA else rc.shape_of(name)


def true_lanes(count, axes):
    """``(workgroups, lanes of the last one)`` of ``mpcasm_ltv_true_inputs`` at ``count`` instances."""
    lanes = count * axes
    groups = -(-lanes // FB_BLOCK)
    return groups, lanes - (groups - 1) * FB_BLOCK


def straddlers(count, axes):
    """The instances below ``count`` whose first and last lane lie in different workgroups."""
    return tuple(b for b in range(count) if (b * axes) // FB_BLOCK != (b * axes + axes - 1) // FB_BLOCK)


def plants_and_gains(rng, batch, shape, steps=None):
    """``A (batch, T, n, n), B (batch, T, n, m), K (batch, T, m, n)`` with ``T = N + 2`` steps: sweep_cases.plants
    over the longer sequence, gains N(0, 0.3) -- true_inputs needs a closed loop, not an optimal one."""
    T = shape.N + 2 if steps is None else steps
    A, B = sc.plants(rng, batch, shape._replace(N=T))
    K = rng.normal(0.0, GAIN_SIGMA, (batch, T, shape.m, shape.n))
    return _frozen(A, B, K)


# --------------------------------------------------------------------------------------------------
# (c) one step of the Riccati sweep
# --------------------------------------------------------------------------------------------------
STEP_T, STEP_BATCH = 2, 70              # two workgroups, the second of six lanes
STEP_SEED = 29
# the instantiations test_gpu_ltv_feedback.py's chains leave out, one chain each under that test's own rule
CHAIN_T, CHAIN_BATCH = 7, 3
CHAIN_SHAPES = [(n, m, CHAIN_T, CHAIN_BATCH) for n, m in NM if (n, m) not in {s[:2] for s in fr.RICCATI_SHAPES}]


@functools.lru_cache(maxsize=None)
def step_case(n, m):
    """``A (70, 2, n, n), B (70, 2, n, m), Q, R, terminal``: feedback_restatement.riccati_case's random plants
    (spectral radius 1.3 .. 1.4, ``Q = G G' + 1e-3 I``, ``R = H H' + 1e-2 I``) and a random SPD terminal weight of
    its own, ``W W' + 1e-3 I``."""
    A, B, Q, R = fr.riccati_case(None, (n, m, STEP_T, STEP_BATCH))
    W = np.random.default_rng(STEP_SEED + 10 * n + m).standard_normal((n, n))
    terminal = W @ W.T + 1e-3 * np.eye(n)
    assert not np.array_equal(terminal, Q)
    return _frozen(A, B, Q, R, terminal)


def step_constants(n, m):
    """``(2 n + 3 m + 2, 2 n + m + 2)``: the roundings behind the residual of one step's gain, and those the
    device's own ``P_1`` carries into step 0 (:func:`step_residuals`)."""
    return 2 * n + 3 * m + 2, 2 * n + m + 2


def step_residuals(A, B, Q, R, terminal, K):
    """The residuals of the two gains ``K (batch, 2, m, n)`` of a sweep over ``T = 2`` steps and their bounds,
    everything in long double on the fp64 inputs and ``|.|`` elementwise: ``(res1, bound1, res0, bound0)``, each
    ``(batch, m, n)``.

    Step 1 (``P = terminal``): ``K_1`` solves ``S K = -W`` with ``S = R + B' P B`` and ``W = B' P A``.  An element of
    ``P B`` is an inner product of length n, one of ``S`` adds n products to it and the term of ``R``, one of ``W`` n
    products: ``2 n + 1`` roundings, so ``|dS| <= (2 n + 1) u (|R| + |B'| |P| |B|)`` and ``|dW| <= (2 n + 1) u |B'| |P|
    |A|``.  The Cholesky solve of an ``m x m`` system has a backward error of ``3 m + 1`` roundings (Higham, Accuracy
    and Stability, Theorem 10.4: ``|dS| <= gamma_{3m+1} |L| |L'|``), taken here on the magnitudes of ``S`` the sums
    above were formed from; test_ltv_feedback_cpu.py holds the fp64 restatement to the result.  Together

        |(R + B' P B) K_1 + B' P A| <= (2 n + 3 m + 2) u [ (|R| + |B'| |P| |B|) |K_1| + |B'| |P| |A| ].

    Step 0: the same residual with ``P_1 = sym(Q + A_1' (P (A_1 + B_1 K_1)))`` in long double from the gains ``K_1``
    that are passed in (teacher-forced: the device's own).  The device's ``P_1`` differs from that one by its own
    roundings -- m + 1 for ``A_cl``, n for ``P A_cl``, n + 1 for ``Q + A' (.)``, none for the mean: ``2 n + m + 2`` --
    on the magnitudes ``M_P = sym(|Q| + |A_1'| |P| (|A_1| + |B_1| |K_1|))``, which adds

        (2 n + m + 2) u (|B_0'| M_P |B_0| |K_0| + |B_0'| M_P |A_0|)."""
    f = lambda v: np.asarray(v, dtype=LD)
    mag = np.abs
    A, B, Q, R, P, K = (f(v) for v in (A, B, Q, R, terminal, K))
    n, m = B.shape[-2:]
    c_step, c_carry = step_constants(n, m)
    u = LD(U64)
    tr = lambda v: np.swapaxes(v, -1, -2)

    def residual(k, P):
        return mag((R + tr(B[:, k]) @ P @ B[:, k]) @ K[:, k] + tr(B[:, k]) @ P @ A[:, k])

    def magnitude(k, absP, absR):
        return (absR + mag(tr(B[:, k])) @ absP @ mag(B[:, k])) @ mag(K[:, k]) + mag(tr(B[:, k])) @ absP @ mag(A[:, k])

    res1, bound1 = residual(1, P), c_step * u * magnitude(1, mag(P), mag(R))
    P1 = Q + tr(A[:, 1]) @ (P @ (A[:, 1] + B[:, 1] @ K[:, 1]))
    P1 = (P1 + tr(P1)) / 2
    MP = mag(Q) + mag(tr(A[:, 1])) @ (mag(P) @ (mag(A[:, 1]) + mag(B[:, 1]) @ mag(K[:, 1])))
    MP = (MP + tr(MP)) / 2
    res0 = residual(0, P1)
    bound0 = c_step * u * magnitude(0, mag(P1), mag(R)) + c_carry * u * magnitude(0, MP, 0 * mag(R))
    return res1, bound1, res0, bound0


def step_ratios(A, B, Q, R, terminal, K):
    """``(worst residual / bound at step 1, at step 0)`` over every element of every instance; NaN where a gain is
    not finite."""
    res1, bound1, res0, bound0 = step_residuals(A, B, Q, R, terminal, K)
    if not np.isfinite(np.asarray(K, dtype=float)).all():
        return float("nan"), float("nan")
    return float((res1 / bound1).max()), float((res0 / bound0).max())


# --------------------------------------------------------------------------------------------------
# (d) the failure paths: a LATER pivot that is not positive
# --------------------------------------------------------------------------------------------------
# (n, m): R = diag(1, .., 1, 0) and, at the failing step, the last column of B zero -- S's last row and column are
# exactly 0 there: every pivot but the last is positive (n >= m: B' P B is regular elsewhere)
FAIL_SHAPES = [(3, 2), (4, 4)]
FAIL_T, FAIL_BATCH = 5, 70
# instance: the step it fails at -- the last step of the sweep's first (every row NaN), the last (only step 0
# NaN), one between; instance 5 in the first workgroup, 64 the first lane and 69 the last live lane of the second
FAILS = {5: FAIL_T - 1, 64: 0, 69: 2}


@functools.lru_cache(maxsize=None)
def failure_case(n, m):
    """``A (70, 5, n, n), B (70, 5, n, m), Q = I, R = diag(1, .., 1, 0)``."""
    rng = np.random.default_rng(41 + 10 * n + m)
    A = rng.standard_normal((FAIL_BATCH, FAIL_T, n, n))
    B = rng.standard_normal((FAIL_BATCH, FAIL_T, n, m))
    for b, k in FAILS.items():
        B[b, k, :, m - 1] = 0.0
    R = np.eye(m)
    R[m - 1, m - 1] = 0.0
    return _frozen(A, B, np.eye(n), R)


# --------------------------------------------------------------------------------------------------
# (e) close and augment: one lane per element, 256 to a workgroup
# --------------------------------------------------------------------------------------------------
AUGMENT_NM = [(n, m) for n, m in NM if n + m <= 4]
# (T, batch): at n = m = 2 At ends exactly on its second workgroup and Bt, Kt exactly on their first (512, 256,
# 256 elements) -- the hand-over from region to region with no partial block between; and sizes where none does
AUGMENT_SIZES = {"exact": (4, 8), "ragged": (3, 7)}
# the (n, m) ltv_close has not run at (the five Riccati shapes and the stride test's (3, 2) aside)
CLOSE_NM = [nm for nm in NM if nm not in {s[:2] for s in fr.RICCATI_SHAPES} | {(3, 2)}]
# (T, batch): batch T = 256 makes batch T n n a multiple of 256 at every n; 21 n n is one at none
CLOSE_SIZES = {"exact": (4, 64), "ragged": (3, 7)}


def augment_blocks(n, m, T, batch):
    """``((totalA, totalB, totalK), (blocksA, blocksB, blocksK))`` of ``mpcasm_ltv_augment``'s launch."""
    nz, steps = n + m, batch * T
    totals = (steps * nz * nz, steps * nz * m, steps * m * nz)
    return totals, tuple(-(-t // CLOSE_BLOCK) for t in totals)


def close_blocks(n, T, batch):
    """``(total, blocks)`` of ``mpcasm_ltv_close``'s launch."""
    total = batch * T * n * n
    return total, -(-total // CLOSE_BLOCK)


def augment_case(n, m, size):
    """``A, B, K`` (per-step gains) of augment_cases.case at ``AUGMENT_SIZES[size]``."""
    T, batch = AUGMENT_SIZES[size]
    return _frozen(*ac.case((n, m, T, batch), "per-step"))


def close_case(n, m, size):
    T, batch = CLOSE_SIZES[size]
    return _frozen(*ac.case((n, m, T, batch), "per-step"))


# --------------------------------------------------------------------------------------------------
# (f) a closed loop on a plant with two inputs
# --------------------------------------------------------------------------------------------------
LOOP_SHAPE, LOOP_BATCH, LOOP_TICKS, LOOP_SEED = "nm-2-2", 5, 3, 53


def loop_inputs(api):
    """``form, A_seq (5, 7, 2, 2), B_seq (5, 7, 2, 2), given (5, ng)``: random plants of spectral radius 1.3 .. 1.4
    at every step (as feedback_restatement.riccati_case's), ``N + ticks - 1`` steps; the formulation of
    rollout_cases' ``nm-2-2`` on the first of them -- tracking costs and an effort cost, no limits."""
    shape = shape_of(LOOP_SHAPE)
    T = shape.N + LOOP_TICKS - 1
    rng = np.random.default_rng(LOOP_SEED)
    A = rng.standard_normal((LOOP_BATCH, T, shape.n, shape.n))
    A *= (rng.uniform(1.3, 1.4, (LOOP_BATCH, T)) / np.abs(np.linalg.eigvals(A)).max(axis=-1))[..., None, None]
    B = rng.standard_normal((LOOP_BATCH, T, shape.n, shape.m))
    form = sc.build(api, rng, shape, plant=(A[0, 0].copy(), B[0, 0].copy()))
    given = rng.normal(0.0, 0.3, (LOOP_BATCH, form.given_len))
    return (form,) + _frozen(A, B, given)
