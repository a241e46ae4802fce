"""A family of shapes that spans every variant of the horizon fill (csrc/fill.hip: fill_choose picks one of seven
kernels, their instantiations, the systems per wavefront and the quad kernel's row grouping from ``(ltv, batch,
N, n, m)`` and from whether S and U are both 16-byte aligned), shared by the CPU test of the decision and of the
bound (test_fill_routes_cpu.py) and the GPU test of the kernels (test_gpu_fill_variants.py).

Every case pins the route the library reports for it (``engine.fill_route``): ``route`` for outputs on a 16-byte
boundary and, where the decision depends on that, ``off8`` for outputs 8 bytes off one.  The shapes are the
smallest that still exercise what the variant does differently, N >= 5 wherever the route allows (so that the
recurrence and the Toeplitz shift both act); N = 1 and N = 2 are cases of their own.  All kernels run the same
recurrence in the same order of association (the first product, then fused multiply-adds in the order of the
states), so a launch 8 bytes off reproduces the aligned launch bit for bit, whatever kernels the two ran on --
but for the sign of an exact zero: the quad and row kernels start a sum with the product ``a[0] * x[0]``, the
others with ``fma(a[0], x[0], +0.0)``, which differ where that product is -0 and every later term is a zero too
(the plants have zero entries), and the row kernel computes the structural zeros of U as zeros times ``A_k``
where the block kernel never writes over its zero fill.  :func:`same_bits` is that comparison."""
import collections
import functools

import numpy as np

import helpers
from helpers import LD
from oracle import qp_oracle as orc

QUAD, TINY, LTI, LTV_ROW, LTV_BLOCK, LTV_WAVE, LTV = 1, 2, 3, 4, 5, 6, 7       # capi.FILL_*
GENERIC, PAD, WHOLE = 1, 2, 4
KERNEL = {QUAD: "fill_lti_quad_kernel", TINY: "fill_lti_tiny_kernel", LTI: "fill_lti_kernel",
          LTV_ROW: "fill_ltv_row_kernel", LTV_BLOCK: "fill_ltv_block_kernel", LTV_WAVE: "fill_ltv_wave_kernel",
          LTV: "fill_ltv_kernel"}
LIMIT = "limit"
RHO = 1.3           # Perron root of the plants

Route = collections.namedtuple("Route", "kernel arg flags spw lshift")
Case = collections.namedtuple("Case", "name ltv batch N n m route off8")


def _c(name, ltv, batch, N, n, m, route, off8=None):
    return Case(name, ltv, batch, N, n, m, route if route is LIMIT else Route(*route),
                None if off8 is None else Route(*off8))


def _q(n, flags, spw, lshift):
    return (QUAD, n, flags, spw, lshift)


_T2, _L64 = (TINY, 0, 0, 2, 0), (LTI, 64, 0, 0, 0)
_LB, _LBP, _LBG = (LTI, 256, 0, 0, 0), (LTI, 256, PAD, 0, 0), (LTI, 256, GENERIC, 0, 0)
_B0 = (LTV_BLOCK, 0, 0, 0, 0)
_WAVE, _V64, _VB = (LTV_WAVE, 0, 0, 0, 0), (LTV, 64, 0, 0, 0), (LTV, 256, 0, 0, 0)


def _row(n):
    return (LTV_ROW, n, 0, 0, 0)


def _blk(n):
    return (LTV_BLOCK, n, 0, 0, 0)


CASES = [
    # ---- fill_lti_quad_kernel<1..4>: every lshift an NS can meet, at the smallest N (short rows: R = 64 >> lshift
    # rows per store, so the first of each NS are the "N < R" shapes)
    _c("quad1-ls0", 0, 3, 2, 1, 1, _q(1, 0, 1, 0), _T2),
    _c("quad1-ls1", 0, 3, 4, 1, 1, _q(1, 0, 1, 1), _T2),
    _c("quad1-ls2", 0, 3, 6, 1, 1, _q(1, 0, 1, 2), _T2),
    _c("quad1-ls3", 0, 3, 10, 1, 1, _q(1, 0, 1, 3), _T2),
    _c("quad1-ls4", 0, 3, 18, 1, 1, _q(1, 0, 1, 4), _T2),
    _c("quad1-ls5", 0, 3, 34, 1, 1, _q(1, 0, 1, 5), _T2),
    _c("quad1-ls6", 0, 3, 66, 1, 1, _q(1, 0, 1, 6), _T2),
    _c("quad2-ls0", 0, 3, 1, 2, 1, _q(2, 0, 1, 0), _T2),
    _c("quad2-ls1", 0, 3, 2, 2, 1, _q(2, 0, 1, 1), _T2),
    _c("quad2-ls2", 0, 3, 3, 2, 1, _q(2, 0, 1, 2), _T2),
    _c("quad2-ls3", 0, 3, 5, 2, 1, _q(2, 0, 1, 3), _T2),
    _c("quad2-ls4", 0, 3, 9, 2, 1, _q(2, 0, 1, 4), _T2),
    _c("quad2-ls5", 0, 3, 17, 2, 1, _q(2, 0, 1, 5), _T2),
    _c("quad2-ls6", 0, 3, 33, 2, 1, _q(2, 0, 1, 6), _T2),
    _c("quad3-ls2", 0, 3, 2, 3, 1, _q(3, 0, 1, 2), _T2),
    _c("quad3-ls3", 0, 3, 4, 3, 1, _q(3, 0, 1, 3), _T2),
    _c("quad3-ls4", 0, 3, 6, 3, 1, _q(3, 0, 1, 4), _T2),
    _c("quad3-ls5", 0, 3, 12, 3, 1, _q(3, 0, 1, 5), _T2),
    _c("quad3-ls6", 0, 3, 22, 3, 1, _q(3, 0, 1, 6), _T2),
    _c("quad4-ls1", 0, 3, 1, 4, 1, _q(4, 0, 1, 1), _T2),
    _c("quad4-ls2", 0, 3, 2, 4, 1, _q(4, 0, 1, 2), _T2),
    _c("quad4-ls3", 0, 3, 3, 4, 1, _q(4, 0, 1, 3), _T2),
    _c("quad4-ls4", 0, 3, 5, 4, 1, _q(4, 0, 1, 4), _T2),
    _c("quad4-ls5", 0, 3, 9, 4, 1, _q(4, 0, 1, 5), _T2),
    _c("quad4-ls6", 0, 3, 17, 4, 1, _q(4, 0, 1, 6), _T2),          # 34 words: longer than half a wavefront
    # ---- short rows: N a multiple of R (whole lines too), the tail group, the loop unrolled by four groups
    _c("quad2-N8-multiple", 0, 3, 8, 2, 1, _q(2, WHOLE, 1, 3), _T2),          # R = 8, one full group
    _c("quad2-N12-m3", 0, 3, 12, 2, 3, _q(2, 0, 1, 4), _T2),                  # R = 4, three full groups
    _c("quad1-N10-tail", 0, 3, 10, 1, 2, _q(1, 0, 1, 3), _T2),                # R = 8: one group and a tail of 2
    _c("quad4-N16-m2", 0, 3, 16, 4, 2, _q(4, WHOLE, 1, 5), _T2) ,             # R = 2: eight groups, two rounds of four
    _c("quad4-N15-tail", 0, 3, 15, 4, 1, _q(4, 0, 1, 5), _T2),                # R = 2: 4 + 3 groups and a tail
    _c("quad3-N20", 0, 3, 20, 3, 1, _q(3, 0, 1, 5), _T2),                     # R = 2, ten groups
    # ---- rows longer than a wavefront (more than 64 words), more than one round of stream_words (more than 256)
    _c("quad4-N33-m2", 0, 3, 33, 4, 2, _q(4, 0, 1, 6), _T2),
    _c("quad3-N100", 0, 3, 100, 3, 1, _q(3, 0, 1, 6), _L64),
    _c("quad4-N130", 0, 1, 130, 4, 1, _q(4, 0, 1, 6), _L64),
    # ---- several inputs, up to m + n = 16
    _c("quad4-m12", 0, 3, 6, 4, 12, _q(4, 0, 1, 4), _L64),
    _c("quad1-m15", 0, 3, 6, 1, 15, _q(1, 0, 1, 2), _T2),
    _c("quad3-m13", 0, 3, 6, 3, 13, _q(3, 0, 1, 4), _L64),
    # ---- more than 64 KB of LDS (the whole-LDS attribute)
    _c("quad4-N73-m12-lds", 0, 1, 73, 4, 12, _q(4, 0, 1, 6), _LB),
    # ---- several systems per wavefront, the batch no multiple of spw
    _c("quad1-spw2", 0, 16401, 2, 1, 1, _q(1, 0, 2, 0), (TINY, 0, 0, 8, 0)),
    _c("quad1-spw3", 0, 24581, 4, 1, 1, _q(1, 0, 3, 1), (TINY, 0, 0, 12, 0)),
    _c("quad1-spw4", 0, 32771, 2, 1, 1, _q(1, 0, 4, 0), (TINY, 0, 0, 16, 0)),
    _c("quad1-spw5", 0, 40961, 4, 1, 1, _q(1, 0, 5, 1), (TINY, 0, 0, 20, 0)),
    _c("quad1-spw6", 0, 49151, 2, 1, 1, _q(1, 0, 6, 0), (TINY, 0, 0, 24, 0)),
    _c("quad1-spw7", 0, 57341, 2, 1, 1, _q(1, 0, 7, 0), (TINY, 0, 0, 28, 0)),
    _c("quad1-spw8", 0, 65531, 2, 1, 1, _q(1, 0, 8, 0), (TINY, 0, 0, 32, 0)),
    _c("quad2-spw5", 0, 40961, 3, 2, 1, _q(2, 0, 5, 2), (TINY, 0, 0, 10, 0)),
    _c("quad2-m2-spw4", 0, 32771, 3, 2, 2, _q(2, 0, 4, 2), (TINY, 0, 0, 8, 0)),
    _c("quad3-spw4", 0, 32771, 2, 3, 1, _q(3, 0, 4, 2), (TINY, 0, 0, 5, 0)),
    _c("quad4-spw3", 0, 24581, 2, 4, 1, _q(4, 0, 3, 2), (TINY, 0, 0, 3, 0)),
    # ---- the 40 KB of LDS a wavefront may take lower spw (2 -> 1) under a batch that would allow 2
    _c("quad4-N54-m4-lds40", 0, 16385, 54, 4, 4, _q(4, 0, 1, 6), _L64),
    # ---- fill_lti_tiny_kernel: spw 2, a middle value, the most the shape allows; ragged last wavefront and
    # workgroup; n (m + n) = 12 and 30 leave idle lanes
    _c("tiny3-spw2", 0, 67, 5, 3, 1, _T2),
    _c("tiny3-spw3", 0, 6139, 5, 3, 1, (TINY, 0, 0, 3, 0)),
    _c("tiny3-spw5", 0, 10223, 5, 3, 1, (TINY, 0, 0, 5, 0)),
    _c("tiny1-spw32", 0, 65411, 5, 1, 1, (TINY, 0, 0, 32, 0)),
    _c("tiny5", 0, 3, 5, 5, 1, _T2),
    _c("tiny1-m20", 0, 5, 5, 1, 20, _T2),
    _c("tiny3-N1", 0, 3, 1, 3, 1, _T2),
    _c("tiny5-N2", 0, 3, 2, 5, 1, _T2),
    # ---- fill_lti_kernel<64, false>: four systems per workgroup
    _c("lti64-b1", 0, 1, 7, 5, 2, _L64),
    _c("lti64-b3", 0, 3, 7, 5, 2, _L64),
    _c("lti64-b4", 0, 4, 7, 5, 2, _L64),
    _c("lti64-b5", 0, 5, 7, 5, 2, _L64),
    _c("lti64-b67", 0, 67, 7, 5, 2, _L64),
    _c("lti64-even", 0, 3, 6, 8, 6, _L64),
    _c("lti64-N1", 0, 3, 1, 3, 8, _L64),
    _c("lti64-N2", 0, 3, 2, 5, 3, _L64),
    # ---- fill_lti_kernel<BLOCK, ...>: PAD, neither, GENERIC; each also beyond 64 KB
    _c("ltiB-pad", 0, 3, 5, 16, 1, _LBP, _LB),
    _c("ltiB-pad-N1", 0, 3, 1, 10, 16, _LBP, _LB),
    _c("ltiB-pad-N2", 0, 3, 2, 16, 1, _LBP, _LB),
    _c("ltiB-pad-lds", 0, 2, 5, 20, 30, _LBP, _LB),
    _c("ltiB", 0, 3, 5, 17, 1, _LB),
    _c("ltiB-11-13", 0, 3, 5, 11, 13, _LB),
    _c("ltiB-lds", 0, 2, 10, 20, 30, _LB),
    _c("ltiB-generic", 0, 3, 5, 32, 1, _LBG),
    _c("ltiB-generic-odd", 0, 2, 5, 33, 1, _LBG),
    _c("ltiB-generic-lds", 0, 2, 5, 40, 33, _LBG),
    # ---- fill_ltv_row_kernel<1..4>: the one-round-trip loop (one input, rows up to 256 words) and the other
    _c("row1", 1, 3, 6, 1, 1, _row(1), _B0),
    _c("row2", 1, 3, 5, 2, 1, _row(2), _blk(2)),
    _c("row3", 1, 3, 6, 3, 1, _row(3), _blk(3)),
    _c("row4", 1, 3, 5, 4, 1, _row(4), _blk(4)),
    _c("row1-m3", 1, 3, 6, 1, 3, _row(1), _B0),
    _c("row2-m2", 1, 3, 7, 2, 2, _row(2), _blk(2)),
    _c("row3-m2", 1, 3, 6, 3, 2, _row(3), _blk(3)),
    _c("row4-m16", 1, 3, 5, 4, 16, _row(4), _blk(4)),
    _c("row3-N100", 1, 3, 100, 3, 1, _row(3), _blk(3)),
    _c("row4-N130", 1, 2, 130, 4, 1, _row(4), _WAVE),
    _c("row2-N1", 1, 3, 1, 2, 1, _row(2), _blk(2)),
    _c("row3-N2", 1, 3, 2, 3, 1, _row(3), _blk(3)),
    # ---- fill_ltv_block_kernel<0, 2, 3, 4>: <2> and <4> only behind outputs 8 bytes off (rows above), <3> and
    # <0> at n = 1 with N n odd, <0> at n >= 5
    _c("block0-n1", 1, 3, 5, 1, 1, _B0),
    _c("block0-n1-m3", 1, 3, 7, 1, 3, _B0),
    _c("block3", 1, 3, 5, 3, 1, _blk(3)),
    _c("block3-m2", 1, 3, 7, 3, 2, _blk(3)),
    _c("block0-n5", 1, 3, 7, 5, 2, _B0),
    _c("block0-n6", 1, 3, 6, 6, 1, _B0),
    _c("block0-N1", 1, 3, 1, 5, 2, _B0),
    _c("block3-N1", 1, 3, 1, 3, 1, _blk(3)),
    # ---- fill_ltv_wave_kernel: four systems per workgroup
    _c("wave-b1", 1, 1, 15, 11, 1, _WAVE),
    _c("wave-b3", 1, 3, 15, 11, 1, _WAVE),
    _c("wave-b4", 1, 4, 15, 11, 1, _WAVE),
    _c("wave-b5", 1, 5, 15, 11, 1, _WAVE),
    _c("wave-b67", 1, 67, 15, 11, 1, _WAVE),
    _c("wave-n9-m3", 1, 3, 16, 9, 3, _WAVE),
    # ---- fill_ltv_kernel<64> and <BLOCK>
    _c("ltv64-b1", 1, 1, 6, 17, 1, _V64),
    _c("ltv64-b3", 1, 3, 6, 17, 1, _V64),
    _c("ltv64-b4", 1, 4, 6, 17, 1, _V64),
    _c("ltv64-b5", 1, 5, 6, 17, 1, _V64),
    _c("ltv64-b67", 1, 67, 6, 17, 1, _V64),
    _c("ltv64-N2", 1, 3, 2, 24, 2, _V64),
    _c("ltvB", 1, 3, 5, 25, 1, _VB),
    _c("ltvB-N1", 1, 3, 1, 24, 12, _VB),
    _c("ltvB-lds", 1, 2, 5, 48, 3, _VB),
    # ---- beyond a kernel limit: nothing is launched
    _c("limit-lti", 0, 3, 1, 70, 33, LIMIT),
    _c("limit-ltv", 1, 3, 1, 257, 1, LIMIT),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUN = [c for c in CASES if c.route is not LIMIT]
# instances of a batch beyond this are checked against the vectorised long-double recurrence; a sample of them
# (SAMPLE) against the oracle itself
SMALL_BATCH = 67
# "quad4-N54-m4-lds40" writes 6 GB, which no host reference can follow: its instances are copies of this many
# plants, instance b of plant b % 5.  The first five instances -- every plant -- are held to the oracle, and every
# other instance is compared with its original on the device, bit for bit: every system the launch writes is held
# to the bound through one of the two.
DISTINCT = {"quad4-N54-m4-lds40": 5}


def sample(case):
    """The instances of a large batch that are held to the oracle itself (every plant where plants repeat)."""
    if case.name in DISTINCT:
        return list(range(DISTINCT[case.name]))
    return sorted({0, case.batch // 2, case.batch - 1})


def same_bits(x, y):
    """Device tensors: equal bit for bit, except that +0 and -0 count as the same (see the module's docstring)."""
    import torch

    return bool(((x.view(torch.int64) == y.view(torch.int64)) | ((x == 0) & (y == 0))).all())


def kappa(case):
    return helpers.kappa(case.N, case.n)


# --------------------------------------------------------------------------------------------------
# inputs: plants free of cancellation (|A^k| = |A|^k), a plant of its own per instance
# --------------------------------------------------------------------------------------------------
def _scalar_plants(rng, batch, m, steps):
    """n = 1, where helpers.cancellation_free_plants leaves nothing to draw: a positive scalar up to the Perron
    root with sign flips, B as there."""
    A = rng.choice([-1.0, 1.0], (batch, steps, 1, 1)) * rng.uniform(0.4, RHO, (batch, steps, 1, 1))
    B = rng.standard_normal((batch, steps, 1, m)) * np.logspace(-2, 2, m)[None, None, None, :] \
        * 10.0 ** rng.uniform(-3, 3, (batch, 1, 1, 1))
    return A, B


@functools.lru_cache(maxsize=3)
def _inputs(ltv, batch, N, n, m):
    rng = np.random.default_rng([ltv, batch, N, n, m])
    if n == 1:
        A, B = _scalar_plants(rng, batch, m, N if ltv else 1)
        if not ltv:
            A, B = A[:, 0], B[:, 0]
        helpers.assert_cancellation_free(A, N, bool(ltv))
    else:
        A, B = helpers.cancellation_free_plants(rng, batch, n, m, RHO, N, per_step=bool(ltv),
                                                at_once=batch > SMALL_BATCH)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def inputs(case):
    """``(A, B)`` of the case, fp64: ``(batch, n, n)``, ``(batch, n, m)``; per step ``(batch, N, ...)``.  The
    same for every test that asks (and for a case's launches at both alignments); read-only."""
    if case.name in DISTINCT:
        A, B = _inputs(case.ltv, DISTINCT[case.name], case.N, case.n, case.m)
        idx = np.arange(case.batch) % DISTINCT[case.name]
        return A[idx], B[idx]
    return _inputs(case.ltv, case.batch, case.N, case.n, case.m)


# --------------------------------------------------------------------------------------------------
# references in long double: (x*, M) from the oracle on (A, B) and on (|A|, |B|)
# --------------------------------------------------------------------------------------------------
def oracle_pair(case, A, B, dtype=LD):
    """One instance: ``{"S": (S*, SM), "U": (U*, UM)}``, ``U`` stacked ``(m, N, N, n)``."""
    extend = orc.extend_matrices_ltv if case.ltv else orc.extend_matrices
    S1, U1 = extend(case.N, A, B, dtype=dtype)
    S2, U2 = extend(case.N, np.abs(A), np.abs(B), dtype=dtype)
    return {"S": (S1, S2), "U": (np.stack(U1), np.stack(U2))}


@functools.lru_cache(maxsize=3)
def _oracle(name):
    case = BY_NAME[name]
    A, B = inputs(case)
    which = range(case.batch) if case.batch <= SMALL_BATCH else sample(case)
    return {b: oracle_pair(case, A[b], B[b]) for b in which}


def oracle(case):
    """instance -> :func:`oracle_pair`, every instance of a batch up to SMALL_BATCH, else the sample; computed
    once, shared, not to be written to."""
    return _oracle(case.name)


def recurrence(A, B, N, dtype=LD):
    """The LTI recurrence over a whole batch at once, in ``dtype``: ``S (batch, N, n, n)``, ``U (batch, m, N, N, n)``."""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    batch, n, m = B.shape
    S = np.zeros((batch, N, n, n), dtype=dtype)
    U = np.zeros((batch, m, N, N, n), dtype=dtype)
    X, P = B, A
    for d in range(N):                                    # X = A^d B, P = A^{d+1}
        S[:, d] = P.transpose(0, 2, 1)
        for k in range(d, N):
            U[:, :, k, k - d, :] = X.transpose(0, 2, 1)
        X, P = np.matmul(A, X), np.matmul(A, P)
    return S, U


@functools.lru_cache(maxsize=1)
def _batch_reference(name):
    case = BY_NAME[name]
    A, B = inputs(case)
    S1, U1 = recurrence(A, B, case.N)
    S2, U2 = recurrence(np.abs(A), np.abs(B), case.N)
    return {"S": (S1, S2), "U": (U1, U2)}


def batch_reference(case):
    """The LTI recurrence in long double over the whole batch at once (the large batches: n <= 4, N <= 5):
    ``{"S": (S*, SM), "U": (U*, UM)}`` with the batch in front."""
    assert not case.ltv and case.batch > SMALL_BATCH and case.name not in DISTINCT
    return _batch_reference(case.name)
