"""The synthetic instances the tests of mpcasm_qp_polish_wide pose (numpy, built once, never changed): per shape
seven strictly complementary QPs of tests/polish_restatement.py's construction, seed ``[no, nc, na, 71]``.

The shapes are the edges of the kernel's loops -- one lane, fewer columns than lanes, 63 / 64 / 65 and 129 / 130
columns (one, two and three columns per lane), more rows than a wavefront's four in flight, no limits at all --
and C3's and C5's own; ``na < no`` throughout (at ``na = no`` ADMM's iterate can guess more active rows than
unknowns: skipped)."""
import functools

import numpy as np

import polish_restatement as pr

SHAPES = [(1, 1, 1), (5, 3, 2), (36, 76, 20), (63, 66, 20), (64, 70, 30), (65, 300, 40), (129, 140, 64),
          (130, 0, 0), (96, 196, 40), (200, 404, 60), (257, 260, 100)]          # (no, nc, na)
LARGEST = (512, 520, 100)            # three instances of it: two plain, one with a wrong active set
BOTH = [(5, 3, 2), (36, 76, 20), (65, 70, 33)]     # what mpcasm_qp_polish takes too
IDS = lambda shapes: ["%dx%d-na%d" % s for s in shapes]
PLAIN, WRONG, NAN, INFEASIBLE, UNSTATED = (0, 1, 2), 3, 4, 5, 6


@functools.lru_cache(maxsize=None)
def problem(no, nc, na, count=7):
    """``count`` complementary QPs of one shape: stacked ``P, q, G, h`` and the constructed active sets (the first
    ``count`` of the same stream, whatever ``count``)."""
    rng = np.random.default_rng([no, nc, na, 71])
    qps = [pr.complementary_qp(rng, no, nc, na) for _ in range(count)]
    return tuple(np.stack([qp[i] for qp in qps]) for i in (0, 1, 2, 3, 6))


def largest():
    """``LARGEST``: instances 0, 1 (plain) and 3 (to be given a wrong active set) of its stream."""
    full = problem(*LARGEST, count=4)
    return tuple(a[[0, 1, 3]] for a in full)
