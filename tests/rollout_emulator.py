"""numpy emulator of csrc/rollout.hip -- TEST INFRASTRUCTURE ONLY: it walks the very words of a row table
(``mpcasm_ltv_rollout_compile``: header, records, combinations) and runs the kernel's recursion in fp64, so that
the table and the arithmetic can be held to the reference without a device."""
import numpy as np

HDR = 12                      # header words: magic, n, m, N, axes, preview rows, ng, no, records, combinations, 0, 0
MAGIC = 0x4C4F5231
REC_WORDS, NMAX = 8, 4
GIVEN, OPTIM, STATE = 0, 1, 2


def parse(words):
    """``(sizes dict, records (nrec, 8), cvec (ncvec, 4))`` of a table's words."""
    words = np.asarray(words, dtype=np.int32)
    assert words[0] == MAGIC and words.size >= HDR
    names = ("n", "m", "N", "axes", "pmrows", "ng", "no", "nrec", "ncvec")
    sizes = {k: int(v) for k, v in zip(names, words[1:10])}
    nrec, ncvec = sizes["nrec"], sizes["ncvec"]
    assert words.size == HDR + REC_WORDS * nrec + 2 * NMAX * ncvec
    recs = words[HDR:HDR + REC_WORDS * nrec].reshape(nrec, REC_WORDS)
    cvec = words[HDR + REC_WORDS * nrec:].copy().view(np.float64).reshape(ncvec, NMAX)
    return sizes, recs, cvec


def trajectory(axes, n, m, A, B, given, optim):
    """``x[a, k] = x_{k+1}`` of axis a: ``x_{k+1} = A_k x_k + B_k u_k`` in fp64, from the axis' columns
    (``axes[a] = (given column of its initial state, first unknown of input j ...)``)."""
    N = A.shape[0]
    traj = np.zeros((len(axes), N, n))
    for a, rec in enumerate(axes):
        x = np.array(given[rec[0]:rec[0] + n], dtype=np.float64)
        for k in range(N):
            u = np.array([optim[rec[1 + j] + k] for j in range(m)], dtype=np.float64)
            x = A[k] @ x + B[k] @ u
            traj[a, k] = x
    return traj


def rollout(words, axes, A, B, given, optim):
    """The rows of one instance, as the kernel forms them from the table."""
    sizes, recs, cvec = parse(words)
    n, m = sizes["n"], sizes["m"]
    traj = trajectory(axes, n, m, np.asarray(A), np.asarray(B), given, optim)
    out = np.full(sizes["pmrows"], np.nan)
    for kind, row0, count, axis, k0, kstep, cv, _ in recs:
        for i in range(count):
            k = k0 + i * kstep
            assert np.isnan(out[row0 + i]), "row %d written twice" % (row0 + i)
            if kind == GIVEN:
                out[row0 + i] = given[k]
            elif kind == OPTIM:
                out[row0 + i] = optim[k]
            else:
                assert kind == STATE
                out[row0 + i] = cvec[cv, :n] @ traj[axis, k]
    return out
