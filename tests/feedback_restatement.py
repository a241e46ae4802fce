"""Pre-stabilised prediction, restated in numpy (csrc/feedback.hip: ``mpcasm_ltv_lqr``, ``mpcasm_ltv_close``,
``mpcasm_ltv_true_inputs``): the backward Riccati sweep over one instance's ``(A_k, B_k)``, the closed-loop
matrices ``A_k + B_k K_k`` and the true inputs ``u_k = K_k x_k + v_k`` of a plan whose unknowns are ``v``.  Every
function takes ``dtype``: ``float`` restates the kernel, ``helpers.LD`` is the reference it is held to -- nothing
below calls LAPACK (numpy's is fp64 only), so long double is really used: the products are numpy's own loops on
the dtype of their operands, the Cholesky and the triangular solves are written out."""
import numpy as np


def cholesky(S):
    """``(L, j)``: the lower factor of ``S = L L^T`` by columns in ``S``'s dtype, ``j = -1``; or ``j`` the first
    column whose pivot is not positive (NaN included), ``L`` then unfinished."""
    m = S.shape[0]
    L = np.zeros_like(S)
    for j in range(m):
        d = S[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0:
            return L, j
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            L[i, j] = (S[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L, -1


def solve_spd(L, W):
    """``(L L^T)^-1 W`` by the two triangular solves, column by column."""
    m = L.shape[0]
    Y = np.zeros_like(W)
    for i in range(m):
        Y[i] = (W[i] - (L[i, :i, None] * Y[:i]).sum(axis=0)) / L[i, i]
    X = np.zeros_like(W)
    for i in range(m - 1, -1, -1):
        X[i] = (Y[i] - (L[i + 1:, i, None] * X[i + 1:]).sum(axis=0)) / L[i, i]
    return X


def lqr(A, B, Q, R, terminal=None, dtype=float):
    """``K (T, m, n), A_cl (T, n, n), info`` of one instance ``A (T, n, n), B (T, n, m)``: for k = T - 1 .. 0

        1. S = R + B_k^T P B_k        (the upper triangle, mirrored)
        2. S = L L^T
        3. K_k = -S^-1 (B_k^T P A_k)  (the two triangular solves)
        4. A_cl_k = A_k + B_k K_k
        5. P <- Q + A_k^T (P A_cl_k)
        6. P <- (P + P^T) / 2

    from ``P = terminal`` (default ``Q``).  ``info``: -1, or the step whose pivot was not positive -- the rows of
    that step and of every earlier one are NaN, the later ones stand."""
    f = lambda v: np.array(v, dtype=dtype)
    A, B, Q, R = f(A), f(B), f(Q), f(R)
    T, n, m = A.shape[0], A.shape[1], B.shape[2]
    P = f(Q if terminal is None else terminal)
    K, Acl = np.full((T, m, n), np.nan, dtype=dtype), np.full((T, n, n), np.nan, dtype=dtype)
    for k in range(T - 1, -1, -1):
        PB = P @ B[k]
        S = np.triu(R + B[k].T @ PB)
        S = S + np.triu(S, 1).T
        L, bad = cholesky(S)
        if bad >= 0:
            return K, Acl, k
        K[k] = -solve_spd(L, PB.T @ A[k])
        Acl[k] = A[k] + B[k] @ K[k]
        P = Q + A[k].T @ (P @ Acl[k])
        P = (P + P.T) / 2
    return K, Acl, -1


def close(A, B, K, dtype=float, magnitude=False):
    """``A + B K`` over the leading axes (``K`` broadcast against them); ``magnitude``: ``|A| + |B| |K|``."""
    f = (lambda v: np.abs(np.asarray(v, dtype=dtype))) if magnitude else (lambda v: np.asarray(v, dtype=dtype))
    return f(A) + f(B) @ f(K)


def true_inputs(plan, Acl, B, K, given, optim, dtype=float):
    """``(u, M)`` of one instance, each ``(axes, N, m)``: along ``x_{k+1} = A_cl_k x_k + B_k v_k`` from the axis'
    initial state in ``given``, with ``v`` the axis' unknowns in ``optim``, ``u_k = K_k x_k + v_k``; ``M`` the same
    sums over the absolute values of every datum (as rollout_cases.first_step_reference's)."""
    sw = plan.sweep
    n, m, N, axes = sw["n"], sw["m"], sw["N"], sw["axes"]
    pair = []
    for mag in (False, True):
        f = (lambda v: np.abs(np.asarray(v, dtype=dtype))) if mag else (lambda v: np.asarray(v, dtype=dtype))
        a_, b_, k_, g_, o_ = f(Acl), f(B), f(K), f(given), f(optim)
        u = np.zeros((axes.shape[0], N, m), dtype=dtype)
        for a in range(axes.shape[0]):
            c0 = int(axes[a, 0])
            x = g_[c0:c0 + n].copy()
            for k in range(N):
                v = np.array([o_[int(axes[a, 1 + j]) + k] for j in range(m)], dtype=dtype)
                u[a, k] = k_[k] @ x + v
                x = a_[k] @ x + b_[k] @ v
        pair.append(u)
    return tuple(pair)


# --------------------------------------------------------------------------------------------------
# The cases test_ltv_feedback_cpu.py and test_gpu_ltv_feedback.py share
# --------------------------------------------------------------------------------------------------
# (n, m, T, batch) of the Riccati sweep: the smallest; the pendulum; n = m = 4 on two wavefronts, the second
# partly filled; m > n on three; a long chain
RICCATI_SHAPES = [(1, 1, 1, 1), (3, 1, 18, 4), (4, 4, 5, 67), (2, 3, 7, 130), (4, 2, 60, 3)]
RICCATI_SEED = 17


def riccati_case(api, shape):
    """``A (batch, T, n, n), B (batch, T, n, m), Q, R``: the pendulum's sequences (``ltv_lipm_steps`` at ``theta =
    0.4 b``) with ``lipm_feedback_weights`` for ``(3, 1, 18, 4)``; else random plants, every step scaled to a
    spectral radius drawn from 1.3 .. 1.4, with ``Q = G G^T + 1e-3 I`` and ``R = H H^T + 1e-2 I``."""
    from mpcasm import problems

    n, m, T, batch = shape
    if shape == (3, 1, 18, 4):
        seqs = [problems.ltv_lipm_steps(api, N=T, theta=0.4 * b) for b in range(batch)]
        return (np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs])) + problems.lipm_feedback_weights()
    rng = np.random.default_rng(RICCATI_SEED + 100 * n + 10 * m + T)
    A = rng.standard_normal((batch, T, n, n))
    radius = np.abs(np.linalg.eigvals(A)).max(axis=-1)
    A *= (rng.uniform(1.3, 1.4, (batch, T)) / radius)[..., None, None]
    B = rng.standard_normal((batch, T, n, m))
    G, H = rng.standard_normal((n, n)), rng.standard_normal((m, m))
    return A, B, G @ G.T + 1e-3 * np.eye(n), H @ H.T + 1e-2 * np.eye(m)


def gain_errors(K, K_ref):
    """``|K - K*|`` of every element relative to its step's largest ``|K*|``, in units of u: ``(.., T, m, n)``."""
    from helpers import LD, U64

    scale = np.abs(K_ref).max(axis=(-2, -1), keepdims=True)
    return np.asarray(np.abs(np.asarray(K, dtype=LD) - K_ref) / scale / LD(U64), dtype=float)


# The closed loop at the size it was built for: lipm_ltv(N = 100), 4 instances on ltv_lipm_steps(N = 104, theta =
# 0.4 b), 3 ticks; rollout_cases.loop_inputs' draw of `given`, row 1 eight times as far out -- instance 1 is primal
# infeasible (held) and the others solved at every tick with the feedback of lipm_feedback_weights, and WITHOUT it
# every instance is NON_CVX at every tick (test_ltv_feedback_cpu.py confirms both with the restatement)
C5_N, C5_T, C5_BATCH, C5_TICKS, C5_SEED = 100, 104, 4, 3, 3
C5_STATUS = [[1, -3, 1, 1]] * C5_TICKS
C5_OPEN_STATUS = [[-7] * C5_BATCH] * C5_TICKS


def c5_loop_inputs(api):
    """``form, A_seq (B, T, n, n), B_seq (B, T, n, m), given (B, ng)``."""
    from mpcasm import problems

    form = problems.lipm_ltv(api, N=C5_N)
    seqs = [problems.ltv_lipm_steps(api, N=C5_T, theta=0.4 * b) for b in range(C5_BATCH)]
    given = np.random.default_rng(C5_SEED).normal(0.0, 0.02, [C5_BATCH, form.given_len])
    given[1] *= 8
    return form, np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs]), given
