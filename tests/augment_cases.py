"""Limits and costs on the true input of a pre-stabilised plan (csrc/feedback.hip: ``mpcasm_ltv_augment``,
``LtvLoop(feedback=, true_input=True)``), restated in numpy: the plant augmented by one delay, block by block; the
QP of ``problems.lipm_ltv_true_input`` built densely from the PLANT, without any augmentation; and the inputs of the
loop that test_ltv_augment_cpu.py and test_gpu_ltv_augment.py share."""
import numpy as np

import feedback_restatement as fr

# (n, m, T, batch) of the kernel's test: a single lane per region; the pendulum; m = n and m > n over many workgroups
# whose last wavefront is partly filled in every region (At: 5 x 67 x 16 = 5 360 = 83 x 64 + 48 elements and 7 x 130
# x 16 = 14 560 = 227 x 64 + 32; Bt and Kt: 2 680 = 41 x 64 + 56 and 10 920 = 170 x 64 + 40); a long sequence
SHAPES = [(1, 1, 1, 1), (3, 1, 18, 4), (2, 2, 5, 67), (1, 3, 7, 130), (3, 1, 60, 3)]
SEED = 23
GAINS = ["one", "per-instance", "per-step"]


def case(shape, gains, shared=False):
    """``A (batch, T, n, n), B (batch, T, n, m)`` (``shared``: without the batch) and ``K`` ``(m, n)``, ``(batch, m,
    n)`` or ``(batch, T, m, n)`` by ``gains``: normal draws, the same for every layout of a shape."""
    n, m, T, batch = shape
    rng = np.random.default_rng(SEED + 1000 * n + 100 * m + T)
    A, B = rng.standard_normal((batch, T, n, n)), rng.standard_normal((batch, T, n, m))
    K = rng.standard_normal((batch, T, m, n))
    if shared:
        A, B = A[0], B[0]
    return A, B, {"one": K[0, 0], "per-instance": K[:, 0], "per-step": K}[gains].copy()


def full_gain(K, T, batch):
    """``K`` of any layout as ``(batch, T, m, n)``."""
    K = K if K.ndim == 4 else K[:, None] if K.ndim == 3 else K[None, None]
    return np.broadcast_to(K, (batch, T) + K.shape[-2:])


def augmented(A, B, K):
    """``At (.., n + m, n + m), Bt (.., n + m, m), Kt (.., m, n + m)`` with the ``A + B K`` block LEFT ZERO: every
    element the kernel copies or sets -- ``[[0, 0], [K, 0]]``, ``[[B], [I]]``, ``[K | 0]`` -- in the dtype of the
    operands, over their leading axes."""
    n, m = B.shape[-2:]
    lead = np.broadcast_shapes(A.shape[:-2], B.shape[:-2], K.shape[:-2])
    A, B, K = (np.broadcast_to(v, lead + v.shape[-2:]) for v in (A, B, K))
    zero = lambda r, c: np.zeros(lead + (r, c), dtype=A.dtype)
    eye = np.broadcast_to(np.eye(m, dtype=A.dtype), lead + (m, m))
    At = np.concatenate([np.concatenate([zero(n, n), zero(n, m)], axis=-1),
                         np.concatenate([K, zero(m, m)], axis=-1)], axis=-2)
    return At, np.concatenate([B, eye], axis=-2), np.concatenate([K, zero(m, m)], axis=-1)


# --------------------------------------------------------------------------------------------------
# The QP of problems.lipm_ltv_true_input straight from the plant: no augmented matrix anywhere
# --------------------------------------------------------------------------------------------------
def dense_true_input_qp(A, B, K, given, omega=3.3445, target_vel=(0.3, 0.0), weights=(1e-3, 1e-2, 1.0),
                        input_limit=None):
    """``P, q`` and, with ``input_limit``, the limit's ``G, h`` (its ``4 N`` rows: upper and lower of x, upper and
    lower of y) of ONE instance from the plant's window ``A (N, 3, 3), B (N, 3, 1)`` and gains ``K (N, 1, 3)``:
    the states are rolled out over ``A + B K`` -- ``x_k = Xg_k x_0 + Xo_k v`` --, the true inputs are ``U = K X +
    I`` -- ``u_k = K_k x_k + v_k`` --, and the three costs of ``lipm_ltv`` are formed on them, the effort term
    ``w U^T U`` on the TRUE inputs.  ``given``: a row of the augmented plan's, ``[x_0 ; u_prev]`` per axis --
    ``u_prev`` is not read.  The unknowns are ``[v_x ; v_y]``."""
    N = A.shape[0]
    Xg, Xo = np.zeros((N + 1, 3, 3)), np.zeros((N + 1, 3, N))
    Xg[0] = np.eye(3)
    for k in range(N):
        Acl = A[k] + B[k] @ K[k]
        Xg[k + 1] = Acl @ Xg[k]
        Xo[k + 1] = Acl @ Xo[k]
        Xo[k + 1, :, k] += B[k][:, 0]
    Ug = np.stack([K[k, 0] @ Xg[k] for k in range(N)])
    Uo = np.stack([K[k, 0] @ Xo[k] for k in range(N)]) + np.eye(N)
    c_vel, c_cop = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, -1.0 / omega ** 2])
    rows = lambda c: (np.einsum("i,kij->kj", c, Xg[1:]), np.einsum("i,kij->kj", c, Xo[1:]))    # (row k: x_{k+1})
    terms = [(weights[0], Ug, Uo, (0.0, 0.0)), (weights[1],) + rows(c_vel) + (tuple(target_vel),),
             (weights[2],) + rows(c_cop) + ((0.0, 0.0),)]
    P, q = np.zeros((2 * N, 2 * N)), np.zeros(2 * N)
    G, h = [], []
    for a in range(2):
        x0, sl = given[4 * a:4 * a + 3], slice(a * N, (a + 1) * N)
        for w, Mg, Mo, aim in terms:
            P[sl, sl] += w * Mo.T @ Mo
            q[sl] += w * Mo.T @ (Mg @ x0 - aim[a])
        if input_limit is not None:
            for sign in (1.0, -1.0):
                block = np.zeros((N, 2 * N))
                block[:, sl] = sign * Uo
                G.append(block)
                h.append(input_limit - sign * (Ug @ x0))
    if input_limit is None:
        return P, q
    return P, q, np.vstack(G), np.concatenate(h)


# --------------------------------------------------------------------------------------------------
# The closed loop: lipm_ltv_true_input(N = 100, input_limit = 0.1), 4 instances on ltv_lipm_steps(N = 104, theta =
# 0.4 b) closed by the Riccati gains of lipm_feedback_weights, 3 ticks; the draw of rollout_cases.loop_inputs for the
# plant's states, the input slots zero
# --------------------------------------------------------------------------------------------------
LOOP_N, LOOP_T, LOOP_BATCH, LOOP_TICKS, LOOP_SEED, LOOP_LIMIT = 100, 104, 4, 3, 3, 0.1
# what test_ltv_augment_cpu.py confirms with the restatement: instances 0, 2 and 3 are SOLVED at every tick (in 25
# iterations at tick 0, the smallest margin of a verdict 0.109) with the limit active, max |u| of the plan 0.0999,
# 0.1001, 0.1001 where the unlimited plan reaches 0.131, 0.129, 0.169.  Instance 1 runs out of iterations at every
# tick with a margin of 0.027 -- too near a tie to hold the device to: it is reported, not asserted.
LOOP_ASSERTED = (0, 2, 3)
LOOP_STATUS = [[1, 1, 1]] * LOOP_TICKS             # of LOOP_ASSERTED
LOOP_TOL = 2e-3                                    # |u| <= limit (1 + 2 eps) at OSQP's eps = 1e-3
LOOP_UNLIMITED_EXCEEDS = 0.12


def loop_inputs(api, N=LOOP_N, T=LOOP_T, input_limit=LOOP_LIMIT):
    """``form, A_seq (B, T, 3, 3), B_seq (B, T, 3, 1), given (B, 8)``: the PLANT's sequences, the augmented plan's
    ``given``."""
    from mpcasm import problems

    form = problems.lipm_ltv_true_input(api, N=N, input_limit=input_limit)
    seqs = [problems.ltv_lipm_steps(api, N=T, theta=0.4 * b) for b in range(LOOP_BATCH)]
    draw = np.random.default_rng(LOOP_SEED).normal(0.0, 0.02, (LOOP_BATCH, 6))
    given = np.zeros((LOOP_BATCH, 8))
    given[:, 0:3], given[:, 4:7] = draw[:, 0:3], draw[:, 3:6]
    assert form.given_len == 8
    return form, np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs]), given


def loop_gains(A, B, dtype=float):
    """``K (B, T, 1, 3)``: the Riccati sweep of ``lipm_feedback_weights`` over every instance's whole sequence."""
    from mpcasm import problems

    Q, R = problems.lipm_feedback_weights()
    return np.stack([fr.lqr(A[b], B[b], Q, R, dtype=dtype)[0] for b in range(A.shape[0])])


def plan_inputs(plan, At, Bt, K, given, optim, dtype=float):
    """``(u, M)`` ``(axes, N, m)`` of one instance of the augmented plan (``fr.true_inputs`` with ``Kt = [K | 0]``)."""
    Kt = np.concatenate([K, np.zeros(K.shape[:-1] + (K.shape[-2],))], axis=-1)
    return fr.true_inputs(plan, At, Bt, Kt, given, optim, dtype=dtype)
