"""What the tests of the forward rollout of a plan compiled with ``ltv=`` share (csrc/rollout.hip:
``Assembler.rollout`` / ``advance``, ``mpcasm.ltv_loop.LtvLoop``): the shapes, the bound, the long-double
reference of the rows, the launch geometries, and the inputs and the CPU restatement of the closed loop -- used by
the CPU tests (test_ltv_rollout_cpu.py) and the GPU tests (test_gpu_ltv_rollout.py, test_gpu_ltv_rollout_variants.py,
test_gpu_ltv_loop.py)."""
import numpy as np

import sweep_cases as sc

# the shapes of the GPU test, by their names in sweep_cases: n = m = N = axes = 1; odd N with the 3 / 1 / 2 sizes;
# m > n; n = m = axes = 4; N past 128; the widest plan (N = 256, 1024 unknowns: the most LDS an instance takes)
# ... and, beside the issue's six, the plan that stages the most per instance (n = m = 4, N = 256 on one axis: 80 KB,
# past the 64 KB a workgroup gets without asking)
GPU_SHAPES = ["one-1-1-1", "lipm-33", "two-n1", "four-a4-n4", "lipm-129", "four-full", "wide-lds"]
EXTRA = {"wide-lds": sc.Shape("wide-lds", None, 4, 4, 256, 1, 0, False, False, 0, ())}
# the shapes whose row table the CPU test compiles beside lipm_ltv at N = 1, 2, 33
TABLE_SHAPES = ["one-1-1-1", "two-n1", "four-a4-n4", "desc"]

# every instantiation roll_chain<NS, MS> of the kernel's switch: n, m in 1 .. 4 at N = 5 on two axes (the second
# axis' columns of optim start behind the first's: non-zero ucol), no limits -- pmrows 42 .. 108, no = 10 m, ng = 2 n
NM_SHAPES = ["nm-%d-%d" % (n, m) for n in range(1, 5) for m in range(1, 5)]
EXTRA.update({"nm-%d-%d" % (n, m): sc.Shape("nm-%d-%d" % (n, m), None, n, m, 5, 2, 0, False, False, 0, ())
              for n in range(1, 5) for m in range(1, 5)})
NM_BATCH, NM_GIVEN_ROWS = 11, 14        # group 8: workgroups of 8 and 3; the advance by index into 14 rows

# What mpcasm_ltv_rollout_info answers for GPU_SHAPES at count >= 8 (test_ltv_rollout_cpu.py asserts it on the
# compiled plans): instances of a workgroup with the rows, LDS bytes an instance stages with the rows, instances of
# a workgroup of the advance.  Derived from roll_lds and the launch in csrc/rollout.hip, not from a run.
INFO = {"one-1-1-1": (8, 80, 8), "lipm-33": (8, 5360, 8), "two-n1": (8, 5232, 8), "four-a4-n4": (3, 17040, 8),
        "lipm-129": (2, 20720, 8), "four-full": (1, 57456, 8), "wide-lds": (1, 81968, 8)}
INFO_SHARED = {"lipm-33": 640}          # the bytes of a workgroup's shared part (the table's body, rowof) with the rows

# The launch geometries test_gpu_ltv_rollout_variants.py runs the rows at: (shape, batch, {count: the live instances
# of every workgroup}).  The splits are the claim of each case -- the GPU test holds Assembler.rollout_info to them
# before it launches, the CPU test the entry on the compiled plan.
GEOMETRY = [
    # group 8: tails of 4 and 1 behind two full workgroups; exactly two, one past one, exactly one, one short, one
    ("lipm-33", 20, {20: (8, 8, 4), 17: (8, 8, 1), 16: (8, 8), 9: (8, 1), 8: (8,), 7: (7,), 1: (1,)}),
    # an odd group, inst0 = 3: tails of 1 and 2
    ("four-a4-n4", 7, {7: (3, 3, 1), 6: (3, 3), 5: (3, 2)}),
    # three workgroups of a group of 2
    ("lipm-129", 5, {5: (2, 2, 1), 4: (2, 2)}),
    # odd pmrows = 5, no = 1, a 1-double plant: every second instance's rows, optim, A and B start on an odd double
    ("one-1-1-1", 19, {19: (8, 8, 3), 9: (8, 1)}),
]
ODD_START = [("lipm-33", 20, 17), ("one-1-1-1", 19, 19)]      # (shape, batch, count) of the runs 8 bytes off
MISSING = ("lipm-33", 20, 17, 23, (8, 9, 16))     # ..., rows of given, the instances whose index points outside it
ADVANCE = ("lipm-33", 20, 25, {20: (8, 8, 4), 17: (8, 8, 1), 9: (8, 1)})      # ..., rows of given, the advance's splits


def kappa_rollout(N, n, m):
    """The depth of a row of the rollout in roundings, for helpers.assert_componentwise: a state of step k + 1
    is the end of k + 1 <= N inner products of length n + m, one per step (x_{j+1} = A_j x_j + B_j u_j: n
    products with the states, m with the inputs, summed), each of which adds at most n + m roundings to what its
    operands carry -- N (n + m) in all; a row is then one inner product of length n with c: n more.  Doubled, as
    helpers.kappa is: the bound ``gamma_k = k u / (1 - k u)`` and the products' own roundings are covered by a
    factor of 2 for every k in reach, and the reference itself is rounded to long double.  So
    ``kappa_rollout = 2 (N (n + m) + n)``; measured with plain numpy in fp64 on lipm_ltv with the plants of
    sweep_cases.plants: within 1.2, 1.6, 8.5, 12.9, 13.1 u M at N = 1, 2, 33, 100, 256, where the bound is 14, 22,
    270, 806, 2 054."""
    return 2 * (N * (n + m) + n)


def shape_of(name):
    return EXTRA[name] if name in EXTRA else sc.BY_NAME[name].shape


def reference_rows(form, name, A, B, given, optim, plan):
    """``(x*, M)`` of the preview rows ``Mg given + Mo optim`` of one instance in long double, rows in the plan's
    order: helpers.precise_reference(..., ltv=True) where that is affordable and the formulation has limits
    (it assembles the whole QP on the way), else the same sums of the oracle without ``P, q, G, h`` -- the pattern
    of sweep_cases.reference: ``extend_matrices_ltv`` in long double, ``preview_matrices``, ``preview``, once plain
    and once with magnitudes."""
    from helpers import LD, precise_reference
    from oracle import qp_oracle as orc

    if plan.no < 256 and orc.all_limits(form):
        return precise_reference(form, name, A, B, given, ltv=True, optim=optim, pm_rows=plan.pm_rows)["rows"]
    dyn = form.dynamics[name]
    N = dyn.matrices[-1].shape[0]
    g = np.asarray(given, dtype=float).reshape(-1, 1)
    x = np.asarray(optim, dtype=float).reshape(-1, 1)
    out, saved = [], list(dyn.matrices)
    try:
        for magnitude in (False, True):
            S, U = orc.extend_matrices_ltv(N, np.abs(A) if magnitude else A, np.abs(B) if magnitude else B, dtype=LD)
            dyn.matrices = list(U) + [S]
            dyn.update_definitions()
            PM = orc.preview_matrices(form, dtype=LD, magnitude=magnitude)
            rows = np.zeros(plan.pmrows, dtype=LD)
            for var, (r0, n) in plan.pm_rows.items():
                rows[r0:r0 + n] = orc.preview(PM, g, x, var, dtype=LD, magnitude=magnitude).ravel()
            out.append(rows)
    finally:
        dyn.matrices = saved
        dyn.update_definitions()
    return tuple(out)


def next_given_reference(plan, rows):
    """``(x*, M)`` of the next given from the pair ``rows`` of :func:`reference_rows`: column c of ``given`` is
    state i of an axis, and its next value that state's first sample -- the row the plan's table gives it."""
    from mpcasm.plan import ROLL_STATE, rollout_rows

    recs, cvec = rollout_rows(plan)
    sw = plan.sweep
    first = {}
    for kind, row0, count, axis, k0, kstep, cv, _ in recs:
        c = cvec[cv]
        if kind == ROLL_STATE and k0 == 0 and np.count_nonzero(c) == 1 and c[np.argmax(c != 0)] == 1.0:
            first.setdefault((int(axis), int(np.argmax(c != 0))), int(row0))
    take = np.zeros(plan.ng, dtype=np.int64)
    for a in range(sw["axes"].shape[0]):
        for i in range(sw["n"]):
            take[sw["axes"][a, 0] + i] = first[(a, i)]
    return rows[0][take], rows[1][take]


# --------------------------------------------------------------------------------------------------
# The closed loop: lipm_ltv(N = 12), 4 instances, 6 ticks; instance b follows ltv_lipm_steps(N = 18,
# theta = 0.4 b), so tick t plans over its steps [t, t + 12)
# --------------------------------------------------------------------------------------------------
LOOP_N, LOOP_T, LOOP_BATCH, LOOP_TICKS, LOOP_SEED = 12, 18, 4, 6, 3
# what these inputs were chosen for (test_ltv_rollout_cpu.py confirms it with the restatement): instance 1 is
# primal infeasible at every tick -- it is held -- and the others are solved at every tick
LOOP_STATUS = {0: 1, 1: -3, 2: 1, 3: 1}


def loop_inputs(api):
    """``form, A_seq (B, T, n, n), B_seq (B, T, n, m), given (B, ng)`` of the loop tests."""
    from mpcasm import problems

    form = problems.lipm_ltv(api, N=LOOP_N)
    seqs = [problems.ltv_lipm_steps(api, N=LOOP_T, theta=0.4 * b) for b in range(LOOP_BATCH)]
    A = np.stack([s[0] for s in seqs])
    B = np.stack([s[1] for s in seqs])
    given = np.random.default_rng(LOOP_SEED).normal(0.0, 0.02, [LOOP_BATCH, form.given_len])
    return form, A, B, given


def window_qp(form, name, A, B, given):
    """``P, q, G, h`` (fp64) of one instance on the per-step plant ``A (N, n, n), B (N, n, m)``: the oracle's
    assembly on the oracle's horizon matrices."""
    from oracle import qp_oracle as orc

    dyn = form.dynamics[name]
    N = dyn.matrices[-1].shape[0]
    saved = list(dyn.matrices)
    try:
        S, U = orc.extend_matrices_ltv(N, A, B)
        dyn.matrices = list(U) + [S]
        dyn.update_definitions()
        G, h, P, q = orc.assemble(form, np.asarray(given, dtype=float).reshape(-1, 1))
    finally:
        dyn.matrices = saved
        dyn.update_definitions()
    return np.asarray(P), np.asarray(q).ravel(), np.asarray(G), np.asarray(h).ravel()


def first_step(plan, A0, B0, given, optim):
    """``x_1 = A_0 x_0 + B_0 u_0`` of every axis in fp64, laid out as a row of ``given``."""
    sw = plan.sweep
    out = np.array(given)
    for a in range(sw["axes"].shape[0]):
        c0 = int(sw["axes"][a, 0])
        u0 = np.array([optim[int(sw["axes"][a, 1 + j])] for j in range(sw["m"])])
        out[c0:c0 + sw["n"]] = A0 @ given[c0:c0 + sw["n"]] + B0 @ u0
    return out


def first_step_reference(plan, A0, B0, given, optim):
    """``(x*, M)`` of :func:`first_step` in long double: ``A_0 x_0 + B_0 u_0`` and ``|A_0| |x_0| + |B_0| |u_0|``."""
    from helpers import LD

    pair = []
    for mag in (False, True):
        f = (lambda v: np.abs(np.asarray(v, dtype=LD))) if mag else (lambda v: np.asarray(v, dtype=LD))
        pair.append(first_step(plan, f(A0), f(B0), f(given), f(optim)))
    return tuple(pair)


def applies(status, on_unsolved):
    """WalkerFleet's rule: 'hold' applies solved and out-of-iterations results, 'apply' all but NaN ones."""
    return status in ((1, -2) if on_unsolved == "hold" else (1, -2, -3, -4))


def restated_loop(api, plan, form, A, B, given, ticks=LOOP_TICKS, on_unsolved="hold", **solver):
    """The loop on the CPU: per tick and instance the oracle's assembly on the window, osqp_restatement.solve
    (cold, OSQP's defaults), ``x_1`` where the status applies.  Returns ``status (ticks, B)``, ``given (ticks + 1,
    B, ng)`` and the smallest margin of any verdict."""
    import osqp_restatement as osqp

    batch, N = given.shape[0], plan.sweep["N"]
    trail, status, margin = [np.array(given, dtype=float)], np.zeros((ticks, batch), dtype=np.int64), np.inf
    for t in range(ticks):
        nxt = trail[-1].copy()
        for b in range(batch):
            P, q, G, h = window_qp(form, "LIP", A[b, t:t + N], B[b, t:t + N], trail[-1][b])
            sol = osqp.solve(P, q, G, h, **solver)
            status[t, b], margin = sol.status, min(margin, sol.margin)
            if applies(sol.status, on_unsolved):
                nxt[b] = first_step(plan, A[b, t], B[b, t], trail[-1][b], sol.x)
        trail.append(nxt)
    return status, np.stack(trail), margin
