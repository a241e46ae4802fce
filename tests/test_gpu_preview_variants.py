"""GPU: every kernel variant of f2 (csrc/preview.hip) element by element against extended precision.

The family of preview_cases.py reaches every instantiation launch_preview_or_goals can select
(test_preview_routes_cpu.py holds it to that); here each case first asserts that the library takes the route
its id names (Assembler.preview_route, the launch's own decision), then launches it into NaN-filled buffers
at the edges of the launch geometry -- the whole batch, the partial last block of four (count = B - 1, B - 2,
B - 3), 1, 3, 4 and 5 instances -- with every instance's own given, solver answer, cost aims and, where the
case has them, plant.  Rows are held to |x - x*| <= kappa (u M + 2^-1022) (helpers.assert_componentwise),
structural zeros to exact zeros, distances to (2 kappa + rows + 4) u sum_r (M_r + |aim|)^2.  Cases whose
streams the batch shares run twice: as they are (the blocked kernel) and with MPCASM_PREVIEW_NO_BLOCKS=1 (the
staged kernel with no stream of an instance's own)."""
import zlib

import numpy as np
import pytest

import preview_cases as pc
from helpers import LD, assert_componentwise, cancellation_free_plants, kappa

pytestmark = pytest.mark.gpu

SAMPLES = (0, 1, 63, 64, 255, 256)
ALL_UP_TO = 64            # batches up to this size are checked whole
NUM_CUS_8X = 8            # (the staged kernel: at most 8 instances per workgroup decide the grid)


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _runs():
    for case in pc.CASES:
        yield case, False
        if case.rows[0] == pc.BLOCKED:
            yield case, True


def _id(case, no_blocks):
    return "%s-%s" % (case.shape.name, pc.route_id(case.no_blocks if no_blocks else case.rows))


def _counts(B):
    return sorted({c for c in (B, B - 1, B - 2, B - 3, 1, 3, 4, 5) if 1 <= c <= B}, reverse=True)


def _samples(B, counts):
    """The first and last instance of the batch and of the blocks of four around every count, SAMPLES."""
    if B <= ALL_UP_TO:
        return list(range(B))
    picked = {0, B - 1} | {b for b in SAMPLES if b < B}
    for c in counts:
        i0 = 4 * ((c - 1) // 4)
        picked |= {b for b in (i0 - 4, i0 - 1, i0, c - 1) if 0 <= b < B}
    return sorted(picked)


def _fused_status(torch, asm, form, g, x, out, count):
    """mpcasm_preview_goal_distance itself (Assembler.full_goal_distances hides MPCASM_ERR_LIMIT behind its
    fallback): the status it returns."""
    from mpcasm import capi, engine

    table, names = asm.goal_terms(form)
    ptrs, strides = asm._src_args()
    work = asm._workspace()
    with torch.cuda.device(asm.device):
        return capi.load().mpcasm_preview_goal_distance(
            asm._handle, ptrs, strides, g.data_ptr(), x.data_ptr(), asm.params.data_ptr(), table.data_ptr(),
            table.shape[0], len(names), out.data_ptr(), work.data_ptr(), count, engine._stream_handle(torch, None))


@pytest.mark.parametrize("case,no_blocks", list(_runs()), ids=[_id(*r) for r in _runs()])
def test_variant(gpu_api, torch_gpu, monkeypatch, case, no_blocks):
    torch = torch_gpu
    from mpcasm import capi, engine, problems

    sh = case.shape
    n, m, N, B = sh.n, sh.m, sh.N, sh.batches[0]
    if no_blocks:
        monkeypatch.setenv("MPCASM_PREVIEW_NO_BLOCKS", "1")      # (the launch reads it per call)
    else:
        monkeypatch.delenv("MPCASM_PREVIEW_NO_BLOCKS", raising=False)
    rng = np.random.default_rng(zlib.crc32(sh.name.encode()))
    f64 = dict(dtype=torch.float64, device="cuda")
    nan = lambda *shape: torch.full(shape, float("nan"), **f64)

    # ---- the instances: plants, given, solver answers, aims
    A = Bm = S = U = None
    if sh.streams == "lti":        # growing, badly scaled plants free of cancellation: M tracks the results
        A, Bm = cancellation_free_plants(rng, B, n, m, 1.3, N)
    elif sh.streams == "bound":
        A, Bm = (np.stack(z) for z in zip(*(problems.random_lti_matrices(rng, n, m) for _ in range(B))))
    form = pc.build(gpu_api, rng, sh, plant=None if A is None else (A[0], Bm[0]))
    asm = engine.Assembler(form, batch=B, lti=["plant"] if sh.streams == "lti" else ())
    if sh.streams == "lti":
        asm.bind_lti("plant", torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"))
    elif sh.streams == "bound":
        S, U = engine.fill_su(torch.as_tensor(A, device="cuda"), torch.as_tensor(Bm, device="cuda"), N)
        for j in range(m):
            asm.bind_source(("plant", j), U[:, j])
        asm.bind_source(("plant", m), S)
    plan = asm.plan
    W, pmrows = plan.ng + plan.no, plan.pmrows
    given, optim = rng.normal(0, 0.3, [B, plan.ng]), rng.normal(0, 0.5, [B, plan.no])
    params = asm.params.cpu().numpy().copy()
    for (kind, name, field), (start, rows, cols) in plan.param_slots.items():
        if kind == "cost" and field == "aim":
            params[:, start:start + rows * cols] += rng.normal(0, 0.5, [B, rows * cols])
    asm.params.copy_(torch.as_tensor(params, device="cuda"))
    gt, xt = torch.as_tensor(given, device="cuda"), torch.as_tensor(optim, device="cuda")
    table, ngoals = pc.goal_table(form, plan)
    assert np.array_equal(asm.goal_terms(form)[0].cpu().numpy(), table)

    # ---- the route: what the id names, from the launch's own decision
    want_rows = case.no_blocks if no_blocks else case.rows
    want_dist = None if no_blocks else case.dist
    route = asm.preview_route()
    assert pc.route_key(route) == want_rows, pc.route_id(pc.route_key(route))
    assert pc.route_key(asm.preview_route(goals=form)) == want_dist
    if sh.name == "own-e32-bound-56kb":          # more than 8 x the grid: the prefetch goes round more than once
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        grid = cus * max(1, min(8, (160 * 1024) // route[6]))
        assert B > NUM_CUS_8X * grid, (B, grid)

    # ---- references of the sampled instances
    counts = _counts(B)
    picked = _samples(B, counts)
    ref = {}
    if sh.streams == "lti":
        kap = kappa(N, n)
        for b in picked:
            ref[b] = pc.generated_rows_reference(form, "plant", A[b], Bm[b], given[b], optim[b], plan)
    else:
        kap = W + pc.longest_definition_row(sh) + 2
        if sh.streams == "shared":
            x, mag = pc.dense_rows_reference(pc.dense_matrix(form, plan), given[picked], optim[picked])
            ref = {b: (x[i], mag[i]) for i, b in enumerate(picked)}
        else:                          # the fp64 S, U the kernel read, instance by instance
            dyn = form.dynamics["plant"]
            saved = list(dyn.matrices)
            try:
                for b in picked:
                    dyn.matrices = [U[b, j].cpu().numpy() for j in range(m)] + [S[b].cpu().numpy()]
                    dyn.update_definitions()
                    x, mag = pc.dense_rows_reference(pc.dense_matrix(form, plan), given[b:b + 1], optim[b:b + 1])
                    ref[b] = (x[0], mag[0])
            finally:
                dyn.matrices = saved
                dyn.update_definitions()
    dref = {b: pc.distance_reference(table, ngoals, ref[b][0], ref[b][1], params[b], kap) for b in picked}

    # ---- launches
    worst = dict(rows=0.0, fused=0.0, two_step=0.0, between=0.0)

    def check_distances(D, count, key, what):
        assert np.isnan(D[count:]).all(), "%s, count %d: distances past count written" % (what, count)
        for b in (b for b in picked if b < count):
            d, bound = dref[b]
            err = np.abs(D[b].astype(LD) - d)
            assert np.isfinite(D[b]).all() and (err <= bound).all(), \
                "%s, count %d, instance %d: %r, d* = %r, bound %r" % (what, count, b, D[b], d.astype(float), bound.astype(float))
            worst[key] = max(worst[key], float(np.max(err / np.where(bound > 0, bound, 1))))

    for count in counts:
        what = "%s, count %d" % (_id(case, no_blocks), count)
        out = nan(B, pmrows)
        assert asm.preview_rows(gt, xt, out=out, count=count) is out
        R = out.cpu().numpy()
        assert np.isnan(R[count:]).all(), "%s: rows past count written" % what
        for b in (b for b in picked if b < count):
            worst["rows"] = max(worst["rows"], assert_componentwise(R[b], ref[b][0], ref[b][1], kap,
                                                                    "%s, instance %d" % (what, b)))
        # the distances: from the rows, and straight from the sources (fused where the route says so)
        two = asm.goal_distance(form, out, out=nan(B, ngoals), count=count).cpu().numpy()
        check_distances(two, count, "two_step", "goal_distance")
        raw = nan(B, ngoals)
        status = _fused_status(torch, asm, form, gt, xt, raw, count)
        if want_dist is None:        # the fallback is what ran, and nothing was written on the way to it
            assert status == capi.ERR_LIMIT and torch.isnan(raw).all(), (status, what)
        else:
            assert status == capi.OK, (status, what)
            check_distances(raw.cpu().numpy(), count, "fused", "mpcasm_preview_goal_distance")
        full = asm.full_goal_distances(form, gt, xt, out=nan(B, ngoals), count=count).cpu().numpy()
        check_distances(full, count, "fused" if want_dist is not None else "two_step", "full_goal_distances")
        if want_dist is not None:    # fused against two-step, instance by instance, to the same bound
            assert np.array_equal(full[:count], raw.cpu().numpy()[:count])
            for b in (b for b in picked if b < count):
                gap = np.abs(full[b].astype(LD) - two[b].astype(LD))
                assert (gap <= dref[b][1]).all(), "%s, instance %d: fused %r, two-step %r" % (what, b, full[b], two[b])
                worst["between"] = max(worst["between"], float(np.max(gap / np.where(dref[b][1] > 0, dref[b][1], 1))))
    fused = "%.3g" % worst["fused"] if want_dist is not None else "falls back"
    print("componentwise %-58s rows worst %8.3g u M  kappa %4d   distances, of their bound: fused %s, two-step %.3g"
          % (_id(case, no_blocks), worst["rows"], kap, fused, worst["two_step"]))
