"""mpcasm_qp_solve_wide_soft (``engine.solve_qp_wide(soft=...)``): the wide solve with soft limits, against
tests/soft_restatement.py with test_gpu_qp_solve_wide.py's ``assert_matches`` and bounds, one shape per
instantiation of the kernel the launch can pick (columns per lane 1, 2, 4, 8; K^-1 on chip and in d_kinv -- with 8
columns per lane K^-1 never fits on chip), against the hard wide entry bit for bit where every row is hard, and
against the narrow soft entry."""
import numpy as np
import pytest

import osqp_restatement as rs
import soft_cases as sc
from test_gpu_qp_solve import to_dev
from test_gpu_qp_solve_wide import assert_matches

pytestmark = pytest.mark.gpu
# (no, nc, K^-1's home): the smallest no of every count of columns per lane, and C3's shape
CASES = [(1, 1, "lds"), (1, 1, "global"), (36, 76, "lds"), (65, 70, "lds"), (65, 70, "global"), (96, 196, "lds"),
         (96, 196, "global"), (129, 40, "lds"), (129, 40, "global"), (257, 260, "global")]
FIELDS = ("x", "y", "z", "status", "iters", "res", "rho")


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def case_id(case):
    return "%dx%d %s" % case


@pytest.mark.parametrize("no,nc,home", CASES, ids=[case_id(c) for c in CASES])
def test_a_mixed_batch_against_the_restatement(gpu_api, torch_gpu, monkeypatch, no, nc, home):
    torch = torch_gpu
    from mpcasm import engine

    monkeypatch.setenv("MPCASM_QP_WIDE_KINV", home)
    assert engine.qp_solve_wide_soft_info(no, nc)[1] == (home == "lds")
    P, q, G, h, lin, quad = sc.mixed_batch(no, nc, sc.seed(no, nc))
    ref = sc.expected(P, q, G, h, lin, quad)
    sol = engine.solve_qp_wide(*to_dev(torch, P, q, G, h), soft=(lin, quad))
    for b in range(P.shape[0]):
        assert_matches(sol, ref[b], b, "wide soft %dx%d" % (no, nc), tol=sc.tolerance(P[b], G[b], ref[b]), P=P[b],
                       G=G[b])
    got = sorted(set(int(s) for s in sol.status.cpu()))
    assert got == sorted({1, -4, -7} | ({-3} if nc >= 2 else set()))


@pytest.mark.parametrize("no,nc,home", [c for c in CASES if c[0] != 36], ids=[case_id(c) for c in CASES if c[0] != 36])
def test_all_rows_hard_is_the_hard_wide_entry_bit_for_bit(gpu_api, torch_gpu, monkeypatch, no, nc, home):
    torch = torch_gpu
    from mpcasm import engine

    monkeypatch.setenv("MPCASM_QP_WIDE_KINV", home)
    assert engine.qp_solve_wide_info(no, nc)[1] == engine.qp_solve_wide_soft_info(no, nc)[1] == (home == "lds")
    P, q, G, h = sc.mixed_batch(no, nc, sc.seed(no, nc))[:4]
    dev = to_dev(torch, P, q, G, h)
    kh, ks = (torch.full(tuple(dev[0].shape), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    hard = engine.solve_qp_wide(*dev, kinv=kh)
    soft = engine.solve_qp_wide(*dev, kinv=ks, soft=(np.inf, 0.0))
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    for name, a, b in zip(FIELDS + ("kinv",), tuple(soft) + (ks,), tuple(hard) + (kh,)):
        assert torch.equal(bits(a), bits(b)), name
    assert len(set(hard.status.tolist())) >= (4 if nc >= 2 else 3)


def test_bad_penalties_and_the_stride(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine

    P, q, G, h, lin, quad = sc.mixed_batch(96, 196, sc.seed(96, 196))
    P, q, G, h, lin, quad = (np.concatenate([a[:5], a[:3]]) for a in (P, q, G, h, lin, quad))
    lin[5, 195], lin[6, 0], quad[7, 100] = -1.0, np.nan, np.inf
    lin[7, 100] = 1.0
    dev = to_dev(torch, P, q, G, h)
    sol = engine.solve_qp_wide(*dev, soft=(lin, quad))
    assert sol.status.tolist()[5:] == [rs.NON_CVX] * 3 and sol.iters.tolist()[5:] == [0] * 3
    for t in (sol.x, sol.y, sol.z, sol.res):
        assert bool(t[5:].isnan().all()) and not bool(t[:5].isnan().any())
    good = engine.solve_qp_wide(*(t[:5].contiguous() for t in dev), soft=(lin[:5], quad[:5]))
    for name, a, b in zip(FIELDS, sol, good):
        assert torch.equal(a[:5], b), name
    one = engine.solve_qp_wide(*dev, soft=(lin[0], quad[0]))
    each = engine.solve_qp_wide(*dev, soft=(np.tile(lin[0], (8, 1)), np.tile(quad[0], (8, 1))))
    for name, a, b in zip(FIELDS, one, each):
        assert torch.equal(a, b), name


def test_narrow_and_wide_agree_on_the_biped_shape(gpu_api, torch_gpu):
    """(36, 76) through both soft entries: each the restatement's within the bound the hard pair's test uses
    (test_gpu_qp_solve_wide.py's ``test_both_paths_where_both_apply``: rounding times cond(K)), so the two within
    twice that of each other."""
    torch = torch_gpu
    from helpers import assert_close
    from mpcasm import engine

    P, q, G, h, lin, quad = sc.mixed_batch(36, 76, sc.seed(36, 76))
    ref = sc.expected(P, q, G, h, lin, quad)
    dev = to_dev(torch, P, q, G, h)
    narrow = engine.solve_qp(*dev, soft=(lin, quad))
    wide = engine.solve_qp_wide(*dev, soft=(lin, quad))
    assert torch.equal(narrow.status, wide.status) and torch.equal(narrow.iters, wide.iters)
    for b in range(P.shape[0]):
        tol = sc.tolerance(P[b], G[b], ref[b])
        for sol in (narrow, wide):
            assert_matches(sol, ref[b], b, "36x76", tol=tol, P=P[b], G=G[b])
        if ref[b].status != rs.NON_CVX:
            assert_close(wide.x[b].cpu().numpy(), narrow.x[b].cpu().numpy(), 2 * tol, "x[%d]" % b)
            assert_close(wide.z[b].cpu().numpy(), narrow.z[b].cpu().numpy(), 2 * tol, "z[%d]" % b)


def test_polish_with_soft_raises(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine

    dev = to_dev(torch, *sc.mixed_batch(5, 9, sc.seed(5, 9))[:4])
    with pytest.raises(ValueError, match="polish"):
        engine.solve_qp_wide(*dev, soft=(1.0, 0.0), polish=True)
