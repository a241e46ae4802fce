"""GPU: K1 (mpcasm_fill_su through the C ABI) against the oracle, the golden
vectors and size-independent properties.  Tolerance: 1e-10 relative (north star);
the kernel follows the reference recurrence, so the observed error is ~1e-16.
"""
import numpy as np
import pytest

from helpers import LD, RTOL, RTOL_TIGHT, assert_close, assert_componentwise, golden, kappa
from oracle import qp_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mpcasm import engine

    return engine


def test_reference_fixture_through_the_drop_in_api(gpu_api):
    """test_dynamics.py:139-152 of the reference, run on this repository's API:
    ExtendedSystem.from_cotrol_system -> tools.extend_matrices -> HIP kernel."""
    g = golden("g1_extend")
    lip = gpu_api.ControlSystem.from_name(system_name="J->CCC", tau=0.1, omega=3.3445,
                                          axes=["_x", "_y"])
    ext = gpu_api.ExtendedSystem.from_cotrol_system(lip, state_vector_name="x", horizon_lenght=36)
    assert ext.matrices[0].shape == (36, 36, 3) and ext.matrices[1].shape == (36, 3, 3)
    assert_close(ext.matrices[0], g["lip36/U0"], RTOL_TIGHT, "U")
    assert_close(ext.matrices[1], g["lip36/S"], RTOL_TIGHT, "S")


@pytest.mark.parametrize("n,m,N", [(3, 1, 16), (3, 1, 32), (3, 1, 100), (8, 6, 20),
                                   (12, 6, 64), (1, 1, 5), (2, 3, 1), (1, 1, 1), (5, 2, 7),
                                   (17, 3, 9), (24, 18, 4),
                                   # few states: the register/DPP kernel (rows per store 1 ... 64,
                                   # rows longer than a wavefront, several inputs) and its fall-backs
                                   (4, 2, 12), (2, 1, 8), (1, 3, 6), (3, 2, 10), (4, 12, 6), (3, 1, 2),
                                   (2, 2, 64), (4, 1, 40), (3, 1, 15), (4, 1, 1), (3, 13, 4)])
def test_lti_against_golden_and_oracle(eng, gpu_api, n, m, N):
    g = golden("g1_extend")
    key = "lti_n%d_m%d_N%d/" % (n, m, N)
    if key + "A" in g:
        A, B = g[key + "A"], g[key + "B"]
    else:
        rng = np.random.default_rng(n * 1000 + m * 10 + N)
        A, B = rng.standard_normal((n, n)) / np.sqrt(n), rng.standard_normal((n, m))
    S, U = gpu_api.tools.extend_matrices(N, A, B)        # drop-in signature: (S, [U_j])
    assert S.shape == (N, n, n) and isinstance(U, list) and len(U) == m
    assert U[0].shape == (N, N, n)
    So, Uo = orc.extend_matrices(N, A, B)
    assert_close(S, So, RTOL_TIGHT, "S vs oracle")
    assert_close(np.stack(U), np.stack(Uo), RTOL_TIGHT, "U vs oracle")
    if key + "S" in g:
        assert_close(S, g[key + "S"], RTOL, "S vs golden")
        if key + "U" in g:
            assert_close(np.stack(U), g[key + "U"], RTOL, "U vs golden")
        else:
            rows = g[key + "U_rows"]
            assert_close(U[0][rows], g[key + "U_first"], RTOL)
            assert_close(U[m - 1][rows], g[key + "U_last"], RTOL)
    # structural zeros are written, exactly
    for j in range(m):
        for k in range(N):
            assert not U[j][k, k + 1:].any()


def test_batched_lti_per_instance_systems(eng):
    """Every instance has its own (A, B); ragged batch sizes hit partially filled
    workgroups (4 systems per 256-thread block on the small path)."""
    rng = np.random.default_rng(77)
    for batch in (1, 3, 4, 5, 67):
        A = rng.standard_normal((batch, 3, 3)) / 2
        B = rng.standard_normal((batch, 3, 1))
        S, U = eng.fill_su_numpy(A, B, 16)
        assert S.shape == (batch, 16, 3, 3) and U.shape == (batch, 1, 16, 16, 3)
        for b in range(batch):
            So, Uo = orc.extend_matrices(16, A[b], B[b])
            assert_close(S[b], So, RTOL_TIGHT)
            assert_close(U[b], np.stack(Uo), RTOL_TIGHT)


def test_batched_lti_several_systems_per_wavefront(eng):
    """Batches large enough for the few-state kernel to put 2 ... 5 systems on one wavefront,
    ragged at the end; every system against a vectorised restatement of the recurrence, a
    sample against the oracle."""
    import torch

    rng = np.random.default_rng(78)
    for batch, n, m, N in ((8195, 3, 1, 16), (4097, 3, 1, 16), (10241, 2, 1, 8), (6151, 4, 3, 6),
                           (6145, 3, 1, 100), (9001, 1, 2, 4)):
        A = rng.standard_normal((batch, n, n)) / np.sqrt(n)
        B = rng.standard_normal((batch, n, m))
        S, U = eng.fill_su(torch.as_tensor(A, device="cuda"), torch.as_tensor(B, device="cuda"), N)
        S, U = S.cpu().numpy(), U.cpu().numpy()
        X, Sref, col = B.copy(), [], []
        P = A.copy()
        for k in range(N):
            col.append(X)                               # A^k B
            Sref.append(P.transpose(0, 2, 1))           # S[k][j][i] = (A^{k+1})[i][j]
            X, P = A @ X, A @ P
        assert_close(S, np.stack(Sref, axis=1), RTOL_TIGHT, "S")
        Uref = np.zeros_like(U)
        for k in range(N):
            for l in range(k + 1):
                Uref[:, :, k, l, :] = col[k - l].transpose(0, 2, 1)
        assert_close(U, Uref, RTOL_TIGHT, "U")
        for b in (0, batch // 3, batch - 1):
            So, Uo = orc.extend_matrices(N, A[b], B[b])
            assert_close(S[b], So, RTOL_TIGHT)
            assert_close(U[b], np.stack(Uo), RTOL_TIGHT)


@pytest.mark.parametrize("n,m,N", [(3, 1, 100), (3, 1, 7), (4, 2, 12), (12, 6, 16), (70, 2, 3),
                                   (2, 1, 64), (1, 1, 10), (4, 3, 30), (3, 2, 101), (3, 1, 16)])
def test_ltv_against_oracle(eng, n, m, N):
    """Per-step (A_k, B_k): parity unpinned beyond the degenerate LTI case (the
    reference has no such path); checked against the oracle's
    own generalisation and, for constant steps, against the LTI kernel."""
    rng = np.random.default_rng(N * 100 + n)
    batch = 3
    A = rng.standard_normal((batch, N, n, n)) / np.sqrt(n)
    B = rng.standard_normal((batch, N, n, m))
    S, U = eng.fill_su_numpy(A, B, N, ltv=True)
    for b in range(batch):
        So, Uo = orc.extend_matrices_ltv(N, A[b], B[b])
        assert_close(S[b], So, RTOL_TIGHT, "S")
        assert_close(U[b], np.stack(Uo), RTOL_TIGHT, "U")
    A0, B0 = A[:, :1].repeat(N, axis=1), B[:, :1].repeat(N, axis=1)
    S1, U1 = eng.fill_su_numpy(A0, B0, N, ltv=True)
    S2, U2 = eng.fill_su_numpy(A0[:, 0], B0[:, 0], N)
    assert_close(S1, S2, RTOL_TIGHT)
    assert_close(U1, U2, RTOL_TIGHT)


def test_ltv_lipm_config_c5(eng, gpu_api):
    from mpcasm import problems

    A, B = problems.ltv_lipm_steps(gpu_api, N=100, theta=0.3)
    S, U = eng.fill_su_numpy(A[None], B[None], 100, ltv=True)
    So, Uo = orc.extend_matrices_ltv(100, A, B)
    assert_close(S[0], So, RTOL)
    assert_close(U[0], np.stack(Uo), RTOL)
    # element by element against extended precision
    S1, U1 = orc.extend_matrices_ltv(100, A, B, dtype=LD)
    S2, U2 = orc.extend_matrices_ltv(100, np.abs(A), np.abs(B), dtype=LD)
    assert_componentwise(S[0], S1, S2, kappa(100, 3), "S")
    assert_componentwise(U[0], np.stack(U1), np.stack(U2), kappa(100, 3), "U")


def test_full_size_properties_c2_and_c4(eng):
    """BASELINE sizes, checked through properties that need no CPU recomputation of
    the whole batch: Toeplitz structure (U[k,l] == U[k-l,0]), zeros above the
    diagonal, linearity in B, and S[k] == A^T-recurrence of S[k-1]."""
    import torch

    rng = np.random.default_rng(4)
    for batch, n, m, N in ((4096, 3, 1, 16), (16, 12, 6, 64)):
        A = torch.as_tensor(rng.standard_normal((batch, n, n)) / np.sqrt(n) * 0.9, device="cuda")
        B1 = torch.as_tensor(rng.standard_normal((batch, n, m)), device="cuda")
        B2 = torch.as_tensor(rng.standard_normal((batch, n, m)), device="cuda")
        S, U1 = eng.fill_su(A, B1, N)
        _, U2 = eng.fill_su(A, B2, N)
        _, U12 = eng.fill_su(A, B1 + 2.0 * B2, N)
        lin = (U12 - (U1 + 2.0 * U2)).abs().max().item()
        assert lin <= 1e-12 * max(1.0, U12.abs().max().item())
        # Toeplitz: every block row is the first block column shifted
        first_col = U1[:, :, :, 0, :]                      # (B, m, N, n): A^k B
        for k in (1, N // 2, N - 1):
            for l in (0, 1, k):
                assert torch.equal(U1[:, :, k, l, :], first_col[:, :, k - l, :])
        iu = torch.triu_indices(N, N, offset=1, device="cuda")
        assert U1[:, :, iu[0], iu[1], :].abs().max().item() == 0.0
        # S[k][j][i] = (A^{k+1})[i][j]  ->  S[k] = S[k-1] @ A^T ... as stored: S_k^T = A S_{k-1}^T
        St = S.transpose(-1, -2)                            # (B, N, n, n) = A^{k+1}
        rec = torch.matmul(A.unsqueeze(1), St[:, :-1])
        assert (rec - St[:, 1:]).abs().max().item() <= 1e-12 * max(1.0, St.abs().max().item())
        assert torch.equal(St[:, 0], A)
        # one instance against the oracle
        b = batch // 2
        So, Uo = orc.extend_matrices(N, A[b].cpu().numpy(), B1[b].cpu().numpy())
        assert_close(S[b].cpu().numpy(), So, RTOL_TIGHT)
        assert_close(U1[b].cpu().numpy(), np.stack(Uo), RTOL_TIGHT)


def test_argument_errors(eng):
    import torch

    A = torch.zeros((2, 3, 3), dtype=torch.float64, device="cuda")
    B = torch.zeros((2, 3, 1), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        eng.fill_su(A, B[:1], 4)
    from mpcasm import capi

    lib = capi.load()
    assert lib.mpcasm_fill_su(None, None, None, None, 1, 4, 3, 1, 0, None) == -1
    assert lib.mpcasm_fill_su(A.data_ptr(), B.data_ptr(), A.data_ptr(), B.data_ptr(),
                              1, 0, 3, 1, 0, None) == -1
    # empty batch is a no-op
    assert lib.mpcasm_fill_su(A.data_ptr(), B.data_ptr(), A.data_ptr(), B.data_ptr(),
                              0, 4, 3, 1, 0, None) == 0
