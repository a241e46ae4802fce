"""GPU: every variant of the horizon fill (csrc/fill.hip) element by element against extended precision.  The
family of fill_cases.py spans what fill_choose can select (test_fill_routes_cpu.py holds it to that); here each
case first asserts that the library takes the route its entry pins for the very pointers of the launch, then runs
mpcasm_fill_su into outputs that are views of NaN-filled buffers with 64 guard doubles on either side, and holds
every element of S and U to kappa(N, n) (u M + 2^-1022) against the oracle in long double on the fp64 inputs the
kernel saw (helpers.assert_componentwise; M from the oracle on the absolute values; structural zeros exact).  The
plants are free of cancellation (Perron root 1.3, badly scaled, mixed signs, a plant of its own per instance, of its
own per step with ltv), so elements span decades and M tracks the results: a relative error of 1e-6 in one small
element fails, where the block measure of test_gpu_fill.py lets it pass.

Measured (MI355X): profiles/fill_variants.txt."""
import numpy as np
import pytest

import fill_cases as fc
from helpers import assert_componentwise
from oracle import qp_oracle as orc

pytestmark = pytest.mark.gpu

GUARD = 64
OFF8 = [c for c in fc.RUN if c.off8 is not None]
LTV_CASES = [c for c in fc.RUN if c.ltv]
LIMITS = [c for c in fc.CASES if c.route is fc.LIMIT]


@pytest.fixture(scope="module")
def eng():
    import os

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    assert "MPCASM_FILL_MIN_WAVES" not in os.environ        # (the pinned routes are those of its default)
    from mpcasm import engine

    return engine


class Guarded:
    """A NaN-filled buffer and the view into it a launch writes: ``off`` doubles (0 or 1: 8 bytes) past a
    16-byte boundary, GUARD doubles in front and behind."""

    def __init__(self, torch, shape, off):
        self.size = int(np.prod(shape))
        self.first = GUARD + off
        self.buf = torch.full((self.first + self.size + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        self.view = self.buf[self.first:self.first + self.size].view(shape)
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == 8 * off

    def check(self, torch, what):
        front, back = self.buf[:self.first], self.buf[self.first + self.size:]
        assert bool(torch.isnan(front).all()), "%s: a write in front of the output" % what
        assert bool(torch.isnan(back).all()) and back.numel() == GUARD, "%s: a write behind the output" % what
        assert not bool(torch.isnan(self.view).any()), "%s: an element never written" % what


def launch(eng, case, A, B, s_off=0, u_off=0, ltv=None, what=""):
    """mpcasm_fill_su of the case's shape into guarded outputs; asserts the route and the guards.  Returns device
    views ``S (batch, N, n, n)``, ``U (batch, m, N, N, n)``."""
    import torch

    ltv = case.ltv if ltv is None else ltv
    batch, N, n, m = case.batch, case.N, case.n, case.m
    S = Guarded(torch, (batch, N, n, n), s_off)
    U = Guarded(torch, (batch, m, N, N, n), u_off)
    if ltv == case.ltv:
        route = eng.fill_route(batch, N, n, m, ltv, aligned16=(S.view.data_ptr() | U.view.data_ptr()) % 16 == 0)
        assert fc.Route(*route[:5]) == (case.off8 if s_off or u_off else case.route), route
    # (torch.tensor copies: the inputs are read-only arrays shared by the tests)
    eng.fill_su(torch.tensor(A, device="cuda"), torch.tensor(B, device="cuda"), N, ltv=bool(ltv), out=(S.view, U.view))
    torch.cuda.synchronize()
    S.check(torch, "%s S%s" % (case.name, what))
    U.check(torch, "%s U%s" % (case.name, what))
    return S.view, U.view


def host(case, S, U):
    """``{instance: (S, U)}`` on the host for the instances the oracle has (every one of a small batch), and the
    whole arrays where the whole batch is compared on the host."""
    if case.name in fc.DISTINCT:      # copies against their originals on the device, bit for bit (one launch, one kernel)
        import torch

        k = fc.DISTINCT[case.name]
        Sb, Ub = S.view(torch.int64), U.view(torch.int64)
        for r in range(k):
            assert bool((Sb[r::k] == Sb[r:r + 1]).all()) and bool((Ub[r::k] == Ub[r:r + 1]).all()), (case.name, r)
        return {b: (S[b].cpu().numpy(), U[b].cpu().numpy()) for b in fc.sample(case)}, None
    Sh, Uh = S.cpu().numpy(), U.cpu().numpy()
    which = range(case.batch) if case.batch <= fc.SMALL_BATCH else fc.sample(case)
    return {b: (Sh[b], Uh[b]) for b in which}, (Sh, Uh)


def hold(case, S, U, what=""):
    """Every element within kappa of extended precision.  Returns the worst errors of S and U in units of u M."""
    per, whole = host(case, S, U)
    ref, kappa = fc.oracle(case), fc.kappa(case)
    worst = [0.0, 0.0]
    for b, mine in per.items():
        for i, key in enumerate("SU"):
            worst[i] = max(worst[i], assert_componentwise(mine[i], *ref[b][key], kappa,
                                                          "%s%s %s[%d]" % (case.name, what, key, b)))
    if case.batch > fc.SMALL_BATCH and whole is not None:
        every = fc.batch_reference(case)
        for i, key in enumerate("SU"):
            worst[i] = max(worst[i], assert_componentwise(whole[i], *every[key], kappa,
                                                          "%s%s %s (whole batch)" % (case.name, what, key)))
    return worst


@pytest.mark.parametrize("case", fc.RUN, ids=[c.name for c in fc.RUN])
def test_every_element_within_kappa(eng, case):
    A, B = fc.inputs(case)
    S, U = launch(eng, case, A, B)
    worst = hold(case, S, U)
    print("componentwise %-22s %-22s<%d> flags %d spw %d lshift %d   S %7.3g  U %7.3g u M   kappa %d"
          % (case.name, fc.KERNEL[case.route.kernel], case.route.arg, case.route.flags, case.route.spw,
             case.route.lshift, worst[0], worst[1], fc.kappa(case)))


@pytest.mark.parametrize("case", OFF8, ids=[c.name for c in OFF8])
def test_outputs_eight_bytes_off_a_16_byte_boundary(eng, case):
    """S, U and both 8 bytes off: the decision passes over the kernels that store 16-byte words (the route pinned
    as ``off8``).  Every kernel runs the same recurrence in the same order of association, so each of the three
    launches reproduces the aligned launch bit for bit, the sign of exact zeros apart (fill_cases.same_bits and
    the reason there); the first is also held to the bound on its own."""
    A, B = fc.inputs(case)
    S0, U0 = launch(eng, case, A, B)
    for s_off, u_off in ((1, 1), (1, 0), (0, 1)):
        what = " (S + %d, U + %d bytes)" % (8 * s_off, 8 * u_off)
        S, U = launch(eng, case, A, B, s_off, u_off, what=what)
        if (s_off, u_off) == (1, 1):
            worst = hold(case, S, U, what)
            print("componentwise %-22s %-22s<%d> flags %d spw %d (8 bytes off)   S %7.3g  U %7.3g u M   kappa %d"
                  % (case.name, fc.KERNEL[case.off8.kernel], case.off8.arg, case.off8.flags, case.off8.spw,
                     worst[0], worst[1], fc.kappa(case)))
        assert fc.same_bits(S, S0) and fc.same_bits(U, U0), case.name + what
        del S, U


@pytest.mark.parametrize("case", LTV_CASES, ids=[c.name for c in LTV_CASES])
def test_equal_steps_reproduce_the_lti_fill(eng, case):
    """Per-step kernels given the same (A, B) at every step, and the LTI fill of that plant: both within the bound
    of the LTI oracle in long double, every instance; and, since ``A_k`` times the row before is the LTI
    recurrence in the same order, equal to each other bit for bit, the sign of exact zeros apart
    (fill_cases.same_bits)."""
    A, B = fc.inputs(case)
    A0, B0 = np.ascontiguousarray(A[:, 0]), np.ascontiguousarray(B[:, 0])
    S1, U1 = launch(eng, case, np.repeat(A0[:, None], case.N, axis=1), np.repeat(B0[:, None], case.N, axis=1))
    S2, U2 = launch(eng, case, A0, B0, ltv=0)
    assert case.batch <= fc.SMALL_BATCH
    hosts = [(S1.cpu().numpy(), U1.cpu().numpy(), "equal steps"), (S2.cpu().numpy(), U2.cpu().numpy(), "lti")]
    for b in range(case.batch):
        Sr, Ur = orc.extend_matrices(case.N, A0[b], B0[b], dtype=fc.LD)
        Sm, Um = orc.extend_matrices(case.N, np.abs(A0[b]), np.abs(B0[b]), dtype=fc.LD)
        for S, U, what in hosts:
            assert_componentwise(S[b], Sr, Sm, fc.kappa(case), "%s %s S[%d]" % (case.name, what, b))
            assert_componentwise(U[b], np.stack(Ur), np.stack(Um), fc.kappa(case), "%s %s U[%d]" % (case.name, what, b))
    assert fc.same_bits(S1, S2) and fc.same_bits(U1, U2), case.name


@pytest.mark.parametrize("case", LIMITS, ids=[c.name for c in LIMITS])
def test_beyond_a_limit_nothing_is_launched(eng, case):
    import torch

    from mpcasm import capi

    steps = case.N if case.ltv else 1
    A = torch.zeros((case.batch, steps, case.n, case.n), dtype=torch.float64, device="cuda")
    B = torch.zeros((case.batch, steps, case.n, case.m), dtype=torch.float64, device="cuda")
    S = Guarded(torch, (case.batch, case.N, case.n, case.n), 0)
    U = Guarded(torch, (case.batch, case.m, case.N, case.N, case.n), 0)
    rc = capi.load().mpcasm_fill_su(A.data_ptr(), B.data_ptr(), S.view.data_ptr(), U.view.data_ptr(), case.batch,
                                    case.N, case.n, case.m, case.ltv, None)
    torch.cuda.synchronize()
    assert rc == capi.ERR_LIMIT
    assert bool(torch.isnan(S.buf).all()) and bool(torch.isnan(U.buf).all())
