"""GPU: mpcasm.diff.solve_qp_diff -- torch.autograd through solve_qp(..., polish=True) -- on the instances of
tests/polish_wide_cases.py that both polishes take (the wide-polish tests already require the plain ones to polish
to the constructed active set).  The loss is (c . x).sum() + (d . y).sum(); after backward, q.grad and h.grad are
-u and w of a direct engine.qp_sensitivity call on the returned iterate, bit for bit; P.grad and G.grad are that
call's u, w in products, within the product bound of tests/sens_cases.py; an instance that is not SENS_DONE has zero
gradients; and a gradient nobody asked for is neither computed nor allocated."""
import numpy as np
import pytest

import polish_wide_cases as cases
import sens_cases as sc
import sens_restatement as sn
from helpers import LD, U64
from mpcasm import capi

pytestmark = pytest.mark.gpu
BROKEN = 6                      # the instance whose P is -I: not solved, so not SENS_DONE


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def operands(torch, no, nc, na):
    qp = [a.copy() for a in cases.problem(no, nc, na)[:4]]
    qp[0][BROKEN] = -np.eye(no)
    rng = np.random.default_rng([no, nc, na, 75])
    c, d = rng.standard_normal((7, no)), rng.standard_normal((7, nc))
    return [torch.as_tensor(a, device="cuda") for a in qp], torch.as_tensor(c, device="cuda"), \
        torch.as_tensor(d, device="cuda")


def check(torch, engine, res, tensors, c, d, wide):
    """The gradients on ``tensors`` = (P, q, G, h) after backward, against a direct sensitivity call."""
    P, q, G, h = tensors
    sens = engine.qp_sensitivity_wide if wide else engine.qp_sensitivity
    direct = sens(P.detach(), G.detach(), h.detach(), res.sol, c, d, status=res.sol.status)
    assert torch.equal(res.verdict, direct.verdict)
    verdict = direct.verdict.tolist()
    assert verdict[BROKEN] != capi.SENS_DONE and res.sol.status[BROKEN].item() != capi.QP_SOLVED
    assert verdict[:3] == [capi.SENS_DONE] * 3 and res.sol.polish[:3].tolist() == [capi.POLISH_DONE] * 3
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert same(q.grad, -direct.u) and same(h.grad, direct.w)
    u, w, x, y = (t.detach().cpu().numpy().astype(LD) for t in (direct.u, direct.w, res.sol.x, res.sol.y))
    hq, z = h.detach().cpu().numpy(), res.sol.z.cpu().numpy()
    worst = [0.0, 0.0]
    for b in range(P.shape[0]):
        for t in (q.grad, h.grad, P.grad, G.grad):
            if verdict[b] != capi.SENS_DONE:
                assert t is None or not bool(t[b].any()), b                    # zero gradients
        if verdict[b] != capi.SENS_DONE:
            continue
        active = sn.active_set(hq[b], y[b].astype(np.float64), z[b])[0]
        _, _, gP, gG = sn.gradients(u[b], w[b], x[b], y[b], active)
        if P.grad is not None:
            bound = 4 * U64 * (np.abs(np.outer(u[b], x[b])) + np.abs(np.outer(x[b], u[b])))
            worst[0] = max(worst[0], sc.product_errors(P.grad[b].cpu().numpy(), gP, bound))
        if G.grad is not None:
            bound = 4 * U64 * (np.abs(np.outer(y[b], u[b])) + np.abs(np.outer(w[b], x[b])))
            assert not bool(G.grad[b][torch.as_tensor(~active, device="cuda")].any())
            worst[1] = max(worst[1], sc.product_errors(G.grad[b].cpu().numpy()[active], gG[active], bound[active]))
    return worst


RUNS = [s + (False,) for s in cases.BOTH] + [cases.BOTH[1] + (True,)]          # wide=True once


@pytest.mark.parametrize("no,nc,na,wide", RUNS, ids=["%dx%d-na%d-%s" % (s[:3] + ("wide" if s[3] else "lds",)) for s in RUNS])
def test_gradients_of_a_linear_loss(gpu_api, torch_gpu, monkeypatch, no, nc, na, wide):
    torch = torch_gpu
    from mpcasm import diff, engine

    tensors, c, d = operands(torch, no, nc, na)
    calls = []
    for name in ("qp_sensitivity", "qp_sensitivity_wide"):
        def spy(*args, _real=getattr(engine, name), _name=name, **kw):
            out = _real(*args, **kw)
            calls.append((_name, kw.get("want_P"), kw.get("want_G"), out))
            return out
        monkeypatch.setattr(engine, name, spy)
    for t in tensors:
        t.requires_grad_(True)
    res = diff.solve_qp_diff(*tensors, wide=wide)
    assert res.verdict is None and res.lres is None
    assert res.x.requires_grad and res.y.requires_grad and not res.sol.x.requires_grad
    assert res.x.data_ptr() == res.sol.x.data_ptr()
    ((c * res.x).sum() + (d * res.y).sum()).backward()
    torch.cuda.synchronize()
    expected = "qp_sensitivity_wide" if wide else "qp_sensitivity"
    assert [(n, p, g) for n, p, g, _ in calls] == [(expected, True, True)]          # ONE call
    assert res.verdict is not None and res.lres is not None
    calls.clear()
    worst = check(torch, engine, res, tensors, c, d, wide)
    sc.record("diff %s %dx%d-na%d" % ("wide" if wide else "lds", no, nc, na), "gP %.3f  gG %.3f" % tuple(worst))

    # P and G constant: their gradients are None, and the dense products were neither asked for nor allocated
    calls.clear()
    fresh, c, d = operands(torch, no, nc, na)
    fresh[1].requires_grad_(True)
    fresh[3].requires_grad_(True)
    res = diff.solve_qp_diff(*fresh, wide=wide)
    ((c * res.x).sum() + (d * res.y).sum()).backward()
    assert fresh[0].grad is None and fresh[2].grad is None
    assert [(n, p, g) for n, p, g, _ in calls] == [(expected, False, False)]
    assert calls[0][3].gP is None and calls[0][3].gG is None
    assert torch.equal(fresh[1].grad, tensors[1].grad) and torch.equal(fresh[3].grad, tensors[3].grad)


def test_the_solution_and_its_device_tensors_are_freed(gpu_api, torch_gpu):
    """The autograd node does not hold its own outputs: after ``del`` and one ``gc.collect()`` the result, its x and
    its solution's tensors are gone, with and without a backward pass."""
    import gc
    import weakref

    torch = torch_gpu
    from mpcasm import diff

    for backward in (False, True):
        tensors, c, d = operands(torch, 5, 3, 2)
        for t in tensors:
            t.requires_grad_(True)
        res = diff.solve_qp_diff(*tensors)
        if backward:
            ((c * res.x).sum() + (d * res.y).sum()).backward()
        alive = [weakref.ref(o) for o in (res, res.x, res.y, res.sol.x, res.sol.z, res.x.grad_fn)]
        del res
        gc.collect()
        assert [r() is None for r in alive] == [True] * len(alive), backward


def test_soft_limits_are_refused(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import diff

    tensors, _c, _d = operands(torch, 5, 3, 2)
    for wide in (False, True):
        with pytest.raises(ValueError):
            diff.solve_qp_diff(*tensors, wide=wide, soft=(1.0, 0.0))
