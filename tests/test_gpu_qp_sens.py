"""GPU: mpcasm_qp_sens (csrc/sens_core.h in csrc/polish.hip) against tests/sens_restatement.py -- its verdicts, the
accuracy of u, w, lres and of the dense gradients, what it leaves untouched -- on the shapes at which each loop of
the kernel can go wrong (tests/polish_restatement.py's: na = 0, na = no, nc > 64 for two ballot passes, no > 64 for
two columns a lane), through engine.qp_jvp, and on the biped's own QPs.  tests/sens_cases.py has the instances, the
yardstick and the judge.

The accuracy tests print ``qp-sens-precision: ...`` lines (pytest -s) and keep the worst ratios per shape in
profiles/qp_sens_precision.txt."""
import numpy as np
import pytest

import polish_restatement as pr
import sens_cases as sc
import sens_restatement as sn
from helpers import LD
from mpcasm import capi, problems

pytestmark = pytest.mark.gpu


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.mark.parametrize("no,nc,na", pr.SHAPES, ids=["%dx%d-na%d" % s for s in pr.SHAPES])
def test_verdicts_accuracy_and_untouched_outputs(gpu_api, torch_gpu, no, nc, na):
    """Seven instances of the shape -- three plain, one NON_CVX by its status with NaN iterates, one MAX_ITER by its
    status, one whose P is -I, one with rx = ry = 0 -- with their status and with status = NULL, with the dense
    gradients and without."""
    from mpcasm import engine

    assert engine.qp_sens_lds_bytes(no, nc) == engine.qp_polish_lds_bytes(no, nc)
    sc.seven(torch_gpu, engine.qp_sensitivity, no, nc, na, "lds")


def test_skipped_when_the_active_set_outgrows_the_unknowns(gpu_api, torch_gpu):
    """(5, 12) with every y positive: na = 12 > no = 5, SKIPPED, nothing written; allocated by the call itself, the
    outputs read as zero gradients."""
    torch = torch_gpu
    from mpcasm import engine

    case = sc.problem(5, 12, 3, count=3)
    y = (case["h"] - case["z"]) + 1.0
    outs, _ = sc.run(torch, engine.qp_sensitivity, case, (case["x"], y, case["z"]), None, "5x12, every row active")
    assert [o.verdict for o in outs] == [sn.SKIPPED] * 3 and all(o.active.all() for o in outs)
    dev = lambda a: torch.as_tensor(np.array(a), device="cuda")
    got = engine.qp_sensitivity(dev(case["P"]), dev(case["G"]), dev(case["h"]), (dev(case["x"]), dev(y), dev(case["z"])),
                                dev(case["rx"]), dev(case["ry"]), want_P=True, want_G=True)
    assert got.verdict.tolist() == [capi.SENS_SKIPPED] * 3
    assert all(not bool(t.any()) for t in (got.u, got.w, got.gP, got.gG, got.lres))
    vjp = engine.qp_vjp(dev(case["P"]), dev(case["G"]), dev(case["h"]), (dev(case["x"]), dev(y), dev(case["z"])),
                        dev(case["rx"]), dev(case["ry"]))
    assert vjp.gP is None and vjp.gG is None and not bool(vjp.gq.any()) and not bool(vjp.gh.any())


def test_the_forward_derivative_through_qp_jvp(gpu_api, torch_gpu):
    """engine.qp_jvp on (36, 76, 20) along a random (dq, dh, symmetric dP, dG): dx, dy against the restatement on
    the long-double right-hand side, by the same yardstick -- the right-hand side is itself a sum the device formed
    in fp64, so the magnitude of its terms, |dq| + |dP||x| + |dG_A'||y_A| and |dh| + |dG||x|, stands where |r| does."""
    torch = torch_gpu
    from mpcasm import engine

    no, nc, na = 36, 76, 20
    case = sc.problem(no, nc, na, count=3)
    rng = np.random.default_rng([no, nc, na, 74])
    dq, dh, dG = rng.standard_normal((3, no)), rng.standard_normal((3, nc)), rng.standard_normal((3, nc, no))
    dP = rng.standard_normal((3, no, no))
    dP = (dP + dP.transpose(0, 2, 1)) / 2.0
    c = lambda a: a.astype(LD)
    rx, ry, terms = [], [], []
    for b in range(3):
        x, y, active = c(case["x"][b]), c(case["y"][b]), case["active"][b]
        r1, r2 = sn.jvp_rhs(x, y, active, c(dq[b]), c(dh[b]), c(dP[b]), c(dG[b]))
        rx.append(r1.astype(np.float64))
        ry.append(r2.astype(np.float64))
        ya = np.where(active, np.abs(y), 0)
        terms.append((np.abs(dq[b]) + np.abs(dP[b]) @ np.abs(x) + np.abs(dG[b]).T @ ya,
                      np.abs(dh[b]) + np.abs(dG[b]) @ np.abs(x)))
    dev = lambda a: torch.as_tensor(np.array(a), device="cuda")
    got = engine.qp_jvp(dev(case["P"]), dev(case["G"]), dev(case["h"]), tuple(dev(case[k]) for k in "xyz"), dev(dq),
                        dev(dh), dP=dev(dP), dG=dev(dG))
    torch.cuda.synchronize()
    assert got.verdict.tolist() == [capi.SENS_DONE] * 3
    u, w = got.dx.cpu().numpy(), got.dy.cpu().numpy()
    res = np.array([sn.kkt_residual(case["P"][b], case["G"][b], case["active"][b], u[b], w[b], rx[b], ry[b])[0]
                    for b in range(3)])
    host = (u, w, None, None, got.verdict.cpu().numpy(), res)         # (qp_jvp returns no lres: the judge's own)
    outs, worst = sc.judge(case["P"], case["G"], case["h"], tuple(case[k] for k in "xyz"), np.stack(rx), np.stack(ry),
                           None, host, "qp_jvp 36x76 na 20", rhs_terms=terms)
    assert all(o.verdict == sn.DONE for o in outs)
    # without dP and dG the right-hand side is (-dq, dh) itself
    plain = engine.qp_jvp(dev(case["P"]), dev(case["G"]), dev(case["h"]), tuple(dev(case[k]) for k in "xyz"), dev(dq),
                          dev(dh))
    direct = engine.qp_sensitivity(dev(case["P"]), dev(case["G"]), dev(case["h"]), tuple(dev(case[k]) for k in "xyz"),
                                   dev(-dq), dev(dh))
    assert torch.equal(plain.dx, direct.u) and torch.equal(plain.dy, direct.w)
    # on a stream of the caller's the right-hand side is formed on that stream too: the same bits
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    held = (dev(case["P"]), dev(case["G"]), dev(case["h"]), tuple(dev(case[k]) for k in "xyz"), dev(dq), dev(dh),
            dev(dP), dev(dG))                                  # (alive until the stream has read them)
    there = engine.qp_jvp(*held[:6], dP=held[6], dG=held[7], stream=side)
    side.synchronize()
    assert torch.equal(there.dx, got.dx) and torch.equal(there.dy, got.dy)
    sc.record("jvp 36x76-na20", "residual %.3f" % worst[0])


# ---- the biped's own QPs ---------------------------------------------------------------------------------------
def test_the_bipeds_qps_five_ticks_in(gpu_api, torch_gpu):
    """64 biped QPs five closed ticks into the loop of a fleet whose walkers start slightly apart, solved with
    polish=True: verdicts, u, w and lres against the restatement on the same iterates, for every instance whose
    restated active-set margin is at least 1e-6 -- at least 0.9 of the 64."""
    torch = torch_gpu
    from mpcasm import engine
    from mpcasm.walkers import WalkerFleet

    conf = problems.BipedConfig(step_samples=8)
    B = 64
    fleet = WalkerFleet(B, conf=conf, api=gpu_api)
    given = fleet.start_at_rest()
    rng = np.random.default_rng(3)
    given += torch.as_tensor(rng.normal(0.0, 2e-3, tuple(given.shape)), device=given.device)
    for _ in range(5):
        fleet.step()
    total = judged = done = 0
    worst = [0.0] * 4
    for entry in fleet.tick(given):
        P, q, G, h = (entry[k].clone() for k in ("P", "q", "G", "h"))
        sol = engine.solve_qp(P, q, G, h, polish=True)
        n, no, nc = P.shape[0], P.shape[1], G.shape[1]
        rx, ry = rng.standard_normal((n, no)), rng.standard_normal((n, nc))
        case = dict(P=P.cpu().numpy(), G=G.cpu().numpy(), h=h.cpu().numpy(), rx=rx, ry=ry)
        xyz = tuple(t.cpu().numpy() for t in (sol.x, sol.y, sol.z))
        outs, w = sc.run(torch, engine.qp_sensitivity, case, xyz, sol.status.cpu().numpy(), "biped", margin=1e-6)
        worst = [max(a, b) for a, b in zip(worst, w)]
        total += n
        judged += sum(o is not None for o in outs)
        done += sum(o is not None and o.verdict == sn.DONE for o in outs)
    assert total == B and judged >= 0.9 * total, (judged, total)
    assert done > 0, (done, judged)
    sc.record("biped-64", "residual %.3f  lres %.3f  gP %.3f  gG %.3f  (%d of %d judged, %d DONE)"
              % (worst[0], worst[1], worst[2], worst[3], judged, total, done))
