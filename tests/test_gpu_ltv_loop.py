"""GPU: the closed loop of a plan compiled with ``ltv=`` (mpcasm.ltv_loop.LtvLoop: window -> assemble -> solve ->
advance, nothing read back), teacher-forced as test_gpu_fleet_loop.py's fleet is: every tick is checked from the
device's own solution and status -- the next ``given`` is the long-double ``x_1 = A_t x_0 + B_t u_0`` where the
status applies under the loop's rule, within kappa_rollout, and the old row, bit for bit, where it does not.  The
inputs (rollout_cases.loop_inputs) make instance 1 primal infeasible and the others solved at every tick on the CPU
restatement (test_ltv_rollout_cpu.py), so both branches of "hold" run."""
import numpy as np
import pytest

import rollout_cases as rc
from helpers import assert_componentwise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.mark.parametrize("on_unsolved", ["hold", "apply"])
def test_the_loop_tick_by_tick(gpu_api, torch_gpu, on_unsolved):
    torch = torch_gpu
    from mpcasm.ltv_loop import LtvLoop

    form, A, B, given0 = rc.loop_inputs(gpu_api)
    loop = LtvLoop(form, "LIP", rc.LOOP_BATCH, torch.as_tensor(A, device="cuda"), torch.as_tensor(B, device="cuda"),
                   on_unsolved=on_unsolved)
    assert loop.given.shape == (rc.LOOP_BATCH, form.given_len) and loop.given.dtype == torch.float64
    assert loop.ticks_possible == rc.LOOP_T - rc.LOOP_N + 1
    loop.given.copy_(torch.as_tensor(given0, device="cuda"))
    plan = loop.asm.plan
    kap = rc.kappa_rollout(rc.LOOP_N, 3, 1)
    applied = held = 0
    seen = np.zeros((rc.LOOP_TICKS, rc.LOOP_BATCH), dtype=np.int64)
    for t in range(rc.LOOP_TICKS):
        pre = loop.given.cpu().numpy()
        out = loop.step()
        assert loop.t == t + 1
        x, status, post = out["x"].cpu().numpy(), out["status"].cpu().numpy(), loop.given.cpu().numpy()
        seen[t] = status
        for b in range(rc.LOOP_BATCH):
            if rc.applies(int(status[b]), on_unsolved):
                assert np.isfinite(x[b]).all()
                ref = rc.first_step_reference(plan, A[b, t], B[b, t], pre[b], x[b])
                assert_componentwise(post[b], *ref, kap, "tick %d, instance %d" % (t, b))
                applied += 1
            else:
                assert np.array_equal(post[b], pre[b]), (t, b)
                held += 1
    print("statuses per tick:", seen.tolist())
    if on_unsolved == "hold":
        assert applied and held, seen
    else:               # (a primal infeasible instance's iterate is applied too: nothing is held)
        assert applied == rc.LOOP_TICKS * rc.LOOP_BATCH and not held, seen
    # the sequences are used up one tick after the last window
    for _ in range(loop.ticks_possible - rc.LOOP_TICKS):
        loop.step()
    with pytest.raises(ValueError):
        loop.step()
    with pytest.raises(ValueError):
        LtvLoop(form, "LIP", rc.LOOP_BATCH, torch.as_tensor(A, device="cuda"), torch.as_tensor(B, device="cuda"),
                on_unsolved="drop")


def test_run_records_and_a_larger_batch_stays_finite(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm.ltv_loop import LtvLoop

    form, A, B, given0 = rc.loop_inputs(gpu_api)
    dev = lambda v: torch.as_tensor(v, device="cuda")
    loop = LtvLoop(form, "LIP", rc.LOOP_BATCH, dev(A), dev(B))
    loop.given.copy_(dev(given0))
    out = loop.run(3, record=True)
    assert set(out) == {"status", "iters", "given"}
    assert out["status"].shape == out["iters"].shape == (3, rc.LOOP_BATCH)
    assert out["status"].dtype == out["iters"].dtype == torch.int32
    assert out["given"].shape == (4, rc.LOOP_BATCH, form.given_len) and out["given"].dtype == torch.float64
    assert torch.equal(out["given"][0].cpu(), torch.as_tensor(given0)) and torch.equal(out["given"][3], loop.given)
    assert set(loop.run(1)) == {"status", "iters"}
    # the same loop, tick by tick, gives the same trail (nothing but the launches above happens in run)
    again = LtvLoop(form, "LIP", rc.LOOP_BATCH, dev(A), dev(B))
    again.given.copy_(dev(given0))
    for t in range(3):
        status = again.step()["status"]
        assert torch.equal(status, out["status"][t]) and torch.equal(again.given, out["given"][t + 1])
    # 512 instances, 3 ticks: the four sequences over and over, every instance its own start
    batch = 512
    reps = batch // rc.LOOP_BATCH
    big = LtvLoop(form, "LIP", batch, dev(np.tile(A, (reps, 1, 1, 1))), dev(np.tile(B, (reps, 1, 1, 1))))
    big.given.copy_(dev(np.random.default_rng(4).normal(0.0, 0.02, [batch, form.given_len])))
    res = big.run(3)
    assert not bool(torch.isnan(big.given).any()) and bool(torch.isfinite(big.given).all())
    assert res["status"].shape == (3, batch)
