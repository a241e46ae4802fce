"""GPU: the steered fleet (WalkerFleet(..., commands=True)): bit for bit the plain fleet while nobody commands
it, and under changing commands -- and a weight edited on the buckets' assemblers -- the host restatement of the
reference's loop (tests/fleet_loop_reference.py) on formulations that carry each walker's commands.  The yardstick
is test_gpu_fleet_loop.py's: equal verdicts and iterations, rows of `given` to 1e-9 of the row tick by tick; a
walker whose solve decides within 1e-6 of a tie is not judged."""
import numpy as np
import pytest

from fleet_loop_reference import HostWalker, rest_given
from mpcasm import capi, problems
from mpcasm.walkers import COMMAND_COLUMNS, WalkerFleet

pytestmark = pytest.mark.gpu
MARGIN = 1e-6
JERK = ("cost", "minimize jerk", "weight")


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def per_row(dev, ref, rtol):
    """max |dev - ref| <= rtol max |ref| in every row (last axis); the worst offender alongside."""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(dev - ref).max(axis=-1) - rtol * np.abs(ref).max(axis=-1)
    i = np.unravel_index(int(np.argmax(err)), err.shape) if err.size else ()
    return bool((err <= 0).all()), (i, float(np.abs(dev[i] - ref[i]).max()), float(np.abs(ref[i]).max()))


class HostForms:
    """Biped formulations that carry a walker's commands (a configuration with ``target_vel`` and
    ``stepping_center`` set so) and a jerk weight, built once per distinct pair."""

    def __init__(self, api):
        self.api, self.forms = api, {}

    def get(self, commands, jerk_weight=None):
        key = (tuple(float(c) for c in commands), jerk_weight)
        if key not in self.forms:
            conf = problems.BipedConfig(step_samples=8)
            conf.target_vel = np.array([key[0][0], key[0][1], 0.0])
            conf.stepping_center = np.array([key[0][2], key[0][3]])
            form = problems.biped(self.api, conf)
            if jerk_weight is not None:
                form.goals["minimize jerk"].update(weight=jerk_weight)
            self.forms[key] = (form, conf)
        return self.forms[key]


def default_commands(conf):
    return np.array([conf.target_vel[0], conf.target_vel[1], conf.stepping_center[0], conf.stepping_center[1]])


# ---- 9. nobody commands: the plain fleet, bit for bit -----------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_untouched_commands_walk_like_the_plain_fleet(gpu_api, torch_gpu, graphs, warm):
    torch = torch_gpu
    conf = problems.BipedConfig(step_samples=8)
    kw = dict(phases=np.arange(8), conf=conf, api=gpu_api, graphs=graphs, warm=warm)
    plain, steered = WalkerFleet(8, **kw), WalkerFleet(8, commands=True, **kw)
    assert plain.commands is None and tuple(steered.commands.shape) == (8, len(COMMAND_COLUMNS))
    assert np.array_equal(steered.commands.cpu().numpy(), np.tile(default_commands(conf), (8, 1)))
    plain.start_at_rest()
    steered.start_at_rest()
    a, b = plain.run(16, record=True), steered.run(16, record=True)
    for k in ("status", "iters", "given"):
        assert torch.equal(a[k], b[k]), k
    assert int((a["status"] == capi.QP_SOLVED).sum()) > 0.8 * a["status"].numel()
    # no parameters are kept per place of the cycle, and the plain fleet still keeps its own
    assert all(item["params"] is None for entry in steered._cache.values() for item in entry)
    assert all(item["params"] is not None for entry in plain._cache.values() for item in entry)


# ---- 10. teacher-forced, the value gate ---------------------------------------------------------------------
def test_64_walkers_under_changing_commands_tick_by_tick(gpu_api, torch_gpu):
    """64 walkers (phases b % 8), 24 ticks; at ticks 8 and 16 a random half draws new commands, at tick 5 the jerk
    weight doubles on both buckets' assemblers.  8 sampled walkers per tick and each bucket's first and last,
    every one against HostWalker.solve from the device's own row before the tick, on a form with the walker's
    commands and the weight."""
    conf = problems.BipedConfig(step_samples=8)
    B, ticks = 64, 24
    fleet = WalkerFleet(B, phases=np.arange(B) % 8, conf=conf, api=gpu_api, on_unsolved="hold", commands=True)
    given = fleet.start_at_rest()
    forms = HostForms(gpu_api)
    rng, pick_rng = np.random.default_rng(11), np.random.default_rng(5)
    commands = np.tile(default_commands(conf), (B, 1))
    weight = None
    samples = checked = 0
    for tick in range(ticks):
        if tick in (8, 16):
            half = np.sort(rng.choice(B, B // 2, replace=False))
            commands[half, 0] = rng.uniform(0.0, 0.6, half.size)
            commands[half, 1] = rng.uniform(-0.05, 0.05, half.size)
            commands[half, 2] = rng.uniform(0.0, 0.1, half.size)
            commands[half, 3] = 0.28 + rng.uniform(-0.02, 0.02, half.size)
            fleet.set_commands(commands[half], walkers=half)
        if tick == 5:
            weight = 2 * conf.cost_weights["minimize jerk"]
            for bucket in fleet.buckets.values():
                bucket["asm"].set_param(*JERK, weight)
        assert np.array_equal(fleet.commands.cpu().numpy(), commands)
        pre = given.cpu().numpy()
        times, counts = fleet.clock.step_times.copy(), fleet.clock.step_count.copy()
        out = fleet.step()
        post = given.cpu().numpy()
        pick = set(pick_rng.choice(B, 8, replace=False).tolist())
        per_walker = {}
        for entry in out:
            ids = entry["index"].cpu().numpy()
            pick.update((int(ids[0]), int(ids[-1])))
            st, it = entry["status"].cpu().numpy(), entry["iters"].cpu().numpy()
            for row, b in enumerate(ids):
                per_walker[int(b)] = (int(st[row]), int(it[row]))
        assert sorted(per_walker) == list(range(B))
        for b in sorted(pick):
            samples += 1
            form, conf_b = forms.get(commands[b], weight)
            sol, nxt = HostWalker(form, conf_b, 0, "hold").solve(pre[b], times[b], counts[b])
            print("tick %2d walker %2d  status %2d iters %4d  margin %.3g" % (tick, b, sol.status, sol.iters, sol.margin))
            if sol.margin <= MARGIN:
                continue
            checked += 1
            assert per_walker[b] == (sol.status, sol.iters), (tick, b, per_walker[b], sol.status, sol.iters)
            ok, worst = per_row(post[b], nxt, 1e-9)
            assert ok, (tick, b, worst)
    print("samples %d, checked %d" % (samples, checked))
    assert checked >= 0.9 * samples, (checked, samples)


# ---- 11. the free run ---------------------------------------------------------------------------------------------
FREE_TICKS = 40


def free_run_schedule(conf):
    """tick -> the (8, 4) commands from that tick on."""
    mid = np.stack([np.array([0.6, 0.3, 0.0, 0.45, 0.2, 0.6, 0.1, 0.5]),
                    np.array([0.0, 0.05, -0.05, 0.0, 0.02, 0.0, 0.0, -0.03]),
                    np.array([0.0, 0.05, 0.0, 0.1, 0.0, 0.02, 0.0, 0.0]),
                    0.28 + np.array([0.0, 0.02, -0.02, 0.0, 0.01, 0.0, 0.0, 0.0])], axis=1)
    return {0: np.tile(default_commands(conf), (8, 1)), 12: mid, 26: np.tile([0.25, 0.0, 0.05, 0.28], (8, 1))}


def free_run(torch, api, conf, **kw):
    fleet = WalkerFleet(8, phases=np.arange(8), conf=conf, api=api, commands=True, **kw)
    fleet.start_at_rest()
    schedule = free_run_schedule(conf)
    starts = sorted(schedule) + [FREE_TICKS]
    status, iters, trail = [], [], []
    for t0, t1 in zip(starts[:-1], starts[1:]):
        if t0:
            fleet.set_commands(schedule[t0])
        res = fleet.run(t1 - t0, record=True)
        status.append(res["status"])
        iters.append(res["iters"])
        trail.append(res["given"] if not trail else res["given"][1:])
    return torch.cat(status), torch.cat(iters), torch.cat(trail)


@pytest.fixture(scope="module")
def free_runs():
    return {}


def eager_run(free_runs, torch, api, conf, warm):
    if warm not in free_runs:
        free_runs[warm] = free_run(torch, api, conf, warm=warm)
    return free_runs[warm]


def test_eight_steered_walkers_walk_like_eight_host_loops(gpu_api, torch_gpu, free_runs):
    conf = problems.BipedConfig(step_samples=8)
    status, iters, trail = (t.cpu().numpy() for t in eager_run(free_runs, torch_gpu, gpu_api, conf, False))
    assert status.shape == (FREE_TICKS, 8) and trail.shape[0] == FREE_TICKS + 1
    schedule, forms = free_run_schedule(conf), HostForms(gpu_api)
    com_x = forms.get(schedule[0][0])[0].given_ID["x0_x"][0]
    for phase in range(8):
        form, conf_b = forms.get(schedule[0][phase])
        walker = HostWalker(form, conf_b, phase, "hold")
        given = rest_given(form, conf)
        st, it, tr, margin = [], [], [given], np.inf
        for t in range(FREE_TICKS):
            if t in schedule:
                walker.form, walker.conf = forms.get(schedule[t][phase])
            sol, given = walker.tick(given)
            st.append(sol.status)
            it.append(sol.iters)
            tr.append(given)
            margin = min(margin, sol.margin)
        assert margin > MARGIN, (phase, margin)
        assert np.array_equal(status[:, phase], st), (phase, status[:, phase], st)
        assert np.array_equal(iters[:, phase], it), (phase, iters[:, phase], it)
        ok, worst = per_row(trail[:, phase], np.array(tr), 1e-8)
        print("phase %d  margin %.3g  worst row %r" % (phase, margin, worst))
        assert ok, (phase, worst)
    # the commands act: the walkers told to go fast and those told to stand end far apart
    final = trail[-1, :, com_x]
    assert final.max() - final.min() > 0.1, final


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_steered_graphs_replay_their_eager_run(gpu_api, torch_gpu, free_runs, warm):
    torch = torch_gpu
    conf = problems.BipedConfig(step_samples=8)
    eager = eager_run(free_runs, torch, gpu_api, conf, warm)
    graphs = free_run(torch, gpu_api, conf, warm=warm, graphs=True)
    for name, a, b in zip(("status", "iters", "given"), eager, graphs):
        assert torch.equal(a, b), name
