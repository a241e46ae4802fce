"""GPU: the order of a closed tick's launches, for both loops on the one solve stage (mpcasm/solve_stage.py).

``mpcasm.capi.load`` is replaced by a proxy that logs the name of every entry called and calls through; per tick the
log, without the host-only size queries (``*_info``, ``*_bytes``) and the set-up of a loop's first tick (SETUP), must be
exactly the sequence written out below -- the table of mpcasm/ltv_loop.py's module docstring and, per structure
bucket, ``WalkerFleet._closed_bucket``'s.  Beside the order: the stage's buffers stay where they are from tick to tick,
and a tick's results carry the keys they always had."""
import numpy as np
import pytest

import augment_cases as ac
import rollout_cases as rc
from mpcasm import capi, problems

pytestmark = pytest.mark.gpu
SOFT = (1e3, 0.0)
OPTIONS = {"plain": {}, "polish": dict(polish=True), "warm": dict(warm=True),
           "warm+polish": dict(warm=True, polish=True), "soft": dict(soft=SOFT),
           "warm+soft": dict(warm=True, soft=SOFT)}
# entries of a loop's first tick that launch nothing: the tables of a bucket's given map, compiled with its stage, and
# of the LTV plan's rows, compiled (sized, then written) ahead of the first advance or true_inputs
SETUP = {"mpcasm_given_map_compile", "mpcasm_ltv_rollout_compile"}

# Eight walkers, one per place of a step cycle of 8: every tick the bucket with one step in the preview holds the one
# walker whose step was just taken (one shift group: it came from the other bucket), the bucket with two holds the
# other seven (two shift groups: six that stay and the one that came over) -- one mpcasm_qp_warm_start per group.
FLEET_TICK = {
    "plain": ["mpcasm_assemble_indexed", "mpcasm_qp_solve", "mpcasm_next_given",
              "mpcasm_assemble_indexed", "mpcasm_qp_solve", "mpcasm_next_given"],
    "polish": ["mpcasm_assemble_indexed", "mpcasm_qp_solve", "mpcasm_qp_polish", "mpcasm_next_given",
               "mpcasm_assemble_indexed", "mpcasm_qp_solve", "mpcasm_qp_polish", "mpcasm_next_given"],
    "warm": ["mpcasm_assemble_indexed", "mpcasm_qp_warm_start", "mpcasm_qp_solve", "mpcasm_qp_warm_store",
             "mpcasm_next_given",
             "mpcasm_assemble_indexed", "mpcasm_qp_warm_start", "mpcasm_qp_warm_start", "mpcasm_qp_solve",
             "mpcasm_qp_warm_store", "mpcasm_next_given"],
    "warm+polish": ["mpcasm_assemble_indexed", "mpcasm_qp_warm_start", "mpcasm_qp_solve", "mpcasm_qp_polish",
                    "mpcasm_qp_warm_store", "mpcasm_next_given",
                    "mpcasm_assemble_indexed", "mpcasm_qp_warm_start", "mpcasm_qp_warm_start", "mpcasm_qp_solve",
                    "mpcasm_qp_polish", "mpcasm_qp_warm_store", "mpcasm_next_given"],
    "soft": ["mpcasm_assemble_indexed", "mpcasm_qp_solve_soft", "mpcasm_next_given",
             "mpcasm_assemble_indexed", "mpcasm_qp_solve_soft", "mpcasm_next_given"],
    "warm+soft": ["mpcasm_assemble_indexed", "mpcasm_qp_warm_start", "mpcasm_qp_solve_soft", "mpcasm_qp_warm_store",
                  "mpcasm_next_given",
                  "mpcasm_assemble_indexed", "mpcasm_qp_warm_start", "mpcasm_qp_warm_start", "mpcasm_qp_solve_soft",
                  "mpcasm_qp_warm_store", "mpcasm_next_given"],
}
FLEET_KEYS = {"plain": {"p", "index", "x", "status", "iters"},
              "polish": {"p", "index", "x", "status", "iters", "polish"},
              "warm": {"p", "index", "x", "status", "iters", "warm"},
              "warm+polish": {"p", "index", "x", "status", "iters", "polish", "warm"},
              "soft": {"p", "index", "x", "status", "iters"},
              "warm+soft": {"p", "index", "x", "status", "iters", "warm"}}

# ltv_loop.py's table: assemble, [warm start], solve, [polish], [warm store], [true inputs], advance
LTV_TICK = {
    "plain": ["mpcasm_assemble", "mpcasm_qp_solve_wide", "mpcasm_ltv_advance"],
    "polish": ["mpcasm_assemble", "mpcasm_qp_solve_wide", "mpcasm_qp_polish_wide", "mpcasm_ltv_advance"],
    "warm": ["mpcasm_assemble", "mpcasm_qp_warm_start", "mpcasm_qp_solve_wide", "mpcasm_qp_warm_store",
             "mpcasm_ltv_advance"],
    "warm+polish": ["mpcasm_assemble", "mpcasm_qp_warm_start", "mpcasm_qp_solve_wide", "mpcasm_qp_polish_wide",
                    "mpcasm_qp_warm_store", "mpcasm_ltv_advance"],
    "soft": ["mpcasm_assemble", "mpcasm_qp_solve_wide_soft", "mpcasm_ltv_advance"],
    "warm+soft": ["mpcasm_assemble", "mpcasm_qp_warm_start", "mpcasm_qp_solve_wide_soft", "mpcasm_qp_warm_store",
                  "mpcasm_ltv_advance"],
}
LTV_KEYS = {"plain": {"x", "status", "iters"}, "polish": {"x", "status", "iters", "polish"},
            "warm": {"x", "status", "iters", "warm"}, "warm+polish": {"x", "status", "iters", "polish", "warm"},
            "soft": {"x", "status", "iters"}, "warm+soft": {"x", "status", "iters", "warm"}}


class LoggedLibrary:
    """The loaded library with every ``mpcasm_*`` entry's name appended to ``log`` when it is called."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        entry = getattr(self._lib, name)
        if not name.startswith("mpcasm_"):
            return entry

        def call(*args):
            self._log.append(name)
            return entry(*args)
        return call


@pytest.fixture
def entry_log(gpu_api, monkeypatch):
    log, lib = [], capi.load()
    monkeypatch.setattr(capi, "load", lambda: LoggedLibrary(lib, log))
    return log


def launches(log):
    """The log of one tick without the host-only queries and the set-up; the log is emptied."""
    kept = [name for name in log if not name.endswith(("_info", "_bytes")) and name not in SETUP]
    del log[:]
    return kept


def addresses(stage):
    return {k: t.data_ptr() for k, t in stage.buffers.items()}


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("option", list(OPTIONS))
def test_the_fleet_s_tick(gpu_api, entry_log, option, graphs):
    """Eight walkers (the fleet of test_eight_walkers_walk_like_the_host_loop), ``2 * step_samples + 1`` ticks.
    Eager: every tick is FLEET_TICK.  With graphs a place's first tick runs as it is and is then captured -- the
    sequence twice -- and the last tick, the first place again, is a replay: nothing is called."""
    from mpcasm.walkers import WalkerFleet

    conf = problems.BipedConfig(step_samples=8)
    fleet = WalkerFleet(8, phases=np.arange(8), conf=conf, api=gpu_api, graphs=graphs, **OPTIONS[option])
    fleet.start_at_rest()
    del entry_log[:]
    where = None
    for tick in range(2 * conf.step_samples + 1):
        out = fleet.step()
        want = FLEET_TICK[option] * (2 if graphs else 1) if tick < 2 * conf.step_samples or not graphs else []
        got = launches(entry_log)
        assert got == want, (option, graphs, tick, got)
        assert [entry["p"] for entry in out] == [1, 2] and all(set(entry) == FLEET_KEYS[option] for entry in out)
        stages = [fleet.buckets[entry["p"]]["stage"] for entry in out]
        for entry, stage in zip(out, stages):
            assert all(entry[k].data_ptr() == stage.buffers[k].data_ptr() for k in FLEET_KEYS[option] - {"p", "index"})
        now = [addresses(stage) for stage in stages]
        assert where is None or now == where, (option, graphs, tick)
        where = now


@pytest.mark.parametrize("mode", ["open", "feedback", "true_input"])
@pytest.mark.parametrize("option", list(OPTIONS))
def test_the_ltv_loop_s_tick(gpu_api, entry_log, option, mode):
    """rollout_cases.loop_inputs at LOOP_BATCH, three ticks; with ``feedback`` mpcasm_ltv_true_inputs goes in front of
    the advance and the results carry ``u``, ``true_input`` (on the plan augmented by its input) changes no launch."""
    import torch

    from mpcasm.ltv_loop import LtvLoop

    kw, want, keys = dict(OPTIONS[option]), list(LTV_TICK[option]), set(LTV_KEYS[option])
    if mode == "true_input":
        form, A, B, given = ac.loop_inputs(gpu_api, N=rc.LOOP_N, T=rc.LOOP_T)
    else:
        form, A, B, given = rc.loop_inputs(gpu_api)
    if mode != "open":
        Q, R = problems.lipm_feedback_weights()
        kw.update(feedback={"Q": Q, "R": R}, true_input=mode == "true_input")
        want.insert(len(want) - 1, "mpcasm_ltv_true_inputs")
        keys.add("u")
    dev = lambda v: torch.as_tensor(np.array(v, order="C"), device="cuda")
    loop = LtvLoop(form, "LIP", rc.LOOP_BATCH, dev(A), dev(B), **kw)
    loop.given.copy_(dev(given))
    del entry_log[:]
    where = addresses(loop.stage)
    for tick in range(3):
        out = loop.step()
        got = launches(entry_log)
        assert got == want, (option, mode, tick, got)
        assert set(out) == keys
        assert all(out[k].data_ptr() == loop.stage.buffers[k].data_ptr() for k in keys - {"u"})
        assert addresses(loop.stage) == where, (option, mode, tick)
