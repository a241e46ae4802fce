"""Host restatement of the reference's walking loop for one walker  --  TEST INFRASTRUCTURE ONLY (the
checker of ``WalkerFleet.step``).

Per tick, as biped_mpc_loop.py:41-95 does it: ``oracle.qp_oracle.assemble`` at the walker's step times,
``osqp_restatement.solve`` (OSQP's rules, cold, its defaults), ``oracle.qp_oracle.preview`` of every
definition, then ``update_given_collector`` and ``arrange_given``; then the clock counts down.  What the
reference leaves open -- a QP that is not solved -- follows the fleet's ``on_unsolved`` rule: ``"hold"``
applies SOLVED and MAX_ITER solutions only, ``"apply"`` every one but NON_CVX."""
import numpy as np

import osqp_restatement as rs
from mpcasm import problems
from oracle import qp_oracle as orc

APPLIES = {"hold": (rs.SOLVED, rs.MAX_ITER),
           "apply": (rs.SOLVED, rs.MAX_ITER, rs.PRIMAL_INFEASIBLE, rs.DUAL_INFEASIBLE)}


def update_given(form, given, optim, PM=None):
    """The reference's preview_all + update_given_collector + arrange_given (biped_mpc_loop.py:54, 62-92):
    the next ``given`` (column vector) from this tick's ``given`` and solution."""
    maps = orc.qp_index_maps(form.domain, form.optim_variables)
    if PM is None:
        PM = orc.preview_matrices(form, maps)
    given, optim = np.asarray(given).reshape(-1, 1), np.asarray(optim).reshape(-1, 1)
    motion = {v: orc.preview(PM, given, optim, v) for v in form.definitions}
    for state, ID in form.dynamics["LIP"].state_ID.items():
        motion["x0" + state[-2:]][ID] = motion[state][0]
    for state, ID in form.dynamics["steps"].state_ID.items():
        motion["s0" + state[-2:]][ID] = motion[state][1]
    for variable, size in form.dynamics["bias"].domain.items():
        motion[variable] = np.zeros([size, 1])
    return orc.arrange_given(maps, motion)


def rest_given(form, conf):
    """The reference's start (biped_mpc_loop.py:26-33): everything at zero but x0_y[0] = s0_y[0] = strt_y."""
    given = np.zeros(form.given_len)
    for var in ("x0_y", "s0_y"):
        given[form.given_ID[var][0]] = conf.strt_y
    return given


class HostWalker:
    """One walker of the reference's loop, ``phase`` ticks into its step cycle, on ``form`` (a biped
    formulation; shared between walkers: it is re-pointed at each walker's step times per tick)."""

    def __init__(self, form, conf, phase, policy="hold"):
        self.form, self.conf, self.policy = form, conf, policy
        self.clock = problems.StepClock(conf.step_samples, conf.num_steps)
        for _ in range(phase):
            self.clock.tick()

    def solve(self, given, step_times=None, step_count=None):
        """This tick's QP at ``given`` (the walker's clock, or the step times given): ``(solution, next
        given)``; the next given is ``given`` itself where the rule holds the walker."""
        st = self.clock.step_times if step_times is None else step_times
        sc = self.clock.step_count if step_count is None else step_count
        self.form.update(step_times=np.array(st), step_count=int(sc))
        A, h, Q, q = orc.assemble(self.form, np.asarray(given).reshape(-1, 1))
        sol = rs.solve(Q, q, A, h)
        if sol.status in APPLIES[self.policy]:
            return sol, update_given(self.form, given, sol.x).ravel()
        return sol, np.array(given, dtype=np.float64).ravel()

    def tick(self, given):
        sol, nxt = self.solve(given)
        self.clock.tick()
        return sol, nxt


def host_loop(form, conf, phase, ticks, policy="hold"):
    """``ticks`` ticks of one walker from rest: ``(statuses, iterations, givens (ticks + 1, ng), margin)``."""
    walker = HostWalker(form, conf, phase, policy)
    given = rest_given(form, conf)
    status, iters, trail, margin = [], [], [given], np.inf
    for _ in range(ticks):
        sol, given = walker.tick(given)
        status.append(sol.status)
        iters.append(sol.iters)
        trail.append(given)
        margin = min(margin, sol.margin)
    return np.array(status), np.array(iters), np.array(trail), margin
