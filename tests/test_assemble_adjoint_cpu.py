"""CPU: the derivative of the assembly with respect to ``given`` (mpcasm_assemble_jvp, mpcasm_assemble_vjp,
mpcasm_assemble_adjoint_info) as far as it goes without a device: the three entries are exported and bound, the info
entry answers for every case and refuses exactly what the launches refuse, the long-double reference equals the
dense composition of the formulas in include/mpcasm.h, and an fp64 restatement of the kernel's six steps from the
plan's tables (adjoint_restatement.py) stays within the yardstick of the GPU test."""
import ctypes
import os

import numpy as np
import pytest

import adjoint_cases as ac
import adjoint_reference as ar
import adjoint_restatement as rs
from helpers import LD, U64, assert_componentwise, cancellation_free_plants
from mpcasm import capi, engine, problems
from mpcasm.plan import compile_plan

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcasm.h")
ERR_PLAN = -2          # MPCASM_ERR_PLAN (include/mpcasm.h)
ENTRIES = ("mpcasm_assemble_jvp", "mpcasm_assemble_vjp", "mpcasm_assemble_adjoint_info")


def _plans(api):
    rng = np.random.default_rng(3)
    return {case.name: ac.compile_case(api, rng, case) for case in ac.CASES}


def _info(plan, strides=None):
    out = (ctypes.c_int32 * 4)()
    itab, dtab = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab)
    n = len(plan.sources)
    st = (ctypes.c_int64 * max(n, 1))(*(strides or [0] * n))
    rc = capi.load().mpcasm_assemble_adjoint_info(itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size, st, out)
    return rc, tuple(out)


def test_entries_are_declared_exported_and_bound():
    text = open(HEADER).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ENTRIES:
        assert name in text and hasattr(lib, name) and name in capi.SIGNATURES
    assert "body.py:266-302" in text and "body.py:236-264" in text and "dh = -cMg d" in text
    assert capi.load().mpcasm_abi_version() == 1004


def test_the_cases_hold_every_kind_of_record(cpu_api):
    ac.assert_coverage({name: plan for name, (_, plan) in _plans(cpu_api).items()})


def test_info_answers_for_every_case_without_a_device(cpu_api):
    plans = {name: plan for name, (_, plan) in _plans(cpu_api).items()}
    plans["body"] = compile_plan(problems.body_case(cpu_api))
    plans["biped"] = compile_plan(problems.biped(cpu_api, problems.BipedConfig(step_samples=8), reduced=True))
    plans["biped-lti"] = compile_plan(problems.biped(cpu_api, problems.BipedConfig(step_samples=8), reduced=True),
                                      lti=("LIP",))
    even = lambda n: n + (n & 1)
    for name, plan in plans.items():
        rc, (lds, whole, words, per_cu) = _info(plan)
        assert rc == 0, name
        it = plan.itab
        nbrow = int(it[it[rs.H["OFF_T_BROW0"]] + it[rs.H["NBASE"]]])
        rtot = int(it[rs.H["RTOT"]])
        # x | gh | y (yt in its place) | r | rho | the stream bases
        assert lds == 8 * (even(max(plan.ng, plan.no)) + even(plan.nc) + even(nbrow) + 2 * even(rtot) + 33), name
        assert whole == (lds > 64 * 1024) and words > 0 and per_cu == max(1, min(8, 160 * 1024 // lds))
        assert engine.adjoint_info(plan) == (lds, whole, words, per_cu)


def test_info_refuses_what_the_launches_refuse(cpu_api):
    import preview_cases as pc

    # a plan compiled with ltv=: no S, U
    ltv = compile_plan(problems.lipm_ltv(cpu_api, N=12), ltv=("LIP",))
    assert _info(ltv) == (capi.ERR_LIMIT, (0, 0, 0, 0))
    with pytest.raises(capi.MpcasmError):
        engine.adjoint_info(ltv)
    # one instance beyond a CU's LDS: 9 axes of 12 states over 160 steps are 18 828 base rows
    shape = pc._shape("beyond-lds", 12, 1, 160, 9, 0, 0)
    _, big = pc.compile_case(cpu_api, np.random.default_rng(1), shape)
    assert _info(big) == (capi.ERR_LIMIT, (0, 0, 0, 0))
    # ... and the same family well inside it
    _, small = pc.compile_case(cpu_api, np.random.default_rng(1), pc._shape("inside", 12, 1, 16, 2, 0, 0))
    assert _info(small)[0] == 0


def test_info_checks_its_arguments_and_the_tables(cpu_api):
    _, plan = ac.compile_case(cpu_api, np.random.default_rng(2), ac.CASES[0])
    lib = capi.load()
    itab, dtab = np.ascontiguousarray(plan.itab).copy(), np.ascontiguousarray(plan.dtab)
    out = (ctypes.c_int32 * 4)()
    strides = (ctypes.c_int64 * len(plan.sources))()
    args = (itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size)
    assert lib.mpcasm_assemble_adjoint_info(*args, strides, out) == 0
    assert lib.mpcasm_assemble_adjoint_info(*args, None, out) == capi.ERR_ARG          # sources, no strides
    assert lib.mpcasm_assemble_adjoint_info(*args, strides, None) == capi.ERR_ARG
    assert lib.mpcasm_assemble_adjoint_info(None, 0, None, 0, strides, out) == capi.ERR_ARG
    strides[0] = -8
    assert lib.mpcasm_assemble_adjoint_info(*args, strides, out) == capi.ERR_ARG
    strides[0] = 0
    assert lib.mpcasm_assemble_adjoint_info(itab.ctypes.data, 4, dtab.ctypes.data, dtab.size, strides, out) == ERR_PLAN
    # a corrupted table: a gterm that points past the workspace
    gt, _ = ac.records(plan)
    g = int(np.flatnonzero((gt[:, ac.GT_FLAGS] & ac.GT_FLAG_DIAG) == 0)[0])
    itab[int(itab[rs.H["OFF_GTERM"]]) + g * ac.GT_WORDS + ac.GT_DOFF] = int(itab[rs.H["RTOT"]]) + 7
    assert lib.mpcasm_assemble_adjoint_info(*args, strides, out) == ERR_PLAN
    assert tuple(out) == (0, 0, 0, 0)


@pytest.mark.parametrize("kind", ["mix", "diag", "body", "biped"])
def test_the_reference_is_the_dense_composition(cpu_api, kind):
    """J of adjoint_reference.jacobian (differences of the oracle's assemble) against J_q = sum s w cMo' cMg and
    J_h = -sum diag(arrow) cMg formed from the oracle's preview matrices: equal to long-double rounding of the
    magnitudes (the differences carry the rounding of the aims' terms too: 64 units of 2^-64 |q(0)|, |h(0)|)."""
    from oracle import qp_oracle as orc

    rng = np.random.default_rng(7)
    form = {"body": lambda: problems.body_case(cpu_api),
            "biped": lambda: problems.biped(cpu_api, problems.BipedConfig(step_samples=8), reduced=True)}.get(
                kind, lambda: ac.build(cpu_api, rng, kind))()
    ac.vary_params(form, rng)
    J = ar.jacobian(form)
    Jq, Jh = ar.dense_jacobian(form)
    _, h0, _, q0 = orc.assemble(form, np.zeros((form.given_len, 1)), dtype=LD, magnitude=True)
    eps = LD(2.0) ** -64
    assert J.Jq.shape == Jq.shape and J.Jh.shape == Jh.shape
    assert np.all(np.abs(J.Jq - Jq) <= 64 * eps * (J.Mq + np.abs(q0)))
    assert np.all(np.abs(J.Jh - Jh) <= 64 * eps * (J.Mh + np.abs(h0)))
    assert np.all(np.abs(J.Jq) <= J.Mq * (1 + 64 * eps) + 64 * eps * np.abs(q0))
    assert np.all(np.abs(J.Jh) <= J.Mh * (1 + 64 * eps) + 64 * eps * np.abs(h0))
    if kind == "mix":
        idle = ac.unread_given_columns(form)
        assert np.all(J.Mq[:, idle] == 0) and np.all(J.Mh[:, idle] == 0)
        assert np.any(J.Mq != 0) and np.any(J.Mh != 0)
    if kind == "diag":
        assert np.all(J.Mq == 0), "a cost on a free variable does not depend on given"


@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_the_restatement_of_the_six_steps_meets_the_yardstick(cpu_api, case):
    """adjoint_restatement.py (fp64, from the plan's tables) against the long-double reference, componentwise with
    the kappa of the GPU test, and its adjointness <gq, dq> + <gh, dh> = <ggiven, d>."""
    from oracle import qp_oracle as orc

    rng = np.random.default_rng(11)
    form, plan = ac.compile_case(cpu_api, rng, case)
    ac.vary_params(form, rng)
    params = plan.current_params()
    sources = ab = None
    if case.streams == "shared":
        J = ar.jacobian(form)
    else:
        A, B = (x[0] for x in cancellation_free_plants(rng, 1, ac.NS, ac.NI, 0.9, ac.N))
        if case.streams == "bound":
            S, U = orc.extend_matrices(ac.N, A, B)
            sources = ac.plant_sources(plan, S, U)
            J = ar.jacobian(form, "plant", tables=(S, U))
        else:
            ab = [(A, B)]
            J = ar.jacobian(form, "plant", plant=(A, B))
    kappa = ac.kappa(plan, generated=case.streams == "lti")
    d, gq, gh = rng.normal(size=plan.ng), rng.normal(size=plan.no), rng.normal(size=plan.nc)
    dq, dh = rs.jvp(plan, d, params, sources, ab)
    (dq_ref, dq_mag), (dh_ref, dh_mag) = ar.jvp_reference(J, d)
    assert_componentwise(dq, dq_ref, dq_mag, kappa, "dq")
    assert_componentwise(dh, dh_ref, dh_mag, kappa, "dh")
    for cq, ch in ((gq, gh), (gq, None), (None, gh)):
        gg = rs.vjp(plan, cq, ch, params, sources, ab)
        assert_componentwise(gg, *ar.vjp_reference(J, cq, ch), kappa, "ggiven")
    gg = rs.vjp(plan, gq, gh, params, sources, ab)
    mag = float(np.abs(gq) @ dq_mag + np.abs(gh) @ dh_mag + ar.vjp_reference(J, gq, gh)[1] @ np.abs(d))
    assert abs((gq @ dq + gh @ dh) - gg @ d) <= kappa * U64 * mag
    if case.kind == "diag":
        assert np.all(dq == 0)
    assert np.all(gg[ac.unread_given_columns(form)] == 0)
