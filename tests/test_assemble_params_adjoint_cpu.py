"""CPU: the derivative of the assembly with respect to the parameters (mpcasm_assemble_params_vjp,
mpcasm_assemble_params_vjp_info) as far as it goes without a device: the two entries are exported and bound, the info
entry answers for every case and refuses exactly what the launch refuses, the long-double reference
(params_adjoint_reference.py: differences of the oracle's assemble) equals an independent dense composition of the
formulas in include/mpcasm.h, and an fp64 restatement of the kernel's steps and of its parameter index from the plan's
tables (params_adjoint_restatement.py) stays within the yardstick of the GPU test."""
import ctypes
import os

import numpy as np
import pytest

import adjoint_cases as ac
import adjoint_reference as ar
import params_adjoint_cases as pac
import params_adjoint_reference as pr
import params_adjoint_restatement as prs
from helpers import LD, assert_componentwise, cancellation_free_plants
from mpcasm import capi, engine, problems
from mpcasm.plan import compile_plan

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcasm.h")
ERR_PLAN = -2          # MPCASM_ERR_PLAN (include/mpcasm.h)
ENTRIES = ("mpcasm_assemble_params_vjp", "mpcasm_assemble_params_vjp_info")


def _plans(api):
    rng = np.random.default_rng(3)
    return {case.name: ac.compile_case(api, rng, case) for case in ac.CASES}


def _info(plan, strides=None):
    out = (ctypes.c_int32 * 4)()
    itab, dtab = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab)
    n = len(plan.sources)
    st = (ctypes.c_int64 * max(n, 1))(*(strides or [0] * n))
    rc = capi.load().mpcasm_assemble_params_vjp_info(itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size, st, out)
    return rc, tuple(out)


def _vectors(rng, plan):
    """``given, x, u, y, w`` of one instance; some rows of ``y`` and ``w`` zero (``w`` wherever ``y`` is)."""
    given, x, u = rng.normal(size=plan.ng), rng.normal(size=plan.no), rng.normal(size=plan.no)
    y, w = np.abs(rng.normal(size=plan.nc)), rng.normal(size=plan.nc)
    off = rng.random(plan.nc) < 0.4
    y[off], w[off] = 0.0, 0.0
    return given, x, u, y, w


def test_entries_are_declared_exported_and_bound():
    text = open(HEADER).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ENTRIES:
        assert name in text and hasattr(lib, name) and name in capi.SIGNATURES
    for formula in ("gP = -1/2 (u x' + x u')", "g[arrow_Ri]  += -(y_R r_u[row] + w_R r_x[row])", "g[extreme_R] += w_R",
                    "g[ap] += s t[wp] sum_k r_u[a+k]"):
        assert formula in text, formula
    assert capi.load().mpcasm_abi_version() == 1004


def test_the_cases_hold_every_kind_of_record(cpu_api):
    pac.assert_coverage({name: plan for name, (_, plan) in _plans(cpu_api).items()})
    pac.assert_centres_coverage(compile_plan(pac.build_centres(cpu_api, np.random.default_rng(5))))


def test_info_answers_for_every_case_without_a_device(cpu_api):
    plans = {name: plan for name, (_, plan) in _plans(cpu_api).items()}
    plans["centres"] = compile_plan(pac.build_centres(cpu_api, np.random.default_rng(5)))
    plans["body"] = compile_plan(problems.body_case(cpu_api))
    plans["biped"] = compile_plan(problems.biped(cpu_api, problems.BipedConfig(step_samples=8), reduced=True))
    plans["biped-lti"] = compile_plan(problems.biped(cpu_api, problems.BipedConfig(step_samples=8), reduced=True),
                                      lti=("LIP",))
    even = lambda n: n + (n & 1)
    for name, plan in plans.items():
        rc, (lds, whole, words, per_cu) = _info(plan)
        assert rc == 0, name
        it = plan.itab
        nbrow = int(it[it[prs.H["OFF_T_BROW0"]] + it[prs.H["NBASE"]]])
        rtot = int(it[prs.H["RTOT"]])
        # x, u | given | y, w | the base rows | r_x, r_u, r_g | the stream bases
        assert lds == 8 * (2 * even(plan.no) + even(plan.ng) + 2 * even(plan.nc) + even(nbrow) + 3 * even(rtot) + 33)
        assert whole == (lds > 64 * 1024) and per_cu == max(1, min(8, 160 * 1024 // lds))
        # a pointer per slot and at least one record of eight words for every slot some record names
        named = int(np.count_nonzero(pac.contributions(plan)))
        assert words >= len(plan.params) + 1 + 8 * named and named > 0, name
        assert words == len(plan.params) + 1 + (-(len(plan.params) + 1) % 4) + \
            8 * sum(len(r) for r in prs.parameter_index(plan)), name
        assert engine.params_adjoint_info(plan) == (lds, whole, words, per_cu)
        assert lds >= engine.adjoint_info(plan).lds


def test_info_refuses_what_the_launch_refuses(cpu_api):
    import preview_cases as pc

    ltv = compile_plan(problems.lipm_ltv(cpu_api, N=12), ltv=("LIP",))
    assert _info(ltv) == (capi.ERR_LIMIT, (0, 0, 0, 0))
    with pytest.raises(capi.MpcasmError):
        engine.params_adjoint_info(ltv)
    _, big = pc.compile_case(cpu_api, np.random.default_rng(1), pc._shape("beyond-lds", 12, 1, 160, 9, 0, 0))
    assert _info(big) == (capi.ERR_LIMIT, (0, 0, 0, 0))
    _, small = pc.compile_case(cpu_api, np.random.default_rng(1), pc._shape("inside", 12, 1, 16, 2, 0, 0))
    assert _info(small)[0] == 0


def test_info_checks_its_arguments_and_the_tables(cpu_api):
    _, plan = ac.compile_case(cpu_api, np.random.default_rng(2), ac.CASES[0])
    lib = capi.load()
    itab, dtab = np.ascontiguousarray(plan.itab).copy(), np.ascontiguousarray(plan.dtab)
    out = (ctypes.c_int32 * 4)()
    strides = (ctypes.c_int64 * len(plan.sources))()
    args = (itab.ctypes.data, itab.size, dtab.ctypes.data, dtab.size)
    assert lib.mpcasm_assemble_params_vjp_info(*args, strides, out) == 0
    assert lib.mpcasm_assemble_params_vjp_info(*args, None, out) == capi.ERR_ARG
    assert lib.mpcasm_assemble_params_vjp_info(*args, strides, None) == capi.ERR_ARG
    assert lib.mpcasm_assemble_params_vjp_info(None, 0, None, 0, strides, out) == capi.ERR_ARG
    strides[0] = -8
    assert lib.mpcasm_assemble_params_vjp_info(*args, strides, out) == capi.ERR_ARG
    strides[0] = 0
    # a corrupted table: a gterm whose rows start past the workspace
    gt, _ = ac.records(plan)
    g = int(np.flatnonzero((gt[:, ac.GT_FLAGS] & ac.GT_FLAG_DIAG) == 0)[0])
    itab[int(itab[prs.H["OFF_GTERM"]]) + g * ac.GT_WORDS + ac.GT_AOFF] = int(itab[prs.H["RTOT"]]) + 7
    assert lib.mpcasm_assemble_params_vjp_info(*args, strides, out) == ERR_PLAN
    assert tuple(out) == (0, 0, 0, 0)


def _form(api, rng, kind):
    if kind == "body":
        return problems.body_case(api)
    if kind == "centres":
        return pac.build_centres(api, rng)
    return ac.build(api, rng, kind)


@pytest.mark.parametrize("kind", ["mix", "diag", "centres", "body"])
def test_the_reference_is_the_dense_composition(cpu_api, kind):
    """g* of params_adjoint_reference.vjp_reference (differences of the oracle's assemble, contracted with the dense
    cotangents) against the formulas of include/mpcasm.h composed per Cost and Constraint from the oracle's preview
    matrices: equal to long-double rounding -- 64 roundings behind an element of the assembly (as
    test_assemble_adjoint_cpu.py counts them) and one per element contracted, in units of 2^-64 of the column's
    magnitude plus the magnitude of the whole assembly against the same cotangents (the differences carry the rounding
    of every other term)."""
    from oracle import qp_oracle as orc

    rng = np.random.default_rng(7)
    form = _form(cpu_api, rng, kind)
    plan = compile_plan(form)
    ac.vary_params(form, rng)
    given, x, u, y, w = _vectors(rng, plan)
    J = pr.jacobian(form, plan, given)
    ref, mag = pr.vjp_reference(J, x, u, y, w)
    dense, dense_mag = pr.dense_gradient(form, plan, given, x, u, y, w)
    G, h, Pm, q = orc.assemble(form, np.reshape(given, (-1, 1)), dtype=LD, magnitude=True)
    _, cot = pr.cotangents(x, u, y, w)
    whole = np.sum(cot[0] * Pm) + cot[1] @ q.ravel() + np.sum(cot[2] * G) + cot[3] @ h.ravel()
    eps = LD(2.0) ** -64
    units = 64 + plan.no * plan.no + plan.nc * plan.no + plan.no + plan.nc
    assert ref.shape == dense.shape == (len(plan.params),)
    assert np.all(np.abs(ref - dense) <= units * eps * (2 * mag + whole))
    assert np.all(np.abs(mag - dense_mag) <= units * eps * (2 * mag + whole))
    assert np.all(np.abs(ref) <= mag * (1 + units * eps) + units * eps * whole)
    assert np.any(mag != 0) and float(np.max(np.abs(ref))) > 0
    # the columns as differences of the WHOLE assemble: the same, up to the rounding the other terms leave behind
    Jw = pr.jacobian(form, plan, given, whole=True)
    ref_w, mag_w = pr.vjp_reference(Jw, x, u, y, w)
    assert np.all(np.abs(ref - ref_w) <= units * eps * (2 * mag + whole))
    assert np.all(np.abs(mag - mag_w) <= units * eps * (2 * mag + whole))
    if kind == "mix":
        assert np.count_nonzero(mag) > len(mag) // 2


def _sources(api, rng, form, plan, streams):
    """One instance's sources for the restatement and for the reference."""
    from oracle import qp_oracle as orc

    if streams == "shared":
        return {}, {}
    A, B = (x[0] for x in cancellation_free_plants(rng, 1, ac.NS, ac.NI, 0.9, ac.N))
    if streams == "bound":
        S, U = orc.extend_matrices(ac.N, A, B)
        return dict(sources=ac.plant_sources(plan, S, U)), dict(name="plant", tables=(S, U))
    return dict(ab=[(A, B)]), dict(name="plant", plant=(A, B))


@pytest.mark.parametrize("name", ac.IDS + ["centres"])
def test_the_restatement_meets_the_yardstick(cpu_api, name):
    """params_adjoint_restatement.py (fp64, from the plan's tables) against the long-double reference, componentwise
    with the kappa of the GPU test; exact zeros where the magnitude is zero."""
    rng = np.random.default_rng(11)
    if name == "centres":
        form, streams = pac.build_centres(cpu_api, rng), "shared"
        plan = compile_plan(form)
    else:
        case = ac.CASES[ac.IDS.index(name)]
        (form, plan), streams = ac.compile_case(cpu_api, rng, case), case.streams
    ac.vary_params(form, rng)
    params = plan.current_params()
    mine, theirs = _sources(cpu_api, rng, form, plan, streams)
    given, x, u, y, w = _vectors(rng, plan)
    J = pr.jacobian(form, plan, given, **theirs)
    ref, mag = pr.vjp_reference(J, x, u, y, w)
    got = prs.params_vjp(plan, given, x, u, y, w, params, **mine)
    kappa = pac.kappa(plan, generated=streams == "lti")
    assert_componentwise(got, ref, mag, kappa, name)
    assert np.count_nonzero(mag) > 0
    # the rows of y and w that are zero: nothing of those lines reaches an extreme of its own
    unnamed = pac.contributions(plan) == 0
    assert not got[unnamed].any()
