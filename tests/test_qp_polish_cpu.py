"""CPU: the polishing step restated (tests/polish_restatement.py) -- that it recovers constructed solutions to
rounding, takes each of its status paths, and pays on the biped's own loop -- and what mpcasm_qp_polish decides
without a device: the LDS an instance takes, the size limit, the argument errors."""
import ctypes

import numpy as np
import pytest

import osqp_restatement as rs
import polish_restatement as pr
import solver_reference as sr
from helpers import LD

LIMIT = 156 * 1024
BIPED_SHAPES = [(34, 72), (36, 76), (50, 104), (52, 108)]
TEST_SHAPES = [(5, 3), (7, 12), (36, 76), (65, 70), (33, 100), (5, 12)]


def lds_doubles(no, nc):
    """include/mpcasm.h: four matrices of no (no | 1), 13 vectors of no, 4 of nc, 16 for the reductions, the
    active rows as int32, rounded up to even."""
    n = 4 * no * (no | 1) + 13 * no + 4 * nc + 16 + (no + 1) // 2
    return n + (n & 1)


def solved(no, nc, na):
    """A complementary QP of the shape and its cold solve at OSQP's defaults (the iterate a polish starts from)."""
    rng = np.random.default_rng([no, nc, na])
    P, q, G, h, xs, ys, active = pr.complementary_qp(rng, no, nc, na)
    sol = rs.solve(P, q, G, h)
    assert sol.status == rs.SOLVED
    return (P, q, G, h), (xs, ys, active), sol


# ---- the restatement: accuracy ---------------------------------------------------------------------------------
@pytest.mark.parametrize("no,nc,na", pr.SHAPES)
@pytest.mark.parametrize("dtype", [np.float64, LD], ids=["fp64", "long double"])
def test_the_constructed_solution_comes_back_to_rounding(no, nc, na, dtype):
    """DONE, exactly the constructed active set, and x^ and both residuals (recomputed in long double) within the
    componentwise rounding magnitudes of solver_reference.res_bounds on the polished point: (no + 2) u Mp for
    |G x^ - z^|, (no + nc + 2) u Md for |P x^ + q + G'y^| -- and for |x^ - x*|, which the stationarity equation
    determines: x* solves the fp64 QP only up to the rounding of q = -(P x* + G'y*), a sum of that magnitude."""
    qp, (xs, ys, active), sol = solved(no, nc, na)
    cold = float(np.abs(sol.x - xs).max())
    out = pr.polish(*qp, sol.x, sol.y, sol.z, status=sol.status, dtype=dtype)
    assert out.polish == pr.DONE
    assert np.array_equal(out.active, active)
    assert out.margins["active"] >= 0.5, out.margins
    assert out.margin >= 1e-6, out.margins
    x, y, z = (np.asarray(v, dtype=np.float64) for v in (out.x, out.y, out.z))
    rp, rd, Mp, Md = sr.residuals(*qp[:3], x, y, z)
    bp, bd = sr.res_bounds(no, nc, Mp, Md)
    err = sr.err_inf(x, xs)
    print("qp-polish-cpu: %-11s (%d, %d, %d)  cold |x - x*| %.1e  polished %.1e  r_p %.1e (bound %.1e)  r_d %.1e (bound %.1e)"
          % (np.dtype(dtype).name, no, nc, na, cold, err, rp, bp, rd, bd))
    assert rp <= bp and rd <= bd, (rp, bp, rd, bd)
    assert err <= bd, (err, bd)
    assert err < cold
    assert (y[~active] == 0).all() and (y[active] > 0).all()
    assert np.array_equal(z, np.minimum(z, qp[3]))


# ---- the restatement: status paths --------------------------------------------------------------------------------
def same_bits(out, x, y, z):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in ((out.x, x), (out.y, y), (out.z, z)))


@pytest.mark.parametrize("no,nc,na", pr.SHAPES[1:])
def test_a_wrong_active_set_is_rejected(no, nc, na):
    """One inactive row called active: the KKT system forces it, its multiplier comes out negative.  (At a vertex,
    na = no, the extra row makes na > no: skipped.)"""
    qp, (xs, ys, active), sol = solved(no, nc, na)
    y, row = pr.wrong_active_set(qp[3], sol.y, sol.z, active)
    out = pr.polish(*qp, sol.x, y, sol.z, status=sol.status)
    assert out.active[row] and not active[row] and int(out.active.sum()) == na + 1
    assert out.polish == (pr.REJECTED if na < no else pr.SKIPPED) and out.res is None
    assert same_bits(out, sol.x, y, sol.z)
    assert out.margin >= 1e-6, out.margins


def test_more_active_rows_than_unknowns_is_skipped():
    qp, _, sol = solved(5, 12, 3)
    y = (qp[3] - sol.z) + 1.0          # every row passes the test
    out = pr.polish(*qp, sol.x, y, sol.z, status=sol.status)
    assert out.active.all() and out.polish == pr.SKIPPED and out.res is None
    assert same_bits(out, sol.x, y, sol.z)


@pytest.mark.parametrize("status", [rs.MAX_ITER, rs.PRIMAL_INFEASIBLE, rs.DUAL_INFEASIBLE, rs.NON_CVX])
def test_an_instance_that_is_not_solved_is_skipped(status):
    qp, _, sol = solved(5, 3, 2)
    nan = np.full(5, np.nan), np.full(3, np.nan), np.full(3, np.nan)
    for x, y, z in ((sol.x, sol.y, sol.z), nan):
        out = pr.polish(*qp, x, y, z, status=status)
        assert out.polish == pr.SKIPPED and out.active is None and same_bits(out, x, y, z)
    # without a status the NaN iterate is read: every comparison fails, nothing changes
    out = pr.polish(*qp, *nan)
    assert out.polish == pr.REJECTED and same_bits(out, *nan)


def test_no_active_row_is_the_unconstrained_minimum():
    qp, (xs, ys, active), sol = solved(5, 3, 0)
    out = pr.polish(*qp, sol.x, sol.y, sol.z, status=sol.status)
    assert out.polish == pr.DONE and not out.active.any()
    ref = -np.linalg.solve(qp[0], qp[1])
    assert np.abs(out.x - ref).max() <= 16 * np.finfo(float).eps * np.abs(ref).max() * np.linalg.cond(qp[0])
    assert not out.y.any()


def test_a_matrix_that_is_not_positive_definite_is_rejected():
    qp, _, sol = solved(5, 3, 2)
    P = qp[0].copy()
    P[2, 2] = -1.0
    out = pr.polish(P, *qp[1:], sol.x, sol.y, sol.z)
    assert out.polish == pr.REJECTED and same_bits(out, sol.x, sol.y, sol.z)


# ---- the restatement on the biped's own loop ------------------------------------------------------------------------
def test_the_biped_loop_is_polished(cpu_api):
    """The host loop of the biped (N = 16), phases 0 and 3, 14 ticks: every QP solved at OSQP's defaults, polished,
    and compared with the same QP solved to 1e-9.  At least 20 of the 28 ticks are accepted; every accepted point is
    within 1e-5 of the tight solution; and on at least 20 accepted ticks ADMM's own point is more than 1e-3 away."""
    from fleet_loop_reference import HostWalker, rest_given
    from mpcasm import problems
    from oracle import qp_oracle as orc

    conf = problems.BipedConfig(step_samples=8)
    form = problems.biped(cpu_api, conf)
    done = rejected = skipped = far = 0
    worst, lines = 0.0, []
    for phase in (0, 3):
        walker = HostWalker(form, conf, phase)
        given = rest_given(form, conf)
        for tick in range(14):
            form.update(step_times=np.array(walker.clock.step_times), step_count=int(walker.clock.step_count))
            G, h, P, q = orc.assemble(form, given.reshape(-1, 1))
            q, h = q.ravel(), h.ravel()
            sol, given = walker.tick(given)
            assert sol.status == rs.SOLVED
            tight = rs.solve(P, q, G, h, eps_abs=1e-9, eps_rel=1e-9, max_iter=200000)
            assert tight.status == rs.SOLVED
            out = pr.polish(P, q, G, h, sol.x, sol.y, sol.z, status=sol.status)
            before, after = (float(np.abs(v - tight.x).max()) for v in (sol.x, out.x))
            lines.append("phase %d tick %2d  (%d, %d)  na %2d  %-8s |x - x_tight| %.1e -> %.1e  margin %.1e"
                         % (phase, tick, P.shape[0], G.shape[0], int(out.active.sum()),
                            {1: "DONE", 0: "SKIPPED", -1: "REJECTED"}[out.polish], before, after, out.margin))
            if out.polish == pr.DONE:
                done += 1
                far += before > 1e-3
                worst = max(worst, after)
                assert after <= 1e-5, lines[-1]
                assert (out.y >= 0).all()
            else:
                rejected += out.polish == pr.REJECTED
                skipped += out.polish == pr.SKIPPED
                assert np.array_equal(out.x, sol.x)
    print("\n".join(lines))
    print("qp-polish-cpu: biped loop, 28 ticks: %d DONE, %d REJECTED, %d SKIPPED; worst accepted |x - x_tight| %.1e; "
          "%d accepted ticks had ADMM's point more than 1e-3 away" % (done, rejected, skipped, worst, far))
    assert done >= 20 and far >= 20, (done, far)


# ---- the library, without a device -------------------------------------------------------------------------------
@pytest.mark.parametrize("no,nc", BIPED_SHAPES + TEST_SHAPES)
def test_lds_bytes_is_the_headers_formula(no, nc):
    from mpcasm import engine

    assert engine.qp_polish_lds_bytes(no, nc) == 8 * lds_doubles(no, nc) <= LIMIT


@pytest.mark.parametrize("no,nc", [(96, 196), (70, 70), (68, 100)])
def test_err_limit_beyond_the_limit(no, nc):
    from mpcasm import capi, engine

    assert 8 * lds_doubles(no, nc) > LIMIT
    with pytest.raises(capi.MpcasmError) as err:
        engine.qp_polish_lds_bytes(no, nc)
    assert err.value.status == capi.ERR_LIMIT
    # ... and the call itself refuses before it touches a device (the pointers are never read)
    lib = capi.load()
    rc = lib.mpcasm_qp_polish(no, nc, 8, 8, 8, 8, 8, 8, 8, None, 1e-6, 3, 8, None, 1, None)
    assert rc == capi.ERR_LIMIT


def test_the_largest_instances_that_fit():
    from mpcasm import capi, engine

    assert engine.qp_polish_lds_bytes(68, 1) <= LIMIT        # 4 * 68 * 69 doubles and the vectors
    assert engine.qp_polish_lds_bytes(68, 66) <= LIMIT
    with pytest.raises(capi.MpcasmError):
        engine.qp_polish_lds_bytes(69, 1)
    with pytest.raises(capi.MpcasmError):
        engine.qp_polish_lds_bytes(68, 67)


def test_argument_errors_are_decided_before_any_device_call():
    from mpcasm import capi

    lib = capi.load()
    good = dict(no=5, nc=3, P=8, q=8, G=8, h=8, x=8, y=8, z=8, status=None, delta=1e-6, refine=3, polish=8, res=None,
                batch=1)
    order = ("no", "nc", "P", "q", "G", "h", "x", "y", "z", "status", "delta", "refine", "polish", "res", "batch")

    def call(**change):
        args = dict(good, **change)
        return lib.mpcasm_qp_polish(*[args[k] for k in order], None)

    for delta in (0.0, -1e-6, float("nan"), float("inf")):
        assert call(delta=delta) == capi.ERR_ARG, delta
    assert call(refine=-1) == capi.ERR_ARG
    assert call(batch=-1) == capi.ERR_ARG
    assert call(no=0) == capi.ERR_ARG and call(nc=-1) == capi.ERR_ARG
    for name in ("P", "q", "G", "h", "x", "y", "z", "polish"):
        assert call(**{name: None}) == capi.ERR_ARG, name
    # without limits G, h, y, z may be null: only then
    assert call(nc=0, G=None, h=None, y=None, z=None, batch=0) == capi.OK
    # batch == 0 answers ok, whatever the pointers, and without a device
    assert call(batch=0) == capi.OK
    assert call(batch=0, P=None, polish=None) == capi.OK
    out = ctypes.c_int64()
    assert lib.mpcasm_qp_polish_lds_bytes(0, 3, ctypes.byref(out)) == capi.ERR_ARG
    assert lib.mpcasm_qp_polish_lds_bytes(5, -1, ctypes.byref(out)) == capi.ERR_ARG
    assert lib.mpcasm_qp_polish_lds_bytes(5, 3, None) == capi.ERR_ARG


def test_the_verdicts_of_the_binding_are_the_headers():
    from mpcasm import capi, engine

    assert (capi.POLISH_DONE, capi.POLISH_SKIPPED, capi.POLISH_REJECTED) == (pr.DONE, pr.SKIPPED, pr.REJECTED) == (1, 0, -1)
    # without polish a solution is the seven fields it always was, and says so; with it, one more at the end
    plain = engine.QpSolution(*range(7))
    assert plain.polish is None and len(plain) == 7 and engine.QpSolution._fields[-1] == "rho"
    polished = engine.PolishedQpSolution(*plain, 7)
    assert polished.polish == 7 and polished[:7] == tuple(plain) and engine.PolishedQpSolution._fields[-1] == "polish"
