"""CPU: what mpcasm_qp_polish_wide decides without a device -- the LDS of a workgroup, the workspace and the
workgroups of a launch by the header's formulas, the size limit, the argument errors -- and the premises of
tests/test_gpu_qp_polish_wide.py on the restatements: on its shapes the plain instances are polished to exactly
the constructed active set, the one with a wrong set is rejected, and no decision is near a tie."""
import ctypes

import numpy as np
import pytest

import osqp_restatement as rs
import polish_restatement as pr
import polish_wide_cases as cases

LIMIT = 156 * 1024
CAP = 512
GRID = [(1, 1), (5, 3), (36, 76), (63, 66), (64, 70), (65, 300), (96, 196), (129, 140), (130, 0), (200, 404),
        (257, 260), (384, 1536), (512, 520), (512, 2048)]
BATCHES = [0, 1, 7, 511, 512, 513, 2 * 512 + 3, 8192]


def lds_doubles(no, nc):
    """include/mpcasm.h: 14 vectors of no (the partial sums of four wavefronts among them), 4 of nc, 16 for the
    reductions, the active rows as int32, rounded up to even."""
    n = 14 * no + 4 * nc + 16 + (no + 1) // 2
    return n + (n & 1)


def slice_doubles(no):
    """include/mpcasm.h: three no x no matrices, rounded up to even."""
    n = 3 * no * no
    return n + (n & 1)


# ---- the library, without a device -----------------------------------------------------------------------------
@pytest.mark.parametrize("no,nc", GRID)
def test_info_is_the_headers_formulas(no, nc):
    from mpcasm import capi, engine

    assert capi.POLISH_WIDE_CAP == CAP
    for batch in BATCHES:
        lds, work, groups = engine.qp_polish_wide_info(no, nc, batch)
        assert lds == 8 * lds_doubles(no, nc) <= LIMIT
        assert groups == min(batch, CAP)
        assert work == 8 * groups * slice_doubles(no)          # by the workgroups, not by the batch
    assert engine.qp_polish_wide_info(no, nc, 8192)[1] == engine.qp_polish_wide_info(no, nc, CAP)[1]


def test_fewer_workgroups_by_the_environment(monkeypatch):
    from mpcasm import engine

    monkeypatch.setenv("MPCASM_QP_POLISH_WIDE_GROUPS", "256")
    assert engine.qp_polish_wide_info(96, 196, 4096)[1:] == (256 * 8 * slice_doubles(96), 256)
    assert engine.qp_polish_wide_info(96, 196, 100)[2] == 100
    for outside in ("0", "513", "many"):
        monkeypatch.setenv("MPCASM_QP_POLISH_WIDE_GROUPS", outside)
        assert engine.qp_polish_wide_info(96, 196, 4096)[2] == CAP


def test_c4_at_8192_instances_stays_within_a_couple_of_gb():
    from mpcasm import engine

    assert engine.qp_polish_wide_info(384, 1536, 8192)[1] == 512 * 3 * 384 * 384 * 8 < 2 * 2 ** 30


@pytest.mark.parametrize("no", [1, 63, 64, 65, 129, 257, 512])
@pytest.mark.parametrize("nc", [0, 1, 2048])
def test_everything_the_wide_solve_takes_is_accepted(no, nc):
    from mpcasm import capi, engine

    assert engine.qp_polish_wide_info(no, nc, 3)[2] == 3
    assert engine.qp_solve_wide_info(no, nc)[0] <= LIMIT
    # ... and the call gets past the limit to the workspace check (no workspace: refused there, before any device)
    rc = capi.load().mpcasm_qp_polish_wide(no, nc, 16, 16, 16, 16, 16, 16, 16, None, 1e-6, 3, 16, None, 3, None, 0,
                                           None)
    assert rc == capi.ERR_ARG


@pytest.mark.parametrize("no,nc", [(513, 4), (513, 0), (512, 3133), (96, 4641), (1, 4985)])
def test_err_limit_beyond_the_limit(no, nc):
    from mpcasm import capi, engine

    assert no > 512 or 8 * lds_doubles(no, nc) > LIMIT
    with pytest.raises(capi.MpcasmError) as err:
        engine.qp_polish_wide_info(no, nc, 4)
    assert err.value.status == capi.ERR_LIMIT
    lds, work, groups = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    lib = capi.load()
    assert lib.mpcasm_qp_polish_wide_info(no, nc, 4, ctypes.byref(lds), ctypes.byref(work),
                                          ctypes.byref(groups)) == capi.ERR_LIMIT
    assert lds.value == 8 * lds_doubles(no, nc) and groups.value == 4      # (the outputs still written)
    # the call itself refuses before it touches a device (the pointers are never read)
    rc = lib.mpcasm_qp_polish_wide(no, nc, 16, 16, 16, 16, 16, 16, 16, None, 1e-6, 3, 16, None, 4, 16, 1 << 40, None)
    assert rc == capi.ERR_LIMIT


def test_the_largest_instances_that_fit():
    from mpcasm import capi, engine

    assert engine.qp_polish_wide_info(512, 3132, 1)[0] <= LIMIT
    assert engine.qp_polish_wide_info(96, 4640, 1)[0] <= LIMIT
    for no, nc in ((512, 3133), (96, 4641)):
        with pytest.raises(capi.MpcasmError):
            engine.qp_polish_wide_info(no, nc, 1)


def test_argument_errors_are_decided_before_any_device_call():
    from mpcasm import capi, engine

    lib = capi.load()
    need = engine.qp_polish_wide_info(96, 196, 5)[1]
    good = dict(no=96, nc=196, P=16, q=16, G=16, h=16, x=16, y=16, z=16, status=None, delta=1e-6, refine=3,
                polish=16, res=None, batch=5, work=4096, bytes=need)
    order = ("no", "nc", "P", "q", "G", "h", "x", "y", "z", "status", "delta", "refine", "polish", "res", "batch",
             "work", "bytes")

    def call(**change):
        args = dict(good, **change)
        return lib.mpcasm_qp_polish_wide(*[args[k] for k in order], None)

    for delta in (0.0, -1e-6, float("nan"), float("inf")):
        assert call(delta=delta) == capi.ERR_ARG, delta
    assert call(refine=-1) == capi.ERR_ARG
    assert call(batch=-1) == capi.ERR_ARG
    assert call(no=0) == capi.ERR_ARG and call(nc=-1) == capi.ERR_ARG
    for name in ("P", "q", "G", "h", "x", "y", "z", "polish"):
        assert call(**{name: None}) == capi.ERR_ARG, name
    # the workspace: null, not on 16 bytes, a byte short
    assert call(work=None) == capi.ERR_ARG
    for work in (4096 + 8, 4096 + 1, 4096 + 4):
        assert call(work=work) == capi.ERR_ARG, work
    assert call(bytes=need - 1) == capi.ERR_ARG and call(bytes=0) == capi.ERR_ARG
    # (the need follows the workgroups: what five instances take is short for six, enough for 513 at 512's)
    assert call(batch=6) == capi.ERR_ARG
    # batch == 0 answers ok, whatever the pointers, and without a device
    assert call(batch=0) == capi.OK
    assert call(batch=0, P=None, polish=None, work=None, bytes=0) == capi.OK
    assert call(nc=0, G=None, h=None, y=None, z=None, batch=0) == capi.OK
    out64, out32 = ctypes.c_int64(), ctypes.c_int32()
    a, b, c = ctypes.byref(out64), ctypes.byref(out64), ctypes.byref(out32)
    assert lib.mpcasm_qp_polish_wide_info(0, 3, 1, a, b, c) == capi.ERR_ARG
    assert lib.mpcasm_qp_polish_wide_info(5, -1, 1, a, b, c) == capi.ERR_ARG
    assert lib.mpcasm_qp_polish_wide_info(5, 3, -1, a, b, c) == capi.ERR_ARG
    for hole in range(3):
        args = [a, b, c]
        args[hole] = None
        assert lib.mpcasm_qp_polish_wide_info(5, 3, 1, *args) == capi.ERR_ARG


def test_the_python_entry_points_are_there():
    import inspect

    from mpcasm import engine
    from mpcasm.ltv_loop import LtvLoop

    assert list(inspect.signature(engine.polish_qp_wide).parameters)[:5] == ["P", "q", "G", "h", "sol_or_xyz"]
    assert "work" in inspect.signature(engine.polish_qp_wide).parameters
    assert inspect.signature(engine.solve_qp_wide).parameters["polish"].default is False
    names = list(inspect.signature(LtvLoop.__init__).parameters)
    assert names[-2:] == ["polish", "solver_kwargs"]
    assert inspect.signature(LtvLoop.__init__).parameters["polish"].default is False


# ---- the premises of the GPU test, on the restatements ----------------------------------------------------------
def premises(qp, constructed, plain, wrong):
    P, q, G, h = qp
    no, nc = P.shape[1], G.shape[1]
    worst = np.inf
    for b in list(plain) + ([wrong] if wrong is not None else []):
        sol = rs.solve(P[b], q[b], G[b], h[b])
        assert sol.status == rs.SOLVED, b
        y = sol.y
        if b == wrong:
            guess = (h[b] - sol.z) < sol.y
            y, row = pr.wrong_active_set(h[b], sol.y, sol.z, guess)
        out = pr.polish(P[b], q[b], G[b], h[b], sol.x, y, sol.z, status=sol.status)
        assert out.margin >= 1e-6, (b, out.margins)
        worst = min(worst, out.margin)
        if b == wrong:
            assert out.polish == pr.REJECTED and out.active[row] and not constructed[b][row], b
            assert int(out.active.sum()) == int(constructed[b].sum()) + 1 <= no
        else:
            assert out.polish == pr.DONE and np.array_equal(out.active, constructed[b]), b
            assert out.margins["active"] >= 0.5
    return worst


@pytest.mark.parametrize("no,nc,na", cases.SHAPES, ids=cases.IDS(cases.SHAPES))
def test_the_restatements_verdicts_on_the_gpu_tests_shapes(no, nc, na):
    """Instances 0 to 3 of every shape from osqp_restatement.solve's iterate: DONE with exactly the constructed
    active set on the plain ones, REJECTED on the one with a wrong set (where the shape has an inactive row to
    call active), every margin at least 1e-6."""
    full = cases.problem(no, nc, na)
    worst = premises(full[:4], full[4], cases.PLAIN, cases.WRONG if na < nc else None)
    print("qp-polish-wide-cpu: (%d, %d, %d) worst margin %.1e" % (no, nc, na, worst))


def test_the_restatements_verdicts_on_the_largest_shape():
    full = cases.largest()
    worst = premises(full[:4], full[4], (0, 1), 2)
    print("qp-polish-wide-cpu: %r worst margin %.1e" % (cases.LARGEST, worst))
