"""CPU: mpcasm_qp_solve_wide_info (no device needed) -- the LDS an instance of the wide solve takes, where
its K^-1 lives, and the size limit include/mpcasm.h states."""
import pytest

from mpcasm import capi, engine

LIMIT = 156 * 1024


def lds_doubles(no, nc, on_chip):
    """The header's count: 3 nc + 23 no + 64 doubles, + no (no | 1) with K^-1 on chip, rounded up to even."""
    n = 3 * nc + 23 * no + 64 + (no * (no | 1) if on_chip else 0)
    return n + (n & 1)


@pytest.mark.parametrize("no,nc,on_chip", [(36, 76, True), (96, 196, True), (200, 404, False),
                                           (384, 1536, False), (512, 2048, False), (7, 0, True)])
def test_info_of_the_baseline_shapes(monkeypatch, no, nc, on_chip):
    monkeypatch.delenv("MPCASM_QP_WIDE_KINV", raising=False)
    lds, on = engine.qp_solve_wide_info(no, nc)
    assert on == on_chip
    assert lds == 8 * lds_doubles(no, nc, on) <= LIMIT
    # K^-1 on chip exactly where it fits beside the vectors
    assert on == (8 * lds_doubles(no, nc, True) <= LIMIT)


def test_the_environment_moves_k_inverse(monkeypatch):
    monkeypatch.setenv("MPCASM_QP_WIDE_KINV", "global")
    assert engine.qp_solve_wide_info(96, 196) == (8 * lds_doubles(96, 196, False), False)
    monkeypatch.setenv("MPCASM_QP_WIDE_KINV", "lds")
    assert engine.qp_solve_wide_info(96, 196) == (8 * lds_doubles(96, 196, True), True)
    assert engine.qp_solve_wide_info(200, 404)[1] is False    # (does not fit: stays in d_kinv)


@pytest.mark.parametrize("no,nc", [(513, 1), (512, 2710), (1, 6628)])
def test_err_limit_just_past_the_limit(monkeypatch, no, nc):
    monkeypatch.delenv("MPCASM_QP_WIDE_KINV", raising=False)
    with pytest.raises(capi.MpcasmError) as err:
        engine.qp_solve_wide_info(no, nc)
    assert err.value.status == capi.ERR_LIMIT
    # one less is admitted
    engine.qp_solve_wide_info(no - 1 if no == 513 else no, nc - 1 if no != 513 else nc)


def test_bad_arguments_and_the_lds_path_unchanged():
    import ctypes

    lds, on = ctypes.c_int64(), ctypes.c_int32()
    lib = capi.load()
    assert lib.mpcasm_qp_solve_wide_info(0, 4, ctypes.byref(lds), ctypes.byref(on)) == -1
    assert lib.mpcasm_qp_solve_wide_info(4, -1, ctypes.byref(lds), ctypes.byref(on)) == -1
    assert lib.mpcasm_qp_solve_wide_info(4, 4, None, ctypes.byref(on)) == -1
    assert lib.mpcasm_abi_version() == 1004
    # the LDS path still refuses C3
    with pytest.raises(capi.MpcasmError) as err:
        engine.qp_solve_lds_bytes(96, 196)
    assert err.value.status == capi.ERR_LIMIT
