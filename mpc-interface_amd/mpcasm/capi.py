"""ctypes binding of libmpcasm.so (C ABI declared in include/mpcasm.h).

The library is built in-tree by ``make -C mpc-interface_amd`` (or
``__graft_entry__.build()``) into this directory.  Loading fails loudly when it
is missing: there is no Python or CPU fallback for the kernels.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MPCASM_LIB: another build of the library, for A/B measurements)
LIB_PATH = os.environ.get("MPCASM_LIB") or os.path.join(_HERE, "libmpcasm.so")

OK = 0
ERR_LIMIT = -5
OPT_PATH = 1
OPT_PHASE_MASK = 2
OPT_RESIDENT_PER_CU = 3
OPT_RESIDENT_GRID = 6
OPT_P_DIRECT = 5     # the persistent kernel writes P 1: straight to HBM, 2: through LDS when it fits, 0: by the launch's size (read at plan creation)
OPT_JIT_FETCH_RUNS = 7  # test aid: chunks of the fetch tables with more runs stay on the table path (0 .. 8)
OPT_JIT = 4            # 0: specialise the persistent kernel for batches >= 512, 1: always, 2: never
PHASE_DEFAULT = 0xBF   # every phase on, cycle stamps (bit 6) off
PHASE_STAMPS = 0x40
STATUS = {
    0: "MPCASM_OK",
    -1: "MPCASM_ERR_ARG",
    -2: "MPCASM_ERR_PLAN",
    -3: "MPCASM_ERR_HIP",
    -4: "MPCASM_ERR_NODEVICE",
    -5: "MPCASM_ERR_LIMIT",
}
# per-instance outcomes of mpcasm_qp_solve (OSQP's values; written on the device, not return codes)
QP_SOLVED, QP_MAX_ITER, QP_PRIMAL_INFEASIBLE, QP_DUAL_INFEASIBLE, QP_NON_CVX = 1, -2, -3, -4, -7
QP_STATUS = {
    1: "MPCASM_QP_SOLVED",
    -2: "MPCASM_QP_MAX_ITER",
    -3: "MPCASM_QP_PRIMAL_INFEASIBLE",
    -4: "MPCASM_QP_DUAL_INFEASIBLE",
    -7: "MPCASM_QP_NON_CVX",
}
# per-instance outcomes of mpcasm_qp_polish
POLISH_DONE, POLISH_SKIPPED, POLISH_REJECTED = 1, 0, -1
POLISH_WIDE_CAP = 512          # MPCASM_POLISH_WIDE_CAP: the most workgroups of one mpcasm_qp_polish_wide launch
POLISH_STATUS = {1: "MPCASM_POLISH_DONE", 0: "MPCASM_POLISH_SKIPPED", -1: "MPCASM_POLISH_REJECTED"}
# per-instance outcomes of mpcasm_qp_sens
SENS_DONE, SENS_SKIPPED, SENS_SINGULAR = 1, 0, -1
SENS_STATUS = {1: "MPCASM_SENS_DONE", 0: "MPCASM_SENS_SKIPPED", -1: "MPCASM_SENS_SINGULAR"}
ROLL_GIVEN, ROLL_OPTIM, ROLL_STATE, ROLL_REC_WORDS = 0, 1, 2, 8   # records of mpcasm_ltv_rollout_compile
ERR_ARG = -1
# mpcasm_fill_route: out[0] and the flags of out[2]
FILL_QUAD, FILL_TINY, FILL_LTI, FILL_LTV_ROW, FILL_LTV_BLOCK, FILL_LTV_WAVE, FILL_LTV = 1, 2, 3, 4, 5, 6, 7
FILL_GENERIC, FILL_PAD, FILL_WHOLE_LINES = 1, 2, 4
GIVEN_KEEP, GIVEN_CONST = -1, -2     # given-map records of mpcasm_given_map_compile (a row: its index >= 0)
PMAP_SIGNED, PMAP_CONST = 1, 2       # flags of a parameter-map record (mpcasm_params_map)


def qp_bit(status):
    """Bit of ``status`` (a ``QP_*`` value) in the ``apply_mask`` of ``mpcasm_next_given``."""
    return 1 << abs(int(status))

# every symbol include/mpcasm.h declares: name -> (restype, argtypes)
_c_double_p = ctypes.POINTER(ctypes.c_double)
_void_p = ctypes.c_void_p
_int32_p, _int64_p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
# the argument runs many entries open with: a plan's host tables (h_itab, n_itab, h_dtab, n_dtab); a plan and its
# sources (plan, h_src, h_src_stride); everything the four mpcasm_qp_solve* entries take up to and including `stream`
_TABLES = [_void_p, ctypes.c_size_t, _void_p, ctypes.c_size_t]
_PLAN_SRC = [_void_p, ctypes.POINTER(_void_p), _int64_p]
_QP_SOLVE = ([ctypes.c_int, ctypes.c_int] + [_void_p] * 7 + [ctypes.c_int, _void_p] + [ctypes.c_double] * 6 +
             [ctypes.c_int] * 3 + [_void_p] * 3 + [ctypes.c_int, _void_p, ctypes.c_int, _void_p])
_QP_SOFT = [_void_p, _void_p, ctypes.c_int64]
SIGNATURES = {
    "mpcasm_abi_version": (ctypes.c_int, []),
    "mpcasm_device_count": (ctypes.c_int, []),
    "mpcasm_last_hip": (ctypes.c_int, []),
    "mpcasm_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "mpcasm_set_option": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "mpcasm_fill_su": (ctypes.c_int, [_void_p, _void_p, _void_p, _void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                       ctypes.c_int, ctypes.c_int, _void_p]),
    "mpcasm_fill_route": (ctypes.c_int, [ctypes.c_int] * 6 + [_int32_p]),
    "mpcasm_plan_create": (ctypes.c_int, _TABLES + [ctypes.POINTER(_void_p)]),
    "mpcasm_plan_destroy": (ctypes.c_int, [_void_p]),
    "mpcasm_resident_lds_bytes": (ctypes.c_int, _TABLES + [_int64_p]),
    "mpcasm_jit_check": (ctypes.c_int, _TABLES + [ctypes.c_char_p, ctypes.c_size_t]),
    "mpcasm_fetch_segments": (ctypes.c_int, _TABLES + [ctypes.c_int, _void_p, ctypes.c_size_t, _int64_p]),
    "mpcasm_preview_route": (ctypes.c_int, _TABLES + [_int64_p, ctypes.c_int, ctypes.c_int, _int32_p]),
    "mpcasm_sweep_route": (ctypes.c_int, _TABLES + [_int32_p]),
    "mpcasm_tiled_route": (ctypes.c_int, _TABLES + [_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _int32_p]),
    "mpcasm_assemble_route": (ctypes.c_int, _TABLES + [ctypes.c_int] * 4 + [_int32_p]),
    "mpcasm_staged_route": (ctypes.c_int, _TABLES + [ctypes.c_int] * 3 + [_int32_p]),
    "mpcasm_plan_sizes": (ctypes.c_int, [_void_p, _int64_p]),
    "mpcasm_plan_csc_sizes": (ctypes.c_int, [_void_p, _int64_p]),
    "mpcasm_plan_set_option": (ctypes.c_int, [_void_p, ctypes.c_int, ctypes.c_int]),
    "mpcasm_assemble_indexed": (ctypes.c_int, _PLAN_SRC + [_void_p] * 8 + [ctypes.c_int, _void_p]),
    "mpcasm_plan_last_kernel": (ctypes.c_int, [_void_p]),
    "mpcasm_plan_prepare": (ctypes.c_int, [_void_p, ctypes.c_int]),
    "mpcasm_jit_stats": (ctypes.c_int, [_int64_p]),
    "mpcasm_workspace_bytes": (ctypes.c_int, [_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "mpcasm_assemble": (ctypes.c_int, _PLAN_SRC + [_void_p] * 7 + [ctypes.c_int, _void_p]),
    "mpcasm_preview_matrices": (ctypes.c_int, _PLAN_SRC + [_void_p, ctypes.c_int, _void_p]),
    "mpcasm_preview": (ctypes.c_int, [_void_p, _void_p, _void_p, _void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                       ctypes.c_int, _void_p]),
    "mpcasm_preview_direct": (ctypes.c_int, _PLAN_SRC + [_void_p, _void_p, _void_p, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_assemble_jvp": (ctypes.c_int, _PLAN_SRC + [_void_p] * 5 + [ctypes.c_int, _void_p]),
    "mpcasm_assemble_vjp": (ctypes.c_int, _PLAN_SRC + [_void_p] * 5 + [ctypes.c_int, _void_p]),
    "mpcasm_assemble_adjoint_info": (ctypes.c_int, _TABLES + [_int64_p, _int32_p]),
    "mpcasm_assemble_params_vjp": (ctypes.c_int, _PLAN_SRC + [_void_p] * 9 + [ctypes.c_int, _void_p]),
    "mpcasm_assemble_params_vjp_info": (ctypes.c_int, _TABLES + [_int64_p, _int32_p]),
    "mpcasm_goal_distance": (ctypes.c_int, [_void_p, ctypes.c_int64, _void_p, ctypes.c_int64, _void_p, ctypes.c_int,
                             ctypes.c_int, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_preview_goal_distance": (ctypes.c_int, _PLAN_SRC + [_void_p, _void_p, _void_p, _void_p, ctypes.c_int,
                                     ctypes.c_int, _void_p, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_admm": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_void_p] * 8 + [ctypes.c_double] * 3 +
                    [ctypes.c_int, ctypes.c_int, ctypes.c_int, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_qp_solve": (ctypes.c_int, _QP_SOLVE),
    "mpcasm_qp_solve_lds_bytes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _int64_p]),
    "mpcasm_qp_solve_wide": (ctypes.c_int, _QP_SOLVE),
    "mpcasm_qp_solve_wide_info": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _int64_p, _int32_p]),
    "mpcasm_qp_solve_soft": (ctypes.c_int, _QP_SOLVE + _QP_SOFT),
    "mpcasm_qp_solve_soft_lds_bytes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _int64_p]),
    "mpcasm_qp_solve_wide_soft": (ctypes.c_int, _QP_SOLVE + _QP_SOFT),
    "mpcasm_qp_solve_wide_soft_info": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _int64_p, _int32_p]),
    "mpcasm_qp_polish": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_void_p] * 8 + [ctypes.c_double, ctypes.c_int,
                         _void_p, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_qp_polish_lds_bytes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _int64_p]),
    "mpcasm_qp_polish_wide": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_void_p] * 8 + [ctypes.c_double,
                              ctypes.c_int, _void_p, _void_p, ctypes.c_int, _void_p, ctypes.c_size_t, _void_p]),
    "mpcasm_qp_polish_wide_info": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _int64_p, _int64_p,
                                   _int32_p]),
    "mpcasm_qp_sens": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_void_p] * 9 + [ctypes.c_double, ctypes.c_int] +
                       [_void_p] * 6 + [ctypes.c_int, _void_p]),
    "mpcasm_qp_sens_lds_bytes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _int64_p]),
    "mpcasm_qp_sens_wide": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_void_p] * 9 + [ctypes.c_double,
                            ctypes.c_int] + [_void_p] * 6 + [ctypes.c_int, _void_p, ctypes.c_size_t, _void_p]),
    "mpcasm_qp_sens_wide_info": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _int64_p, _int64_p,
                                 _int32_p]),
    "mpcasm_qp_warm_store": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_void_p] * 4 + [ctypes.c_int] + [_void_p] *
                             4 + [ctypes.c_int64, ctypes.c_int, ctypes.c_int, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_qp_warm_start": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_void_p] * 6 + [ctypes.c_int64,
                             ctypes.c_int, ctypes.c_int] + [_void_p] * 3 + [ctypes.c_int, ctypes.c_uint32,
                             ctypes.c_double] + [_void_p] * 5 + [ctypes.c_int, _void_p]),
    "mpcasm_params_map": (ctypes.c_int, [_void_p, ctypes.c_int64, _void_p, _void_p, ctypes.c_int, _void_p,
                          ctypes.c_int64, ctypes.c_int, _void_p, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_given_map_compile": (ctypes.c_int, [_void_p, _void_p, _void_p, ctypes.c_int, _void_p, ctypes.c_int64,
                                 _int64_p]),
    "mpcasm_next_given": (ctypes.c_int, _PLAN_SRC + [_void_p, ctypes.c_int64, _void_p, _void_p, _void_p,
                          ctypes.c_uint32, _void_p, ctypes.c_int64, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_ltv_rollout_compile": (ctypes.c_int, _TABLES + [_void_p, _void_p, ctypes.c_int, _void_p, ctypes.c_int,
                                   _void_p, ctypes.c_int64, _int64_p]),
    "mpcasm_ltv_rollout": (ctypes.c_int, _PLAN_SRC + [_void_p, ctypes.c_int64, _void_p, _void_p, _void_p,
                           ctypes.c_int64, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_ltv_advance": (ctypes.c_int, _PLAN_SRC + [_void_p, ctypes.c_int64, _void_p, _void_p, _void_p,
                           ctypes.c_uint32, _void_p, ctypes.c_int64, ctypes.c_int, _void_p]),
    "mpcasm_ltv_rollout_info": (ctypes.c_int, _TABLES + [ctypes.c_int64, ctypes.c_int, ctypes.c_int, _int32_p,
                                _int64_p, _int32_p]),
    "mpcasm_ltv_lqr": (ctypes.c_int, [ctypes.c_int] * 4 + [_void_p, ctypes.c_int64, _void_p, ctypes.c_int64] +
                       [_void_p] * 7),
    "mpcasm_ltv_close": (ctypes.c_int, [ctypes.c_int] * 4 + [_void_p, ctypes.c_int64, _void_p, ctypes.c_int64,
                         _void_p, ctypes.c_int64, ctypes.c_int64, _void_p, _void_p]),
    "mpcasm_ltv_augment": (ctypes.c_int, [ctypes.c_int] * 4 + [_void_p, ctypes.c_int64, _void_p, ctypes.c_int64,
                           _void_p, ctypes.c_int64, ctypes.c_int64, _void_p, _void_p, _void_p, _void_p]),
    "mpcasm_ltv_true_inputs": (ctypes.c_int, _PLAN_SRC + [_void_p, ctypes.c_int64, _void_p, ctypes.c_int64, _void_p,
                               _void_p, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_gather": (ctypes.c_int, [_void_p, ctypes.c_int64, _void_p, ctypes.c_int, _void_p, ctypes.c_int, _void_p]),
    "mpcasm_box_transform": (ctypes.c_int, [_void_p, ctypes.c_int64, ctypes.c_int, _void_p, ctypes.c_int,
                             ctypes.c_int, _void_p, ctypes.c_int64, _void_p]),
    "mpcasm_box_transform_ss": (ctypes.c_int, [_void_p, ctypes.c_int64, ctypes.c_int, _void_p, ctypes.c_int,
                                ctypes.c_int, _void_p, ctypes.c_int, ctypes.c_int, _void_p, ctypes.c_int64, _void_p]),
}
KERNEL_NAMES = {0: "none", 1: "resident_assemble_kernel (persistent, ahead of time)",
                2: "resident_spec_kernel (persistent, compiled for the plan by hiprtc)",
                3: "fused_assemble_kernel", 4: "staged pipeline (compose_rowsets / hessian / constraints)",
                5: "tiled_assemble_kernel",
                6: "toeplitz_scan_kernel (tiled, scan form: P summed along diagonals)",
                7: "ltv_sweep_kernel (per-step dynamics, no horizon matrix)",
                8: "shared_p_kernel / shared_g_kernel (tiled, shared-model form: weighted sums of per-term matrices)"}
(KERNEL_NONE, KERNEL_RESIDENT, KERNEL_RESIDENT_JIT, KERNEL_FUSED, KERNEL_STAGED, KERNEL_TILED, KERNEL_TILED_SCAN,
 KERNEL_SWEEP, KERNEL_TILED_SHARED) = range(9)                               # MPCASM_KERNEL_*
PREVIEW_NONE, PREVIEW_DIRECT, PREVIEW_STAGED, PREVIEW_BLOCKED = range(4)   # out[0] of mpcasm_preview_route
PREVIEW_ROUTES = {0: "none", 1: "direct", 2: "staged", 3: "blocked"}
TILED_SCAN, TILED_TOEPLITZ, TILED_SHARED, TILED_GENERAL = range(1, 5)         # out[0] of mpcasm_tiled_route
TILED_FORMS = {1: "scan", 2: "toeplitz", 3: "shared", 4: "general"}
TILED_TABLES_NONE, TILED_TABLES_SMALL, TILED_TABLES_SYSTEM = range(3)         # out[8]
STAGED_NONE, STAGED_BLOCK, STAGED_GEMM = range(3)                             # out[0] of mpcasm_staged_route
STAGED_FORMS = {0: "none", 1: "block", 2: "gemm"}
STAGED_SYM, STAGED_WHOLE_LINES = 1, 2                                         # out[1]
WANT_COST, WANT_CONSTRAINTS = 1, 2
BOX_RECENTER, BOX_TRANSLATE, BOX_ROTATE, BOX_SCALE, BOX_MARGIN = range(5)


class MpcasmError(RuntimeError):
    """A C-ABI call returned a negative status."""

    def __init__(self, status, where, hip=0):
        self.status = status
        self.hip = hip
        msg = "%s failed: %s" % (where, STATUS.get(status, str(status)))
        if hip:
            msg += " (hipError_t %d)" % hip
        super().__init__(msg)


_lib = None


def load():
    """The loaded library (cached); raises RuntimeError when it was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libmpcasm.so is missing (%s): build it with `make -C mpc-interface_amd` "
                "or __graft_entry__.build(); the assembly kernels have no fallback" % LIB_PATH
            )
        try:
            # torch ships its own HIP runtime: load it first so that this library binds to the
            # same copy (two runtimes in one process do not share devices or streams)
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)       # AttributeError = symbol not exported
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib


def check(status, where):
    if status != OK:
        raise MpcasmError(status, where, load().mpcasm_last_hip())
