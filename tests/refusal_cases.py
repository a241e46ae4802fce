"""What the C boundary refuses, written down by hand: one row per (entry, plan, variant) with the status the entry
answers and what it leaves in the caller's results.  Every row is decided on the host, before any device work --
a negative status, or the MPCASM_OK of an empty call -- so no row reaches a launch.

CPU_ROWS: the twelve host-only queries that take a plan's tables (test_capi_refusals_cpu.py).
GPU_ROWS: the entries that take a ``mpcasm_plan*`` (test_gpu_capi_refusals.py).

profiles/capi_refusals.txt holds what the library answered before the entries' openings were put on shared helpers
(``MPCASM_LIB=<that build> python tests/refusal_cases.py cpu gpu``); the tests hold the tables to that file and the
library to the tables.

Plans: ``plain`` lipm3d N = 8; ``lti`` the same compiled with lti=["LIP"] (its horizon tables are made by a pre-pass:
t_nlti != 0); ``ltv`` lipm_ltv N = 12 compiled with ltv=["LIP"] (the sweep kernel's).  All three have two sources and
non-empty given, unknowns, limits, parameters and row sets.

A variant is a list of changes to a valid call joined by `` + ``: ``null X`` (the argument X is NULL), ``X=v``,
``truncated`` (n_itab one word short), ``stride -1`` (the first source's), ``off X n`` (the pointer X moved by n bytes),
``wrong device`` (another device current).
"""
import collections
import ctypes
import os
import sys

import numpy as np

OK, ARG, PLAN, LIMIT = 0, -1, -2, -5
UNTOUCHED, ZEROED, NO_OUT = "untouched", "zeroed", "-"
FILL = 0x5A            # every byte of a result buffer before the call

Row = collections.namedtuple("Row", "entry plan variant code out recorded")
RECORDING = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "capi_refusals.txt")


def _rows(entry, plan, *cases):
    return [Row("mpcasm_" + entry, plan, c[0], c[1], c[2] if len(c) > 2 else NO_OUT, True) for c in cases]


# ------------------------------------------------------------------------------------------------------------------
# the host-only queries.  ERR_ARG leaves the results as they were; every later refusal finds them zeroed -- except
# in the four entries that zero nothing (resident_lds_bytes, fetch_segments, ltv_rollout_compile; jit_check empties
# its log, which reads as ZEROED here)
# ------------------------------------------------------------------------------------------------------------------
def _tables(zeroes=True):
    """The three variants every query has: either table pointer missing, the tables a word short."""
    return [("null h_itab", ARG, UNTOUCHED), ("null h_dtab", ARG, UNTOUCHED),
            ("truncated", PLAN, ZEROED if zeroes else UNTOUCHED)]


_STRIDES = [("null h_src_stride", ARG, ZEROED), ("stride -1", ARG, ZEROED), ("truncated + stride -1", PLAN, ZEROED)]

CPU_ROWS = (
    _rows("resident_lds_bytes", "plain", *_tables(zeroes=False), ("null out", ARG), ("null out + truncated", ARG))
    + _rows("jit_check", "plain", *_tables())
    + _rows("fetch_segments", "plain", *_tables(zeroes=False), ("null n_words", ARG, UNTOUCHED),
            ("null out", ARG, UNTOUCHED), ("limit=-1", ARG, UNTOUCHED), ("limit=-1 + truncated", ARG, UNTOUCHED))
    + _rows("preview_route", "plain", *_tables(), *_STRIDES, ("null out", ARG), ("null out + truncated", ARG),
            ("nterms=-1", ARG, UNTOUCHED), ("ngoals=-1", ARG, UNTOUCHED), ("nterms=-1 + truncated", ARG, UNTOUCHED))
    + _rows("preview_route", "lti", ("stride -1", ARG, ZEROED))
    + _rows("preview_route", "ltv", ("valid", LIMIT, ZEROED), ("stride -1", LIMIT, ZEROED),
            ("null h_src_stride", ARG, ZEROED))
    + _rows("sweep_route", "ltv", *_tables(), ("null out", ARG), ("null out + truncated", ARG))
    + _rows("sweep_route", "plain", ("valid", ARG, ZEROED))
    + _rows("sweep_route", "lti", ("valid", ARG, ZEROED))
    + _rows("tiled_route", "plain", *_tables(), *_STRIDES, ("null out", ARG), ("null out + truncated", ARG),
            ("batch=0", ARG, UNTOUCHED), ("path=-2", ARG, UNTOUCHED), ("path=5", ARG, UNTOUCHED),
            ("want=0", ARG, UNTOUCHED), ("want=4", ARG, UNTOUCHED), ("path=5 + truncated", ARG, UNTOUCHED),
            ("valid", ARG, ZEROED))                  # (a plan of the persistent kernel: off the tiled path)
    + _rows("tiled_route", "ltv", ("valid", ARG, ZEROED), ("stride -1", ARG, ZEROED))
    + _rows("assemble_route", "plain", *_tables(), ("null out", ARG), ("null out + truncated", ARG),
            ("batch=0", ARG, UNTOUCHED), ("path=-2", ARG, UNTOUCHED), ("path=5", ARG, UNTOUCHED),
            ("inputs_aligned=-1", ARG, UNTOUCHED), ("inputs_aligned=2", ARG, UNTOUCHED),
            ("indexed=-1", ARG, UNTOUCHED), ("indexed=2", ARG, UNTOUCHED), ("path=-2 + truncated", ARG, UNTOUCHED))
    + _rows("assemble_route", "ltv", ("indexed=1", LIMIT, ZEROED))      # (the index rides on the persistent kernel)
    + _rows("staged_route", "plain", *_tables(), ("null out", ARG), ("null out + truncated", ARG),
            ("batch=0", ARG, UNTOUCHED), ("want_cost=-1", ARG, UNTOUCHED), ("want_cost=2", ARG, UNTOUCHED),
            ("want_constraints=-1", ARG, UNTOUCHED), ("want_constraints=2", ARG, UNTOUCHED),
            ("want_cost=0 + want_constraints=0", ARG, UNTOUCHED), ("batch=0 + truncated", ARG, UNTOUCHED))
    + _rows("staged_route", "ltv", ("valid", ARG, ZEROED))
    + _rows("staged_route", "lti", ("valid", ARG, ZEROED))
    + [row for entry in ("assemble_adjoint_info", "assemble_params_vjp_info") for row in (
        _rows(entry, "plain", *_tables(), *_STRIDES, ("null out", ARG), ("null out + truncated", ARG))
        + _rows(entry, "lti", ("stride -1", ARG, ZEROED))
        + _rows(entry, "ltv", ("valid", LIMIT, ZEROED), ("stride -1", LIMIT, ZEROED),
                ("null h_src_stride", ARG, ZEROED)))]
    + _rows("ltv_rollout_compile", "ltv", *_tables(zeroes=False), ("null h_sizes", ARG, UNTOUCHED),
            ("null h_recs", ARG, UNTOUCHED), ("null words", ARG), ("nrec=0", ARG, UNTOUCHED),
            ("ncvec=-1", ARG, UNTOUCHED), ("null h_cvec", ARG, UNTOUCHED), ("capacity=-1", ARG, UNTOUCHED),
            ("sizes[2]=13", ARG, UNTOUCHED), ("nrec=0 + truncated", ARG, UNTOUCHED))
    + _rows("ltv_rollout_compile", "plain", ("valid", ARG, UNTOUCHED))
    + _rows("ltv_rollout_info", "ltv", *_tables(), ("null group", ARG, UNTOUCHED), ("null lds_bytes", ARG, UNTOUCHED),
            ("null workgroups", ARG, UNTOUCHED), ("table_words=-1", ARG, UNTOUCHED), ("rows_out=-1", ARG, UNTOUCHED),
            ("rows_out=2", ARG, UNTOUCHED), ("count=-1", ARG, UNTOUCHED), ("count=0", OK, ZEROED),
            ("count=-1 + truncated", ARG, UNTOUCHED))
    + _rows("ltv_rollout_info", "plain", ("valid", ARG, ZEROED))
    + _rows("ltv_rollout_info", "lti", ("valid", ARG, ZEROED))
)


def _buffer(ctype, n):
    buf = (ctype * n)()
    ctypes.memset(buf, FILL, ctypes.sizeof(buf))
    return buf


def _state(bufs):
    """UNTOUCHED / ZEROED for the result buffers of a call (NO_OUT: none was passed)."""
    raw = b"".join(bytes(b) for b in bufs)
    if not raw:
        return NO_OUT
    if raw == bytes([FILL]) * len(raw):
        return UNTOUCHED
    return ZEROED if not any(raw) else "written"


def cpu_plans(api):
    from mpcasm import problems
    from mpcasm.plan import compile_plan

    return {"plain": compile_plan(problems.lipm3d(api, N=8)),
            "lti": compile_plan(problems.lipm3d(api, N=8), lti=("LIP",)),
            "ltv": compile_plan(problems.lipm_ltv(api, N=12), ltv=("LIP",))}


def _cpu_arguments(entry, plan):
    """The arguments of a valid call behind the tables, by name and in order, and the names of its results."""
    from mpcasm.plan import rollout_rows, rollout_sizes

    nsrc = len(plan.sources)
    strides = ("h_src_stride", (ctypes.c_int64 * nsrc)(*([0] * nsrc)))
    out = lambda n, ctype=ctypes.c_int32: ("out", _buffer(ctype, n))
    if entry == "mpcasm_resident_lds_bytes":
        return [out(2, ctypes.c_int64)], ["out"]
    if entry == "mpcasm_jit_check":        # (results: the log, whose first byte the entry clears)
        return [("log", _buffer(ctypes.c_char, 1)), ("log_capacity", 1)], ["log"]
    if entry == "mpcasm_fetch_segments":
        return [("limit", 0), out(4), ("capacity", 4), ("n_words", _buffer(ctypes.c_int64, 1))], ["out", "n_words"]
    if entry == "mpcasm_preview_route":
        return [strides, ("nterms", 0), ("ngoals", 0), out(8)], ["out"]
    if entry == "mpcasm_sweep_route":
        return [out(8)], ["out"]
    if entry == "mpcasm_tiled_route":
        return [strides, ("batch", 2), ("want", 3), ("path", 0), out(16)], ["out"]
    if entry == "mpcasm_assemble_route":
        return [("batch", 2), ("path", 0), ("inputs_aligned", 1), ("indexed", 0), out(4)], ["out"]
    if entry == "mpcasm_staged_route":
        return [("want_cost", 1), ("want_constraints", 1), ("batch", 2), out(8)], ["out"]
    if entry in ("mpcasm_assemble_adjoint_info", "mpcasm_assemble_params_vjp_info"):
        return [strides, out(4)], ["out"]
    if plan.ltv:
        recs, cvec = rollout_rows(plan)
        sizes = np.ascontiguousarray(rollout_sizes(plan), dtype=np.int32)
    else:                                  # (never read: such a plan is refused first)
        recs, cvec, sizes = np.zeros((1, 8), np.int32), np.zeros((1, 4)), np.zeros(7, np.int32)
    recs, cvec = np.ascontiguousarray(recs, dtype=np.int32), np.ascontiguousarray(cvec, dtype=np.float64)
    if entry == "mpcasm_ltv_rollout_compile":
        return [("h_sizes", (ctypes.c_int32 * 7)(*sizes)), ("h_recs", (ctypes.c_int32 * recs.size)(*recs.ravel())),
                ("nrec", recs.shape[0]), ("h_cvec", (ctypes.c_double * cvec.size)(*cvec.ravel())),
                ("ncvec", cvec.shape[0]), ("h_table", None), ("capacity", 0),
                ("words", _buffer(ctypes.c_int64, 1))], ["words"]
    assert entry == "mpcasm_ltv_rollout_info", entry
    return [("table_words", 64), ("rows_out", 1), ("count", 2), ("group", _buffer(ctypes.c_int32, 1)),
            ("lds_bytes", _buffer(ctypes.c_int64, 1)), ("workgroups", _buffer(ctypes.c_int32, 1))], \
        ["group", "lds_bytes", "workgroups"]


def _apply(args, variant):
    """``args`` (name -> value) changed as ``variant`` says; pointers moved by ``off`` become integers."""
    for change in ([] if variant in ("valid", "wrong device") else variant.split(" + ")):
        words = change.split()
        if words[0] == "null":
            assert words[1] in args, change
            args[words[1]] = None
        elif change == "truncated":
            args["n_itab"] -= 1
        elif change == "stride -1":
            args["h_src_stride"][0] = -1
        elif words[0] == "off":
            args[words[1]] = args[words[1]] + int(words[2])
        elif change.startswith("sizes["):
            args["h_sizes"][int(change[6])] = int(change.split("=")[1])
        else:
            name, value = change.split("=")
            assert name in args, change
            args[name] = int(value)
    return args


def run_cpu_row(lib, plans, row):
    """``(status, state of the results)`` of the library for a row of CPU_ROWS."""
    plan = plans[row.plan]
    itab, dtab = np.ascontiguousarray(plan.itab), np.ascontiguousarray(plan.dtab)
    assert dtab.size, "the table pointers' variants need a plan with numbers"
    tail, results = _cpu_arguments(row.entry, plan)
    args = collections.OrderedDict([("h_itab", itab.ctypes.data), ("n_itab", itab.size), ("h_dtab", dtab.ctypes.data),
                                    ("n_dtab", dtab.size)] + tail)
    bufs = [args[name] for name in results]
    _apply(args, row.variant)
    passed = [b for name, b in zip(results, bufs) if args[name] is not None]
    return getattr(lib, row.entry)(*args.values()), _state(passed)


# ------------------------------------------------------------------------------------------------------------------
# the entries that take a plan.  Arguments by name, in the order of include/mpcasm.h, between h_src_stride and stream
# ------------------------------------------------------------------------------------------------------------------
GPU_ARGS = {
    "mpcasm_plan_prepare": "batch",
    "mpcasm_assemble": "d_params d_given d_P d_q d_G d_h d_work batch",
    "mpcasm_assemble_indexed": "d_params d_given d_given_index d_P d_q d_G d_h d_work batch",
    "mpcasm_preview_matrices": "d_PM batch",
    "mpcasm_preview_direct": "d_given d_optim d_out d_work batch",
    "mpcasm_assemble_jvp": "d_params d_dgiven d_dq d_dh d_work batch",
    "mpcasm_assemble_vjp": "d_params d_gq d_gh d_ggiven d_work batch",
    "mpcasm_assemble_params_vjp": "d_params d_given d_x d_u d_y d_w d_verdict d_gparams d_work batch",
    "mpcasm_next_given": "d_next rows d_optim d_index d_status apply_mask d_map map_words d_work count",
    "mpcasm_ltv_rollout": "d_given rows d_optim d_index d_table table_words d_out count",
    "mpcasm_ltv_advance": "d_next rows d_optim d_index d_status apply_mask d_table table_words count",
    "mpcasm_ltv_true_inputs": "d_K k_stride d_given rows d_optim d_index d_uout count",
    "mpcasm_preview_goal_distance": "d_given d_optim d_params d_terms nterms ngoals d_dist d_work batch",
}
_SRC = [("null h_src", ARG), ("null h_src_stride", ARG), ("stride -1", ARG)]


def _plan(count="batch"):
    return [("null plan", ARG), (count + "=-1", ARG)]


def _nulls(*names):
    return [("null " + name, ARG) for name in names]


# a call with another device current: MPCASM_ERR_ARG from every entry that launches with the plan's tables.  Rows of
# two-device machines: the recording was made where one device shows, so none of them is in it
_WRONG_DEVICE = [Row(entry, "ltv" if "ltv" in entry else "plain", "wrong device", ARG, NO_OUT, False)
                 for entry in GPU_ARGS]
# (mpcasm_preview_matrices among them: before, it had no such check and launched there -- parent: launched; now ERR_ARG)

GPU_ROWS = (
    _rows("plan_prepare", "plain", *_plan())
    + _rows("assemble", "plain", *_plan(), ("batch=0", OK), *_SRC, *_nulls("d_params", "d_given", "d_P", "d_q", "d_G",
                                                                            "d_h", "d_work"),
            ("off d_P 8", ARG), ("off d_h 8", ARG), ("null plan + batch=0", ARG))
    + _rows("assemble", "lti", ("null d_work", ARG), ("null d_work + stride -1", ARG), ("batch=0 + null d_work", OK))
    + _rows("assemble", "ltv", ("batch=0", OK), ("stride -1", ARG))
    + _rows("assemble_indexed", "plain", *_plan(), ("batch=0", OK), ("null d_given_index", ARG),
            ("null d_given_index + batch=0", ARG), ("null h_src", ARG), ("stride -1", ARG))
    + _rows("preview_matrices", "plain", *_plan(), ("batch=0", OK), *_SRC, ("null d_PM", ARG),
            ("batch=0 + null h_src", ARG))
    + _rows("preview_matrices", "lti", ("valid", LIMIT), ("batch=0", LIMIT), ("null h_src", ARG))
    + _rows("preview_matrices", "ltv", ("valid", LIMIT), ("batch=0", LIMIT))
    + _rows("preview_direct", "plain", *_plan(), ("batch=0", OK), *_SRC, *_nulls("d_given", "d_optim", "d_out"),
            ("batch=0 + null h_src", ARG))
    + _rows("preview_direct", "lti", ("null d_work", ARG), ("null d_work + stride -1", ARG),
            ("batch=0 + null d_work", OK))
    + _rows("preview_direct", "ltv", ("valid", LIMIT), ("batch=0", OK), ("null h_src", ARG))
    + _rows("assemble_jvp", "plain", *_plan(), ("batch=0", OK), *_SRC, *_nulls("d_params", "d_dgiven"),
            ("null d_dq + null d_dh", ARG), ("batch=0 + null h_src", OK))
    + _rows("assemble_jvp", "lti", ("null d_work", ARG), ("null d_work + stride -1", ARG))
    + _rows("assemble_jvp", "ltv", ("valid", LIMIT), ("batch=0", LIMIT), ("null d_dq + null d_dh", ARG))
    + _rows("assemble_vjp", "plain", *_plan(), ("batch=0", OK), *_SRC, *_nulls("d_params", "d_ggiven"),
            ("null d_gq + null d_gh", ARG))
    + _rows("assemble_vjp", "lti", ("null d_work", ARG), ("null d_work + stride -1", ARG))
    + _rows("assemble_vjp", "ltv", ("valid", LIMIT), ("batch=0", LIMIT), ("null d_gq + null d_gh", ARG))
    + _rows("assemble_params_vjp", "plain", *_plan(), ("batch=0", OK), *_SRC,
            *_nulls("d_params", "d_given", "d_x", "d_u", "d_y", "d_w", "d_gparams"))
    + _rows("assemble_params_vjp", "lti", ("null d_work", ARG), ("null d_work + stride -1", ARG))
    + _rows("assemble_params_vjp", "ltv", ("valid", LIMIT), ("batch=0", LIMIT), ("null d_params", LIMIT))
    + _rows("next_given", "plain", *_plan("count"), ("rows=-1", ARG), ("map_words=-1", ARG), ("count=0", OK), *_SRC,
            *_nulls("d_next", "d_optim", "d_map"), ("null d_index + rows=1", ARG))
    + _rows("next_given", "lti", ("null d_work", ARG), ("null d_work + stride -1", ARG))
    + _rows("next_given", "ltv", ("valid", LIMIT), ("count=0", LIMIT), ("null d_next", LIMIT))
    + [row for entry, out in (("ltv_rollout", ["d_out"]), ("ltv_advance", [])) for row in (
        _rows(entry, "ltv", *_plan("count"), ("rows=-1", ARG), ("table_words=-1", ARG), ("count=0", OK), *_SRC,
              *_nulls(*(["d_given" if out else "d_next", "d_optim", "d_table"] + out)),
              ("null d_index + rows=1", ARG), ("count=0 + null h_src", OK))
        + _rows(entry, "plain", ("valid", ARG), ("count=0", ARG))
        + _rows(entry, "lti", ("valid", ARG)))]
    + _rows("ltv_rollout", "ltv", ("off d_out 4", ARG))
    + _rows("ltv_true_inputs", "ltv", *_plan("count"), ("rows=-1", ARG), ("k_stride=-1", ARG), ("count=0", OK), *_SRC,
            *_nulls("d_K", "d_given", "d_optim", "d_uout"), ("off d_K 4", ARG), ("off d_uout 4", ARG),
            ("off d_index 2", ARG), ("null d_index + rows=1", ARG))
    + _rows("ltv_true_inputs", "plain", ("valid", ARG), ("count=0", ARG))
    + _rows("preview_goal_distance", "plain", *_plan(), ("nterms=-1", ARG), ("ngoals=-1", ARG), ("batch=0", OK),
            ("ngoals=0", OK), *_SRC, *_nulls("d_dist", "d_given", "d_optim", "d_terms", "d_params"),
            ("batch=0 + null d_dist", OK))
    + _rows("preview_goal_distance", "lti", ("null d_work", ARG), ("null d_work + stride -1", ARG))
    + _rows("preview_goal_distance", "ltv", ("valid", LIMIT), ("batch=0", OK), ("null d_dist", ARG))
    + _WRONG_DEVICE
)


class GpuBench:
    """One assembler at batch 2 for each plan, and for each the operands of a valid call of every entry: inputs of
    zeros, results of NaN (``outputs``).  No row writes any of them."""

    def __init__(self, api):
        import torch
        from mpcasm import engine, problems

        self.torch, self.engine = torch, engine
        self.asm = {"plain": engine.Assembler(problems.lipm3d(api, N=8), batch=2),
                    "lti": engine.Assembler(problems.lipm3d(api, N=8), batch=2, lti=["LIP"]),
                    "ltv": engine.Assembler(problems.lipm_ltv(api, N=12), batch=2, ltv=["LIP"])}
        self.buf, self.outputs = {}, {}
        for key, asm in self.asm.items():
            f = dict(dtype=torch.float64, device=asm.device)
            i = dict(dtype=torch.int32, device=asm.device)
            ng, no, nc, npar, rows = asm.ng, asm.no, asm.nc, asm.params.shape[1], asm.plan.pmrows
            nan = lambda *shape: torch.full(shape, float("nan"), **f)
            out = dict(d_P=nan(2, no, no), d_q=nan(2, no), d_G=nan(2, nc, no), d_h=nan(2, nc), d_PM=nan(2, rows, ng + no),
                       d_out=nan(2, rows), d_dq=nan(2, no), d_dh=nan(2, nc), d_ggiven=nan(2, ng), d_gparams=nan(2, npar),
                       d_next=nan(2, ng), d_uout=nan(2, 4, 12, 4), d_dist=nan(2, 1))
            zeros = lambda *shape: torch.zeros(shape, **f)
            self.outputs[key] = out
            self.buf[key] = dict(
                out, d_params=zeros(2, npar), d_given=zeros(2, ng), d_optim=zeros(2, no), d_dgiven=zeros(2, ng),
                d_gq=zeros(2, no), d_gh=zeros(2, nc), d_x=zeros(2, no), d_u=zeros(2, no), d_y=zeros(2, nc),
                d_w=zeros(2, nc), d_K=zeros(2, 12, 4, 4), d_work=asm._workspace(),
                d_given_index=torch.arange(2, **i), d_index=torch.arange(2, **i), d_status=torch.ones(2, **i),
                d_verdict=torch.ones(2, **i), d_map=torch.zeros(64, **i), d_table=torch.zeros(64, **i),
                d_terms=torch.zeros((1, 4), **i))
        self.scalars = dict(batch=2, count=2, rows=2, apply_mask=2, map_words=64, table_words=64, k_stride=0, nterms=1,
                            ngoals=1)

    def run(self, lib, row):
        """The library's status for a row of GPU_ROWS."""
        torch, asm = self.torch, self.asm[row.plan]
        n = len(asm._src)
        args = collections.OrderedDict(plan=asm._handle.value)
        if row.entry != "mpcasm_plan_prepare":
            args["h_src"] = (ctypes.c_void_p * n)(*(t.data_ptr() for t in asm._src))
            args["h_src_stride"] = (ctypes.c_int64 * n)(*asm._src_stride)
        for name in GPU_ARGS[row.entry].split():
            args[name] = self.scalars[name] if name in self.scalars else self.buf[row.plan][name].data_ptr()
        _apply(args, row.variant)
        device = asm.device
        if row.variant == "wrong device":
            device = torch.device("cuda", (asm.device.index + 1) % torch.cuda.device_count())
        with torch.cuda.device(device):
            tail = [] if row.entry == "mpcasm_plan_prepare" else [self.engine._stream_handle(torch, None)]
            return getattr(lib, row.entry)(*args.values(), *tail)

    def results_untouched(self):
        """Whether every result buffer of every plan still holds nothing but NaN, the device idle."""
        self.torch.cuda.synchronize()
        return all(bool(self.torch.isnan(t).all().item()) for out in self.outputs.values() for t in out.values())


# ------------------------------------------------------------------------------------------------------------------
def line(half, row, code, out):
    return "%s | %s | %s | %s | %d | %s" % (half, row.entry, row.plan, row.variant, code, out)


def recorded(half):
    """The rows of ``half`` in profiles/capi_refusals.txt, as ``line`` writes them."""
    with open(RECORDING) as f:
        return [text.rstrip("\n") for text in f if text.startswith(half + " |")]


def main(halves):
    """Print what the library in use (``MPCASM_LIB``) answers for the rows, one line each."""
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(os.path.dirname(here), "mpc-interface_amd"), os.path.dirname(here)]
    from mpcasm import capi, problems
    from oracle import qp_oracle
    import mpc_interface.tools as tools

    lib = capi.load()
    if "cpu" in halves:
        tools.extend_matrices, kept = qp_oracle.extend_matrices, tools.extend_matrices
        plans = cpu_plans(problems.load_api("mpc_interface"))
        tools.extend_matrices = kept
        for row in CPU_ROWS:
            print(line("cpu", row, *run_cpu_row(lib, plans, row)))
    if "gpu" in halves:
        bench = GpuBench(problems.load_api("mpc_interface"))
        devices = lib.mpcasm_device_count()
        print("# gpu half recorded with %d device%s visible" % (devices, "" if devices == 1 else "s"))
        for row in GPU_ROWS:
            if row.variant == "wrong device" and (devices < 2 or row.entry == "mpcasm_preview_matrices"):
                continue                   # (no other device; and the one entry that used to launch there)
            print(line("gpu", row, bench.run(lib, row), NO_OUT))
        print("# results still NaN after every row: %s" % bench.results_untouched())


if __name__ == "__main__":
    main(sys.argv[1:])
