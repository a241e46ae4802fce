// plan_dev.h -- device-side view of a plan and the source table of a launch: plain structs, no
// HIP runtime types, so that the persistent kernel's source also compiles under hiprtc
// (MPCASM_SPEC, resident.hip).
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#include "plan_tables.h"

namespace mpcasm {

// every int field of PlanDev, once, in the struct's order: X(field, WORD) is copied from header word H_WORD of
// itab, D(field) is derived from the tables by plan_view's own code (plan_check.cpp; rs_p_direct by host_plan).
// The struct, plan_view's copies and the constants of a specialised kernel (jit.hip) are generated from this
// list.  Eight header words have no field: MAGIC, VERSION, NITAB, NDTAB, NDIAGCOEF, PM_NOPS, PM_NPOOL, T_NDELTA.
#define MPCASM_PLAN_INT_FIELDS(X, D)                                                                                    \
  X(ng, NG) X(no, NO) X(nc, NC) X(nparams, NPARAMS) X(nsrc, NSRC) X(nbase, NBASE) X(nseg, NSEG) X(rtot, RTOT)           \
  X(nent, NENT) X(ngterm, NGTERM) X(nlimit, NLIMIT) X(nlax, NLAX) X(pmrows, PMROWS) X(pm_nent, PM_NENT) X(ldv, LDV)     \
  X(off_seg, OFF_SEG) X(off_colseg, OFF_COLSEG) X(off_rowptr, OFF_ROWPTR) X(off_entbase, OFF_ENTBASE)                   \
  X(off_entk, OFF_ENTK) X(off_gterm, OFF_GTERM) X(off_limit, OFF_LIMIT) X(off_lax, OFF_LAX)                             \
  X(off_rowlimit, OFF_ROWLIMIT) X(off_pm_rowptr, OFF_PM_ROWPTR) X(off_pm_entbase, OFF_PM_ENTBASE)                       \
  X(off_pm_entk, OFF_PM_ENTK) X(doff_entcoef, DOFF_ENTCOEF) X(doff_pm_entcoef, DOFF_PM_ENTCOEF) X(fused_ok, FUSED_OK)   \
  X(arena_total, ARENA_TOTAL) X(off_arena, OFF_ARENA) X(nfd, NFD) X(off_fd_idx, OFF_FD_IDX) X(off_fd_ptr, OFF_FD_PTR)   \
  X(nops, NOPS) X(off_op, OFF_OP) X(ncoef, NCOEF) X(doff_coefpool, DOFF_COEFPOOL) D(max_axes) D(rs_sym_any)             \
  X(rs_ok, RS_OK) X(rs_jc, RS_JC) X(rs_sym, RS_SYM) X(rs_ntrip, RS_NTRIP) X(off_rs_src, OFF_RS_SRC)                     \
  X(off_rs_gidx, OFF_RS_GIDX) X(off_rs_dst, OFF_RS_DST) X(doff_rs_coef, DOFF_RS_COEF) X(off_rs_trip, OFF_RS_TRIP)       \
  X(off_rs_wtrip, OFF_RS_WTRIP) X(rs_nsplit, RS_NSPLIT) X(off_rs_split, OFF_RS_SPLIT) X(off_rs_rr, OFF_RS_RR)           \
  X(rs_unit, RS_UNIT) X(rs_nchunk, RS_NCHUNK) X(off_rs_inmeta, OFF_RS_INMETA) X(rs_img, RS_IMG)                         \
  X(rs_img_given, RS_IMG_GIVEN) X(rs_img_params, RS_IMG_PARAMS) X(doff_rs_const, DOFF_RS_CONST) X(rs_nlti, RS_NLTI)     \
  X(off_rs_lti, OFF_RS_LTI) X(rs_img_dma, RS_IMG_DMA) X(rs_ab, RS_AB) X(off_rs_abmeta, OFF_RS_ABMETA)                   \
  X(rr_packed, RR_PACKED) X(off_rs_dpar, OFF_RS_DPAR) X(doff_rs_dcoef, DOFF_RS_DCOEF) X(rs_ngdesc, RS_NGDESC)           \
  X(off_rs_gdesc, OFF_RS_GDESC) X(pm_nfd, PM_NFD) X(off_pm_map, OFF_PM_MAP) X(off_pm_fdptr, OFF_PM_FDPTR)               \
  X(off_pm_op, OFF_PM_OP) X(doff_pm_pool, DOFF_PM_POOL) X(doff_diagcoef, DOFF_DIAGCOEF) D(ndiag) X(rs_nzblk, RS_NZBLK)  \
  X(off_rs_zblk, OFF_RS_ZBLK) D(rs_p_direct) X(rs_gsingle, RS_GSINGLE) X(csc_pnnz, CSC_PNNZ) X(off_csc_p, OFF_CSC_P)    \
  X(csc_gnnz, CSC_GNNZ) X(off_csc_g, OFF_CSC_G) X(csc_gsingle, CSC_GSINGLE) X(t_ci_ok, T_CI_OK) X(t_nop, T_NOP)         \
  X(off_t_cig, OFF_T_CIG) X(off_t_cio, OFF_T_CIO) X(t_doff_delta, T_DOFF_DELTA) X(t_ok, T_OK) X(t_nstage, T_NSTAGE)     \
  X(off_t_stage, OFF_T_STAGE) X(t_nlti, T_NLTI) X(off_t_lti, OFF_T_LTI) X(off_t_lti_ids, OFF_T_LTI_IDS)                 \
  X(t_work, T_WORK) X(off_t_grow, OFF_T_GROW) X(off_t_srow, OFF_T_SROW) X(t_doff_scoef, T_DOFF_SCOEF)                   \
  X(off_t_pig, OFF_T_PIG) X(t_ngrest, T_NGREST) X(off_t_grest, OFF_T_GREST) X(off_t_brow0, OFF_T_BROW0) D(t_nbrow)      \
  X(t_toeplitz, T_TOEPLITZ) D(rs_diag_table) X(off_t_bcolptr, OFF_T_BCOLPTR) X(off_t_bcols, OFF_T_BCOLS)                \
  X(rs_ngfix, RS_NGFIX) X(off_rs_gfix, OFF_RS_GFIX) X(rs_compact, RS_COMPACT) X(rs_ldv, RS_LDV) X(rs_vd, RS_VD)         \
  X(rs_vrow0, RS_VROW0) X(off_rs_rrwin, OFF_RS_RRWIN) X(t_np1, T_NP1) X(off_t_p1ptr, OFF_T_P1PTR)                       \
  X(off_t_p1ent, OFF_T_P1ENT) X(off_t_p2y, OFF_T_P2Y) X(t_scan, T_SCAN) X(t_scan_nblk, T_SCAN_NBLK)                     \
  X(off_t_scan_blk, OFF_T_SCAN_BLK) X(off_t_scan_gt, OFF_T_SCAN_GT) X(t_doff_scan_gc, T_DOFF_SCAN_GC)                   \
  X(off_t_scan_grow, OFF_T_SCAN_GROW) X(t_doff_scan_gcoef, T_DOFF_SCAN_GCOEF) X(t_scan_ngrest, T_SCAN_NGREST)           \
  X(off_t_scan_grest, OFF_T_SCAN_GREST) X(off_t_scan_colblk, OFF_T_SCAN_COLBLK) X(t_scan_nother, T_SCAN_NOTHER)         \
  X(sw_ok, SW_OK) X(sw_n, SW_N) X(sw_m, SW_M) X(sw_horizon, SW_HORIZON) X(sw_src_a, SW_SRC_A) X(sw_src_b, SW_SRC_B)     \
  X(sw_naxes, SW_NAXES) X(off_sw_axis, OFF_SW_AXIS) X(sw_nterm, SW_NTERM) X(off_sw_term, OFF_SW_TERM)                   \
  X(sw_nlim, SW_NLIM) X(off_sw_lim, OFF_SW_LIM) X(off_sw_col, OFF_SW_COL) X(sw_doff_cvec, SW_DOFF_CVEC)                 \
  X(sw_ncvec, SW_NCVEC) X(off_sw_cptr, OFF_SW_CPTR) X(off_sw_cent, OFF_SW_CENT) X(sw_ncent, SW_NCENT)                   \
  X(off_sw_gptr, OFF_SW_GPTR) X(off_sw_gent, OFF_SW_GENT) X(sw_ngent, SW_NGENT) X(off_rs_prog, OFF_RS_PROG)             \
  X(t_scan_fused, T_SCAN_FUSED)

// device-side view of a plan (pointers into the device copies of the tables).
//   rs_p_direct: the persistent kernel sends the blocks of P straight to HBM (set by
//   resident_choose_p_direct: P does not fit in LDS beside the workspace, or MPCASM_OPT_P_DIRECT);
//   rs_sym_any: every Hessian term has A == B;  rs_src16: sources that the 16-byte image loads
//   read (bit per source);  ndiag: number of diagonal gterms, doff_diagcoef: their coefficients
struct PlanDev {
  const int32_t* itab;
  const double* dtab;
#define MPCASM_X(f, ...) int f;
  MPCASM_PLAN_INT_FIELDS(MPCASM_X, MPCASM_X)
#undef MPCASM_X
  unsigned rs_src16;
};

// LDS the persistent kernel may ask for (a whole CU's 160 KiB less what the runtime keeps)
constexpr int RESIDENT_LDS_LIMIT = 156 * 1024;

// sources of one launch (device pointers + per-instance strides, by value)
struct SrcTable {
  const double* ptr[MAX_SOURCES];
  long long stride[MAX_SOURCES];
};

}  // namespace mpcasm
