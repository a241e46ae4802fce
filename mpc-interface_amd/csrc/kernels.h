// kernels.h -- internal launch interface between capi.hip, dispatch.hip and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <vector>

#include "../../include/mpcasm.h"
#include "plan_check.h"
#include "plan_dev.h"
#include "plan_tables.h"

namespace mpcasm {

// capi.hip: raise a kernel's dynamic-LDS limit to the CU's whole LDS -- ONCE per (function, device),
// process-wide and under a mutex.  The attribute belongs to the function, not to the calling thread
// or the plan: a limit that followed each launch's size could be lowered by one host thread under
// another thread's larger plan (and a replayed graph node of the larger plan would meet it).
constexpr int CU_LDS_BYTES = 160 * 1024;
hipError_t allow_whole_lds(const void* fn);

// fill.hip
int launch_fill_su(const double* A, const double* B, double* S, double* U, int batch, int N, int n,
                   int m, int ltv, hipStream_t stream, hipError_t* err);
// host only: what launch_fill_su launches (mpcasm_fill_route).  `kernel`: MPCASM_FILL_*; `arg`: the kernel's
// integer template argument (NS of the quad, ltv-row and ltv-block kernels, TPI of the lti and ltv kernels, else
// 0); `generic`, `pad`: fill_lti_kernel's GENERIC and PAD; `spw`: systems per wavefront (quad and tiny kernels);
// `lshift`, `whole_lines`: the quad kernel's; `grid`: workgroups; `lds`: dynamic LDS of a workgroup;
// `row`: the row of that kernel's table of instantiations.  What the decision depends on beside the sizes: whether
// S and U are both 16-byte aligned, and MPCASM_FILL_MIN_WAVES.  MPCASM_ERR_LIMIT where nothing is launched: one
// system's LDS is more than a workgroup is granted (RESIDENT_LDS_LIMIT), or no instantiation takes the sizes.
struct FillChoice {
  int kernel, arg, generic, pad, spw, lshift, whole_lines, grid, row;
  size_t lds;
};
int fill_choose(int batch, int N, int n, int m, int ltv, bool aligned16, FillChoice* out);

// ---- mpcasm_assemble: options, route and call record --------------------------------------------------------
// The process-wide options of mpcasm_set_option (defined in capi.hip, beside the table of their ranges): read and
// written relaxed, so a launch on one thread may race a mpcasm_set_option on another and sees the old value or
// the new.  No launch code reads this record: it reads the LaunchOptions of its call.
struct Options {
  std::atomic<int> path{0};              // MPCASM_OPT_PATH: 0 best, 1 no persistent kernel, 2 staged only, 3, 4: mpcasm.h
  std::atomic<int> phase_mask{0xBF};     // MPCASM_OPT_PHASE_MASK: diagnostic (timing-only ablation)
  std::atomic<int> per_cu{0};            // MPCASM_OPT_RESIDENT_PER_CU: tuning aid, 0 = automatic
  std::atomic<int> jit{0};               // MPCASM_OPT_JIT: 0 automatic (batches >= JIT_MIN_BATCH), 1 always, 2 never
  std::atomic<int> p_direct{0};          // MPCASM_OPT_P_DIRECT (read when a plan is created)
  std::atomic<int> grid{0};              // MPCASM_OPT_RESIDENT_GRID: 0 = every resident workgroup slot
  std::atomic<int> fetch_runs{FS_MAX};   // MPCASM_OPT_JIT_FETCH_RUNS (test aid): most runs of a chunk fetched by arithmetic
};
extern Options g_options;
// the options in force for ONE launch or its prediction: the plan's own where mpcasm_plan_set_option gave it some,
// else the process-wide ones (capi.hip launch_options, the only place that says so)
struct LaunchOptions {
  int path, jit, per_cu, grid, phase_mask, fetch_runs;
};
// dispatch.hip: which kernel family a launch of `batch` instances runs on -- the ONE statement of the order (sweep,
// persistent, tiled, fused, staged).  Host only, no device call.  `kernel`: MPCASM_KERNEL_* (the persistent kernel
// as MPCASM_KERNEL_RESIDENT, ahead of time or compiled for the plan); `p_direct`: the persistent kernel's hand-over
// of P for this batch (resident_p_direct_for; 0 on the sweep kernel); `lds`: dynamic LDS bytes of the persistent
// or the fused kernel, else 0.  MPCASM_ERR_LIMIT: rows of `given` by index off the persistent kernel, or a plan
// with generated horizon matrices or CSC results that no kernel takes.
struct AssembleRoute {
  int kernel, p_direct;
  size_t lds;
};
int assemble_route(const PlanDev& plan, int batch, const LaunchOptions& opt, bool inputs_aligned, bool indexed,
                   AssembleRoute* out);
// what travels unchanged from mpcasm_assemble to the kernel launches.  h_itab / device: the plan's tables on the
// host and its device, for the per-plan compiled kernel (jit.hip); *err: the runtime's word where MPCASM_ERR_HIP
// comes back; *kernel: the MPCASM_KERNEL_* actually launched (what mpcasm_plan_last_kernel reports)
struct AssembleCall {
  const SrcTable& src;
  const double *params, *given;
  double *P, *q, *G, *h;
  void* work;
  int batch;
  hipStream_t stream;
  int num_cus, device;
  const int32_t* h_itab;
  bool indexed;
  LaunchOptions opt;
  hipError_t* err;
  int* kernel;
};
int launch_assemble(const PlanDev& plan, const AssembleCall& call);

// assemble.hip
size_t assemble_workspace_bytes(const PlanDev& p, int batch);
int launch_assemble_staged(const PlanDev& p, const AssembleCall& call);
// host only: what launch_assemble_staged launches for a plan (mpcasm_staged_route).  `hessian`: MPCASM_STAGED_*
// (NONE: the cost is not wanted, or no unknown); the GEMM (128 unknowns or more): `sym` (only the block pairs
// bi <= bj, mirrored on store), `nb` blocks of 128 columns, `npairs` workgroups per instance, `ncb` 64-column
// blocks of the gradient kernel; the block kernel: `nbr` x `nbc` blocks of 32 x 32 of [P | q], `k3_nrb`
// workgroups per instance; `k2_nrb`, `k4_nrb`: row blocks per instance of K2 and K4; grid_*: workgroups of the
// four launches (0: not launched; K4's are dealt to the XCDs in groups of eight instances); `whole_lines`: K4's
// rows are whole cache lines (16 | no); `max_axes`: the most axes of a limit.  Which branch of K4 a row takes
// follows from that row's own axes and the parity of no.  MPCASM_ERR_LIMIT where nothing is launched.
struct StagedChoice {
  int hessian, sym, nb, npairs, ncb, nbr, nbc, whole_lines, max_axes;
  int k2_nrb, k3_nrb, k4_nrb;
  unsigned grid_k2, grid_k3, grid_gradient, grid_k4;
};
int staged_choose(const PlanDev& p, bool want_cost, bool want_constraints, int batch, StagedChoice* out);
// tiled.hip
bool tiled_eligible(const PlanDev& p);
size_t tiled_workspace_bytes(const PlanDev& p, int batch);
int launch_assemble_tiled(const PlanDev& p, const AssembleCall& call);
int launch_lti_tables(const PlanDev& p, const SrcTable& src, double* work, int batch,
                      const int32_t* h_itab, SrcTable* eff, hipStream_t stream, hipError_t* err);
// (toeplitz_zero_pad, the zeros toeplitz_assemble_kernel keeps in LDS behind the group's table: plan_check.h, beside
// the checker that holds the stages to it)
// host only: what launch_assemble_tiled launches for a plan (mpcasm_tiled_route).  `form`: MPCASM_TILED_*;
// scan form: fused (the kernel makes its table and d itself) or behind the pre-passes, the instantiation
// toeplitz_scan_kernel<kp, cb>, whether the records of G's rows ride in LDS, whether results leave as whole
// lines; `lds`: dynamic LDS of the scan or the Toeplitz kernel; `tables`: the pre-pass that makes the horizon
// tables (MPCASM_TILED_TABLES_*); `tg`: shared_p_kernel<tg> (0: P not wanted, or no weight); `sym`: only the
// lower block pairs of P (Toeplitz, general and the K_g of the shared form).  What the decision depends on
// beside the plan: the sources' strides, the batch, which halves are wanted, MPCASM_OPT_PATH, and whether the
// launch has `given` and a workspace.  `row`: the row of the scan form's or of shared_p_kernel's table of
// instantiations that kp, cb or tg were read from (-1: none of either is launched).
struct TiledChoice {
  int form, fused, kp, cb, rows_in_lds, whole_lines, tables, tg, sym, row;
  int dlen;     // (scan form: doubles of d in LDS)
  size_t lds;
};
int tiled_choose(const PlanDev& p, const SrcTable& src, const int32_t* h_itab, int path, int batch,
                 bool want_cost, bool want_constraints, bool have_given, bool have_work, TiledChoice* out);
// (host only: the streams a launch reads once launch_lti_tables has run -- the strides alone with work == nullptr)
int lti_effective_sources(const PlanDev& p, const SrcTable& src, double* work, const int32_t* h_itab,
                          SrcTable* eff);
// sweep.hip: a dynamics compiled as ltv -- per-step, per-instance (A_k, B_k), no horizon matrix
bool sweep_eligible(const PlanDev& p);
// host only: what launch_assemble_sweep launches for a plan (mpcasm_sweep_route) -- the instantiation
// ltv_sweep_kernel<cpt, NS, MS, AS, pair> (specialised: NS, MS, AS = 3, 1, 2, else 0, 0, 0), how the lines of G
// are walked (per_line, reg_lines), the dynamic LDS of a workgroup and the row of the table of instantiations;
// MPCASM_ERR_LIMIT where nothing is launched
struct SweepChoice {
  int cpt, specialised, pair, per_line, reg_lines, row;
  size_t lds;
};
int sweep_choose(const PlanDev& p, const int32_t* h_itab, SweepChoice* out);
int sweep_lines_ahead(int cpt);   // LR: the lines of a step whose words and weights are fetched at once
int launch_assemble_sweep(const PlanDev& p, const AssembleCall& call);
// preview.hip
int launch_preview_direct(const PlanDev& p, const SrcTable& eff, const double* given,
                          const double* optim, double* out, int batch, int num_cus,
                          hipStream_t stream, hipError_t* err, const int32_t* h_itab = nullptr);
int launch_preview_goals(const PlanDev& p, const SrcTable& eff, const double* given, const double* optim,
                         const double* params, long long nparams, const int32_t* terms, int nterms,
                         int ngoals, double* out, int batch, int num_cus, hipStream_t stream,
                         hipError_t* err, const int32_t* h_itab);
// host only: the kernel the two launches above pick (mpcasm_preview_route; ngoals == 0: the rows)
int preview_route(const PlanDev& p, const SrcTable& eff, const int32_t* h_itab, int nterms, int ngoals,
                  int32_t out[8]);
// the next tick's `given` (mpcasm_next_given): the map's rows / constants into the instances' rows
int launch_next_given(const PlanDev& p, const SrcTable& eff, const int32_t* map, long long map_words,
                      double* given, long long rows, const double* optim, const int32_t* index,
                      const int32_t* status, unsigned apply_mask, int count, int num_cus, hipStream_t stream,
                      hipError_t* err);
int compile_given_map(const PlanDev& p, const int32_t* h_itab, const int32_t* rows, const double* values,
                      std::vector<int32_t>* out);
// adjoint.hip: the derivative of the assembly with respect to `given`, applied matrix-free (mpcasm_assemble_jvp,
// mpcasm_assemble_vjp).  The transposed index is derived from the plan's tables on the host; offsets are words
// into `idx`, the o_* doubles into the kernel's dynamic LDS.  An entry of a rho row's contributions is two words:
// source | flags, parameter slot.
constexpr int32_t ADJ_SRC_MASK = (1 << 28) - 1, ADJ_HALF = 1 << 29, ADJ_LIMIT = 1 << 30;
struct AdjointView {
  const int32_t* idx;
  int rowbase;            // [base rows] the base variable of every base row
  int bsplit;             // [NBASE] where the unknowns begin among the base variable's columns (T_BCOLS)
  int cb_ptr, cb_ent;     // [NG + NO + 1], [..] per column the base variables that cover it
  int et_ptr, et_ent;     // [base rows + 1], [NENT][2] the CSC of E: workspace row, entry
  int rj_ptr, rj_ent;     // [RTOT + 1], [..][2] what adds into a rho row, JVP
  int rv_ptr, rv_ent;     // ... VJP
  int lanes_j, lanes_v;   // threads per column of the last step
  int o_x, o_gh, o_y, o_r, o_rho, o_bases;
};
struct AdjointIndex {
  std::vector<int32_t> words;
  AdjointView view;
  size_t lds;             // dynamic LDS of a workgroup
  int per_cu;             // resident workgroups per CU: grid = min(batch, CUs * per_cu)
};
int adjoint_build_index(const PlanDev& p, const int32_t* h_itab, AdjointIndex* out);
int launch_assemble_adjoint(const PlanDev& p, const SrcTable& eff, const AdjointIndex& index, bool vjp,
                            const double* params, const double* in_x, const double* in_h, double* out_x,
                            double* out_h, int batch, int num_cus, hipStream_t stream, hipError_t* err);
// ... and with respect to the parameters (mpcasm_assemble_params_vjp).  The parameter index: per slot
// [SL_PTR[s], SL_PTR[s + 1]) its records of PA_REC_WORDS words -- kind | flags, rows n, f0 .. f4, 0:
//   PA_GT_WEIGHT    rows a, rows b (PA_P), rows d, the aim's slot      the weight of a non-diagonal gterm
//   PA_GT_AIM       rows a, the weight's slot                          its aim
//   PA_DIAG_WEIGHT  first column, coefficients (dtab), the aim's slot  the weight of a GT_FLAG_DIAG gterm
//   PA_DIAG_AIM     first column, coefficients (dtab), the weight's slot
//   PA_LIMIT_ARROW  first line R, workspace row and its step per line, the centre's slot and its step per line
//   PA_LIMIT_CENTER first line R, the arrow's slot and its step per line
//   PA_LIMIT_EXTREME first line R
// (PA_HALF: s = 1/2; PA_P: the gterm has a Hessian part).  o_*: doubles into the kernel's dynamic LDS.
enum { PA_GT_WEIGHT = 0, PA_GT_AIM, PA_DIAG_WEIGHT, PA_DIAG_AIM, PA_LIMIT_ARROW, PA_LIMIT_CENTER, PA_LIMIT_EXTREME };
constexpr int32_t PA_KIND_MASK = 15, PA_HALF = 1 << 4, PA_P = 1 << 5;
constexpr int PA_REC_WORDS = 8;
struct ParamsView {
  const int32_t* idx;
  int sl_ptr, sl_rec;     // [NPARAMS + 1], [..][PA_REC_WORDS] (16-byte aligned)
  int lanes;              // threads per parameter slot
  int o_x, o_u, o_g, o_y, o_w, o_yb, o_rx, o_ru, o_rg, o_bases;
};
struct ParamsIndex {
  std::vector<int32_t> words;
  ParamsView view;
  size_t lds;
  int per_cu;
};
int params_adjoint_build_index(const PlanDev& p, const int32_t* h_itab, ParamsIndex* out);
int launch_assemble_params_adjoint(const PlanDev& p, const SrcTable& eff, const AdjointIndex& adj,
                                   const ParamsIndex& index, const double* params, const double* given,
                                   const double* x, const double* u, const double* y, const double* w,
                                   const int32_t* verdict, double* gparams, int batch, int num_cus,
                                   hipStream_t stream, hipError_t* err);
// rollout.hip: the preview rows and the next given of a plan compiled as ltv, by the forward recursion
int compile_rollout_table(const PlanDev& p, const int32_t* recs, int nrec, const double* cvec, int ncvec,
                          std::vector<int32_t>* out);
struct RolloutGeometry {
  int group;       // instances of one workgroup
  size_t lds;      // dynamic LDS bytes of a workgroup
  unsigned grid;   // workgroups
};
int ltv_rollout_geometry(const PlanDev& p, long long table_words, bool rows_out, int count, RolloutGeometry* geo);
int launch_ltv_rollout(const PlanDev& p, const SrcTable& src, const int32_t* table, long long table_words,
                       double* given, long long rows, const double* optim, const int32_t* index,
                       const int32_t* status, unsigned apply_mask, double* out, int write_given, int count,
                       hipStream_t stream, hipError_t* err);
// feedback.hip: pre-stabilised prediction for a dynamics compiled as ltv -- the gains of a backward Riccati sweep,
// A_cl = A + B K, and the true inputs u_k = K_k x_k + v_k of a plan whose unknowns are v
int launch_ltv_lqr(int n, int m, int T, int batch, const double* A, long long strideA, const double* B,
                   long long strideB, const double* Q, const double* R, const double* PT, double* K, double* Acl,
                   int32_t* info, hipStream_t stream, hipError_t* err);
int launch_ltv_close(int n, int m, int T, int batch, const double* A, long long strideA, const double* B,
                     long long strideB, const double* K, long long strideK, long long stepK, double* Acl,
                     hipStream_t stream, hipError_t* err);
// ... and the closed loop augmented by one delay, z = [x ; u_prev], whose last m states are the true inputs
int launch_ltv_augment(int n, int m, int T, int batch, const double* A, long long strideA, const double* B,
                       long long strideB, const double* K, long long strideK, long long stepK, double* At, double* Bt,
                       double* Kt, hipStream_t stream, hipError_t* err);
int launch_ltv_true_inputs(const PlanDev& p, const SrcTable& src, const double* K, long long strideK,
                           const double* given, long long rows, const double* optim, const int32_t* index,
                           double* out, int count, hipStream_t stream, hipError_t* err);
int launch_goal_distance(const double* preview, long long preview_stride, const double* params,
                         long long nparams, const int32_t* terms, int nterms, int ngoals,
                         double* out, int batch, hipStream_t stream, hipError_t* err);
// fused.hip
size_t fused_lds_bytes(const PlanDev& p, int nw);
int launch_assemble_fused(const PlanDev& p, const AssembleCall& call, size_t lds_bytes);
// resident.hip
size_t resident_lds_bytes(const PlanDev& p);
int resident_choose_p_direct(const PlanDev& p, int option);
int resident_p_direct_for(const PlanDev& p, int batch);
// whether this launch's buffers meet the alignment the plan's input loads assume
bool resident_inputs_aligned(const PlanDev& p, const SrcTable& src, const double* params,
                             const double* given);
int launch_assemble_resident(const PlanDev& p, const AssembleCall& call, size_t lds_bytes);
int launch_preview_matrices(const PlanDev& p, const SrcTable& src, double* PM, int batch,
                            hipStream_t stream, hipError_t* err);
int launch_box_transform(double* params, long long nparams, int batch, const int32_t* facets,
                         int nfacets, int op, const double* arg, long long arg_stride,
                         hipStream_t stream, hipError_t* err);
int launch_box_transform_ss(double* params, long long nparams, int batch, const int32_t* facets,
                            int nfacets, int op, const double* L, int lrows, int ss_dim,
                            const double* arg, long long arg_stride, hipStream_t stream,
                            hipError_t* err);
int launch_gather(const double* src, long long src_stride, const int32_t* index, int nnz,
                  double* dst, int batch, hipStream_t stream, hipError_t* err);
// ---- the QP solvers (admm.hip, admm_wide.hip, polish.hip, polish_wide.hip) ----------------------------------
// a batch of dense QPs  min 1/2 x'Px + q'x  s.t.  Gx <= h  and its iterates, as the C entries take them
struct QpBatch {
  int no, nc, batch;
  const double *P, *q, *G, *h;
  double *x, *y, *z;
};
// what the solve mode adds to a kernel's arguments (unused by the plain iteration)
struct SolveArgs {
  double* rho;        // [batch] in: the step an instance starts with; out: the one it ended with
  int32_t* status;    // [batch] MPCASM_QP_*
  int32_t* iters;     // [batch] the iterations an instance ran
  double eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
  int check_every, adaptive_rho_interval;
};
// the settings of a solve: the kernel's own part and what the launch passes beside it (mpcasm_admm: max_iter is
// `iters`, the step a scalar of its own)
struct QpSolve : SolveArgs {
  double sigma, alpha;
  int max_iter, warm;
  double* kinv;
  int kinv_valid;
  double* res;
};
// soft limits (mpcasm_qp_solve_soft, mpcasm_qp_solve_wide_soft): row i costs lin_i t + 1/2 quad_i t^2 for
// t = (Gx - h)_i > 0; lin_i = +inf is a hard row.  [batch][nc] at `stride` doubles (0: one pair for the batch)
struct QpSoft {
  const double *lin, *quad;
  int64_t stride;
};
// what a soft instantiation's kernel takes in SolveArgs' place
struct SoftSolveArgs : SolveArgs {
  QpSoft soft;
};
struct QpPolish {
  const int32_t* status;
  double delta;
  int refine_iters;
  int32_t* polish;
  double* res;
};
// the sensitivity of a batch of solved QPs (mpcasm_qp_sens, mpcasm_qp_sens_wide): operands, the iterate, the
// right-hand side, the polish's settings and the outputs (gP, gG, lres: null for "not wanted")
struct QpSens {
  int no, nc, batch;
  const double *P, *G, *h, *x, *y, *z;
  const int32_t* status;
  const double *rx, *ry;
  double delta;
  int refine_iters;
  double *u, *w, *gP, *gG;
  int32_t* verdict;
  double* lres;
};

// the launch of a kernel, the only one outside resident.hip's launch_jc and jit.hip (`lds`: its dynamic LDS, 0 for
// none): more than a workgroup may have -> MPCASM_ERR_LIMIT; more than 64 KiB -> allow_whole_lds first; *err is the
// runtime's word where MPCASM_ERR_HIP comes back.  A sequence of launches returns at the first not MPCASM_OK.
template <typename... Params, typename... Args>
int launch_with_lds(void (*kernel)(Params...), dim3 grid, int block, size_t lds, hipStream_t stream, hipError_t* err,
                    Args... args) {
  if (lds > (size_t)RESIDENT_LDS_LIMIT) return MPCASM_ERR_LIMIT;
  if (lds > 64 * 1024) {
    *err = allow_whole_lds(reinterpret_cast<const void*>(kernel));
    if (*err != hipSuccess) return MPCASM_ERR_HIP;
  }
  hipLaunchKernelGGL(kernel, grid, dim3((unsigned)block), lds, stream, args...);
  *err = hipGetLastError();
  return *err == hipSuccess ? MPCASM_OK : MPCASM_ERR_HIP;
}

size_t admm_lds_bytes(int no, int nc);   // (one instance of mpcasm_admm or mpcasm_qp_solve)
int launch_admm(const QpBatch& b, double rho, const QpSolve& s, hipStream_t stream, hipError_t* err);
int launch_qp_solve(const QpBatch& b, const QpSolve& s, hipStream_t stream, hipError_t* err);
// admm_wide.hip: the solve to tolerance with G read in place and K^-1 in LDS or in d_kinv
int qp_solve_wide_info(int no, int nc, int64_t* lds_bytes, int32_t* kinv_on_chip);
int launch_qp_solve_wide(const QpBatch& b, const QpSolve& s, hipStream_t stream, hipError_t* err);
// the soft instantiations of the two solves: the penalty vectors on chip beside h
size_t admm_soft_lds_bytes(int no, int nc);
int launch_qp_solve_soft(const QpBatch& b, const QpSolve& s, const QpSoft& soft, hipStream_t stream, hipError_t* err);
int qp_solve_wide_soft_info(int no, int nc, int64_t* lds_bytes, int32_t* kinv_on_chip);
int launch_qp_solve_wide_soft(const QpBatch& b, const QpSolve& s, const QpSoft& soft, hipStream_t stream,
                              hipError_t* err);
// polish.hip: OSQP's polishing of solved instances (active-set KKT solve with refinement)
size_t polish_lds_bytes(int no, int nc);
int launch_qp_polish(const QpBatch& b, const QpPolish& p, hipStream_t stream, hipError_t* err);
// polish_wide.hip: the same polish with G and P read in place and the matrices of the KKT solve in a workspace of
// the caller's, one slice per workgroup of a launch of min(batch, POLISH_WIDE_CAP) workgroups
constexpr int POLISH_WIDE_CAP = MPCASM_POLISH_WIDE_CAP;
int qp_polish_wide_info(int no, int nc, int batch, int64_t* lds_bytes, int64_t* work_bytes, int32_t* workgroups);
int launch_qp_polish_wide(const QpBatch& b, const QpPolish& p, double* work, hipStream_t stream, hipError_t* err);
// sens_core.h in polish.hip and polish_wide.hip: one more solve with the polish's KKT system and the caller's
// right-hand side, on the polish's LDS layout, workspace and launch geometry (their sizes are the polish's)
int launch_qp_sens(const QpSens& s, hipStream_t stream, hipError_t* err);
int launch_qp_sens_wide(const QpSens& s, double* work, hipStream_t stream, hipError_t* err);
// warm.hip: a closed loop's warm store -- the scatter after a solve, the shifted start before the next
int launch_qp_warm_store(int no, int nc, const double* x, const double* y, const double* rho, const int32_t* status,
                         int tag, double* sx, double* sy, double* srho, int32_t* smeta, int64_t store_rows,
                         int store_no, int store_nc, const int32_t* index, int count, hipStream_t stream,
                         hipError_t* err);
int launch_qp_warm_start(int no, int nc, const double* G, const double* h, const double* sx, const double* sy,
                         const double* srho, const int32_t* smeta, int64_t store_rows, int store_no, int store_nc,
                         const int32_t* index, const int32_t* col_src, const int32_t* row_src, int expect_tag,
                         uint32_t warm_mask, double rho_cold, double* x, double* y, double* z, double* rho,
                         int32_t* warm, int count, hipStream_t stream, hipError_t* err);
// params.hip: a closed loop's commands -- per-walker command columns into the parameter rows of a launch
int launch_params_map(double* params, int64_t n_params, const int32_t* recs, const double* coef, int nrecs,
                      const double* cmd, int64_t cmd_stride, int ncmd, const int32_t* index, const double* sign,
                      int batch, hipStream_t stream, hipError_t* err);
int launch_preview(const double* PM, const double* given, const double* optim, double* out,
                   int batch, int rows, int ng, int no, hipStream_t stream, hipError_t* err);

}  // namespace mpcasm
