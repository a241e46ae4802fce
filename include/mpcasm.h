/*
 * mpcasm.h -- C ABI of libmpcasm.so, the MI355X (gfx950) batched QP-assembly
 * engine behind the mpc_interface problem-description API.
 *
 * The reference (Gepetto/mpc-interface) has no native boundary on this path:
 * everything is numpy inside one Python process.  Each entry point below
 * replaces the reference function cited next to it (paths relative to the
 * reference checkout); INTEGRATION.md shows the ctypes stubs a maintainer of
 * the reference would add to call them.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer named d_* is a DEVICE pointer
 *     (hipMalloc'ed or a torch-ROCm tensor's data_ptr()), h_* is a HOST pointer;
 *   - the caller owns every buffer; the library allocates only the device copy
 *     of a plan's tables, released by mpcasm_plan_destroy;
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as
 *     void*, NULL = default stream); no call synchronises the device;
 *   - every function returns MPCASM_OK (0) or a negative mpcasm_status; no
 *     exception crosses the boundary;
 *   - all floating point data is IEEE binary64, row-major, densely packed.
 */
#ifndef MPCASM_H
#define MPCASM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mpcasm_status {
  MPCASM_OK = 0,
  MPCASM_ERR_ARG = -1,      /* null pointer, non-positive size, bad flag        */
  MPCASM_ERR_PLAN = -2,     /* malformed plan tables (magic/version/bounds)     */
  MPCASM_ERR_HIP = -3,      /* a HIP runtime call failed (see mpcasm_last_hip)  */
  MPCASM_ERR_NODEVICE = -4, /* no HIP device visible                            */
  MPCASM_ERR_LIMIT = -5     /* problem exceeds a kernel limit (LDS, sources)    */
} mpcasm_status;

typedef struct mpcasm_plan mpcasm_plan; /* opaque, immutable after creation */

/* library / device ------------------------------------------------------- */

/* ABI version of this header (major*1000 + minor).  1004 with mpcasm_staged_route.  1003 for the build that added
 * mpcasm_qp_solve_wide and also for the build that added mpcasm_ltv_rollout_compile,
 * mpcasm_ltv_rollout and mpcasm_ltv_advance, for the one that added mpcasm_qp_polish_wide and
 * mpcasm_qp_polish_wide_info, for the one that added mpcasm_ltv_rollout_info, for the one that added mpcasm_ltv_lqr,
 * mpcasm_ltv_close and mpcasm_ltv_true_inputs, for the one that added mpcasm_ltv_augment, for the one that added
 * mpcasm_qp_solve_soft, mpcasm_qp_solve_wide_soft and their two info entries and for the one that added
 * mpcasm_qp_sens, mpcasm_qp_sens_wide and their two info entries and for the one that added mpcasm_assemble_jvp,
 * mpcasm_assemble_vjp and mpcasm_assemble_adjoint_info and for the one that added mpcasm_assemble_route and for the one that
 * added mpcasm_assemble_params_vjp and mpcasm_assemble_params_vjp_info (the project's tests pin
 * the value): a client cannot tell from this number whether
 * those entries are there -- look the symbols up (dlsym) instead. */
int mpcasm_abi_version(void);
/* Number of visible HIP devices (0 when none; never fails). */
int mpcasm_device_count(void);
/* Last hipError_t seen by the calling thread inside the library (0 = none). */
int mpcasm_last_hip(void);
/* Static string for a status code. */
const char* mpcasm_status_string(int status);
/* Process-wide options.  MPCASM_OPT_PATH selects the assembly kernels: 0 = best
 * available (persistent fused kernel when one instance fits on chip), 1 = never
 * the persistent kernel (per-instance fused kernel if it fits; the tiled kernel's scan form with its
 * pre-passes instead of the set-up fused into it), 2 = always the
 * staged K2 -> K3 -> K4 pipeline with the workspace in HBM, 3 = as 1, and a wide problem whose
 * rows are windows of generated horizon tables still composes its tiles (the tiled kernel's
 * general form instead of its Toeplitz form), 4 = as 1, and such a problem multiplies its windows
 * on the matrix core even where every Hessian term is the full horizon of one state (the tiled
 * kernel's Toeplitz form instead of its scan form, which sums P along diagonals).  The parity
 * tests use it to exercise every path; all paths give the same results. */
enum { MPCASM_OPT_PATH = 1, MPCASM_OPT_PHASE_MASK = 2, MPCASM_OPT_RESIDENT_PER_CU = 3, MPCASM_OPT_JIT = 4,
       MPCASM_OPT_P_DIRECT = 5, MPCASM_OPT_RESIDENT_GRID = 6, MPCASM_OPT_JIT_FETCH_RUNS = 7 };
/* MPCASM_OPT_PHASE_MASK is a profiling aid (timing-only ablation of the fused
 * kernels: bit 0 compose, 1 Hessian, 2 gradient, 3 constraints, 4 input staging
 * after the first instance, 5 P/q stores, 7 register prefetch of the next instance's
 * inputs; bit 6, off by default, makes the persistent kernel also write per-wavefront
 * cycle sums of its phases into d_work, which mpcasm_workspace_bytes sizes for it;
 * default 0xBF).  Results are WRONG with any of bits 0-5 cleared -- never use it
 * outside a profile.  Bits 8-14 are A/B aids of the persistent kernel that leave the results
 * right: 8 no runs of four consecutive instances per workgroup, 10-12 runs of 2^k instead,
 * 13 the workgroups of one XCD take neighbouring instances, 14 every workgroup starts its G and
 * P streams at their first line (default: at a line of its own); bit 9 computes G without
 * storing it (results WRONG).
 * MPCASM_OPT_RESIDENT_PER_CU (tuning aid): workgroups of the persistent kernel per CU;
 * 0 (default) = chosen from the batch size, never more than are resident at once.
 * MPCASM_OPT_RESIDENT_GRID: at most this many workgroups of the persistent kernel per launch
 * (0, the default: all that are resident at once).  For callers that run launches of several plans
 * side by side on streams of their own (the structure buckets of a walker fleet): every launch gets
 * its share of the chip's workgroup slots and none waits for another to drain.
 * MPCASM_OPT_JIT: the persistent kernel compiled for the very plan by hiprtc (its sizes and
 * matrix-core trip lists become constants; same source, same results as the ahead-of-time
 * kernel): 0 (default) = for batches of at least 512 instances, when libhiprtc.so is there
 * (compiled once per plan structure and device, on the first such launch: that launch blocks
 * for the compilation, a second or two); 1 = for every batch; 2 = never.
 * MPCASM_OPT_JIT_FETCH_RUNS (test aid, 0 .. 8, default 8): a chunk of the fetch tables with more runs of
 * streams than this stays on the table path of the per-plan kernel (mpcasm_fetch_segments); read when a
 * plan's kernel is first compiled and by mpcasm_jit_check, so that a small plan exercises both ways.
 * MPCASM_OPT_P_DIRECT (read by mpcasm_plan_create): how the persistent kernel writes P -- 1: its
 * 4x4 blocks go from the matrix core straight to HBM; 2: collected in LDS and copied out with
 * 16-byte stores whenever P fits there beside the workspace; 0 (default): as 1 when the launch
 * writes less than ~0.55 GB, or when P in LDS would cost a workgroup per CU and an instance's
 * results are small (< 128 KB), else as 2.
 * These options are process-wide test / tuning hooks.  Every launch reads them once, when it starts, into a
 * record of its own that travels with it: a change made while other threads launch is seen whole by the launches
 * that start after it and not at all by those under way (the values are atomic, there is no data race) -- but
 * which launches those are is the caller's to order.  A caller with several plans on several threads uses
 * mpcasm_plan_set_option. */
int mpcasm_set_option(int option, int value);
/* The same choice for ONE plan (MPCASM_OPT_PATH, MPCASM_OPT_JIT, MPCASM_OPT_RESIDENT_PER_CU,
 * MPCASM_OPT_RESIDENT_GRID; value
 * -1: back to the process-wide value): part of the plan's state, read by every mpcasm_assemble on
 * it -- what a caller with several plans on several threads uses instead of the hooks above. */
int mpcasm_plan_set_option(mpcasm_plan* plan, int option, int value);
/* Needs no device: validates the tables as mpcasm_plan_create does and reports the dynamic LDS
 * bytes one workgroup of the persistent kernel needs for them -- out[0] with P handed over
 * directly, out[1] with P collected in LDS (0: the plan does not run on the persistent kernel).
 * Two workgroups share a CU's 160 KB: a plan compiler uses it to pick the layout of the workspace
 * that fits two (mpcasm.engine.Assembler, workspace="auto"). */
int mpcasm_resident_lds_bytes(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                              int64_t out[2]);
/* Diagnostic, needs no device: validates the tables as mpcasm_plan_create does, generates the
 * per-plan constants and compiles the persistent kernel for them with hiprtc (gfx950).
 * MPCASM_OK, MPCASM_ERR_LIMIT (no persistent kernel for this plan, or no libhiprtc.so) or
 * MPCASM_ERR_HIP (compilation failed); the compiler's log goes to `log` (may be NULL). */
int mpcasm_jit_check(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                     char* log, size_t log_capacity);
/* Diagnostic, needs no device: how the per-plan kernel fetches the plan's inputs.  The fetch tables
 * (one (stream, byte offset) per lane and 64-lane chunk: the (A, B) of the generated systems, then the
 * image) are contiguous runs of streams and padding, and the per-plan kernel gets every chunk of at
 * most `limit` runs (at most 8) as constants and works its lanes' addresses out by arithmetic; a
 * chunk with more stays on the table.  Writes per chunk: kind (0: (A, B), 1: image), chunk, runs (0:
 * on the table), then per run 6 words -- first lane, lanes, stream, first byte, bytes per lane step,
 * period in lanes: lane l reads byte first + ((l - first lane) % period) * step of the stream.
 * *n_words: the words that make up the answer; MPCASM_ERR_LIMIT when `capacity` is too small for
 * them or the plan does not run on the persistent kernel. */
int mpcasm_fetch_segments(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                          int limit, int32_t* out, size_t capacity, int64_t* n_words);

/* Compile ahead of the first launch what a launch of `batch` instances of this plan would
 * compile (the persistent kernel specialised for the plan, MPCASM_OPT_JIT): a control loop calls
 * it once with the plan's capacity, so that no tick ever blocks for a compilation; launches of
 * fewer instances then run the compiled kernel too.  Other plans keep launching meanwhile (the
 * compilation holds no lock).  Code objects are kept on disk -- $MPCASM_CACHE_DIR, else
 * $XDG_CACHE_HOME/mpcasm, else ~/.cache/mpcasm; MPCASM_NO_DISK_CACHE=1: never -- named by a hash of
 * everything the compiler sees, so every later process (and the other ranks of a node) loads
 * instead of compiling.  MPCASM_OK also when nothing needs compiling or hiprtc is missing (the
 * ahead-of-time kernel runs then); MPCASM_ERR_ARG when the current device is not the plan's. */
int mpcasm_plan_prepare(const mpcasm_plan* plan, int batch);
/* Diagnostic: out[0] = kernels compiled by this process so far, out[1] = code objects loaded from
 * the disk cache, out[2] = code objects written to it. */
int mpcasm_jit_stats(int64_t out[3]);

/* K1  horizon extension ---------------------------------------------------
 * Replaces tools.extend_matrices(N, A, B)      python/mpc_interface/tools.py:14-33
 * (C++ twin gecko::tools::extend_matrices      cpp/src/tools.cc:83-144),
 * batched over `batch` independent systems.
 *
 *   ltv == 0:  d_A [batch][n][n],     d_B [batch][n][m]      x+ = A x + B u
 *   ltv == 1:  d_A [batch][N][n][n],  d_B [batch][N][n][m]   x_{k+1} = A_k x_k + B_k u_k
 *   d_S [batch][N][n][n]      S[b][k][j][i]    = (A^{k+1})[i][j]          (A_k...A_0 when ltv)
 *   d_U [batch][m][N][N][n]   U[b][j][k][l][i] = (A^{k-l} B)[i][j], l<=k  (A_k..A_{l+1} B_l when ltv)
 *                                              = 0,                 l>k
 * i.e. U[b][j] is the reference's list element U[j] (shape N x N x n).
 * Every byte of S and U is written (zeros included).
 */
int mpcasm_fill_su(const double* d_A, const double* d_B, double* d_S, double* d_U,
                   int batch, int N, int n, int m, int ltv, void* stream);

/* plans -------------------------------------------------------------------
 * A plan is the compiled *structure* of one Formulation (index maps, flattened
 * definition graph, cost and constraint tables): what the reference re-derives
 * from dicts on every call of
 *   Formulation.make_preview_matrices          python/mpc_interface/body.py:149-193
 *   Formulation.generate_all_qp_constraints    body.py:304-320
 *   Formulation.generate_all_qp_costs          body.py:322-329
 * The tables are produced by the host plan compiler (mpcasm/plan.py); their
 * layout is documented in csrc/plan_tables.h.  h_itab / h_dtab are copied.
 */
int mpcasm_plan_create(const int32_t* h_itab, size_t n_itab,
                       const double* h_dtab, size_t n_dtab,
                       mpcasm_plan** out_plan);
int mpcasm_plan_destroy(mpcasm_plan* plan);

/* Sizes of a plan: out[0]=given_len ng, out[1]=optim_len no, out[2]=rows of
 * the stacked G (nc), out[3]=params per instance, out[4]=number of sources,
 * out[5]=row-set rows, out[6]=leading dimension of the workspace rows,
 * out[7]=preview rows (sum over definitions). */
int mpcasm_plan_sizes(const mpcasm_plan* plan, int64_t out[8]);

/* f3  sparse hand-off, first form: a plan compiled with csc=... (mpcasm/plan.py) makes
 * mpcasm_assemble write the `data` arrays of
 *   Q = scipy.sparse.csc_matrix(Q); A = scipy.sparse.csc_matrix(A)
 *   python/use_examples/simple_functional_example/biped_mpc_loop.py:57-58
 * directly -- d_P is then [batch][out[0]], d_G [batch][out[1]] (both 0 for a dense plan);
 * indptr / indices are the plan compiler's, one pattern for the whole batch (entries that
 * happen to be 0.0 are stored).  Such a plan exists on the persistent kernel only:
 * mpcasm_plan_create answers MPCASM_ERR_LIMIT when the problem does not fit on chip (assemble
 * dense and convert with mpcasm_gather then). */
int mpcasm_plan_csc_sizes(const mpcasm_plan* plan, int64_t out[2]);

/* Bytes of scratch the assembly of `batch` instances needs (device memory,
 * caller-allocated, 16-byte aligned): a part per instance and, for wide problems, a part per launch
 * behind it (the shared-model form's tables) -- a buffer sized for a larger batch serves every
 * smaller one. */
int mpcasm_workspace_bytes(const mpcasm_plan* plan, int batch, size_t* out_bytes);

/* K2+K3+K4  batched QP assembly --------------------------------------------
 * Replaces, for `batch` instances of one structure,
 *   Formulation.generate_all_qp_matrices(given)  body.py:333-348
 * on top of the preview matrices of make_preview_matrices (body.py:149-193):
 *
 *   h_src        host array of plan.n_sources DEVICE pointers: the horizon
 *                matrices ExtendedSystem.matrices[k] ([N][p][n] each,
 *                dynamics.py:199) the definitions read
 *   h_src_stride host array, elements between consecutive instances of each
 *                source (0 = one copy shared by the whole batch)
 *   d_params     [batch][n_params]  per-instance Cost / Constraint numbers
 *                (weight, aim, cross_aim; arrow, center, extreme)
 *   d_given      [batch][ng]        the 'given' vector (body.py:195-207)
 *   d_P [batch][no][no]  d_q [batch][no]  d_G [batch][nc][no]  d_h [batch][nc]
 *                qpsolvers layout: minimise 1/2 x'Px + q'x  s.t.  Gx <= h
 *                (the reference returns them as A=G, h, Q=P, q).
 *   d_work       scratch of mpcasm_workspace_bytes(plan, batch)
 *
 * Any of d_P/d_q (both) or d_G/d_h (both) may be NULL to skip that half.  The result
 * buffers are 16-byte aligned (MPCASM_ERR_ARG otherwise).
 *
 * K1 fused (plans compiled with lti=[...], mpcasm/plan.py): for a dynamics whose
 * horizon matrices are generated on chip, i.e. what
 *   tools.extend_matrices(N, A, B)             python/mpc_interface/tools.py:14-33
 * would have produced from the system's (A, B), the slot of the group's FIRST
 * horizon matrix (U_0) carries A [n][n] and the slot of its SECOND one (U_1, or S
 * when m = 1) carries B [n][m], each with its own per-instance stride (n*n, n*m or
 * 0); the group's other slots are ignored.  Such a plan runs in the persistent
 * kernel only: MPCASM_ERR_LIMIT when one instance does not fit on chip, and
 * mpcasm_preview_matrices refuses it (there is no S, U to read).
 */
int mpcasm_assemble(const mpcasm_plan* plan, const double* const* h_src,
                    const int64_t* h_src_stride, const double* d_params,
                    const double* d_given, double* d_P, double* d_q, double* d_G,
                    double* d_h, void* d_work, int batch, void* stream);

/* The same with the rows of d_given picked by an index: instance b reads d_given[d_given_index[b]]
 * and row b of everything else (parameters, per-instance sources; results to row b).  What a walker
 * fleet's structure bucket needs (biped_mpc_loop.py:41-56 for many walkers: the bucket's walkers are
 * scattered over the fleet-wide `given`): no gather pass in front of the assembly.  Persistent kernel
 * only: MPCASM_ERR_LIMIT for a plan that runs elsewhere (gather the rows and call mpcasm_assemble).
 * Every d_given_index[b] must lie in [0, rows of d_given): the kernel does not check it. */
int mpcasm_assemble_indexed(const mpcasm_plan* plan, const double* const* h_src,
                            const int64_t* h_src_stride, const double* d_params, const double* d_given,
                            const int32_t* d_given_index, double* d_P, double* d_q, double* d_G,
                            double* d_h, void* d_work, int batch, void* stream);

/* Which kernels the latest successful mpcasm_assemble on this plan launched (a record for
 * benchmarks and tests; 0 before the first launch): the persistent kernel ahead of time / compiled
 * for the plan, the per-instance fused kernel, the staged K2 -> K3 -> K4 pipeline, the tiled
 * kernel for wide problems.  With two threads launching on one plan the record is the last writer's. */
enum { MPCASM_KERNEL_NONE = 0, MPCASM_KERNEL_RESIDENT = 1, MPCASM_KERNEL_RESIDENT_JIT = 2,
       MPCASM_KERNEL_FUSED = 3, MPCASM_KERNEL_STAGED = 4, MPCASM_KERNEL_TILED = 5,
       MPCASM_KERNEL_TILED_SCAN = 6 /* the tiled kernel's scan form: P summed along diagonals */,
       MPCASM_KERNEL_SWEEP = 7 /* per-step dynamics (a plan compiled with ltv): no horizon matrix */,
       MPCASM_KERNEL_TILED_SHARED = 8 /* wide problem, every source shared by the batch: P and G as
                                         weighted sums of matrices computed once per launch */ };
int mpcasm_plan_last_kernel(const mpcasm_plan* plan);

/* K2 alone  preview matrices ------------------------------------------------
 * Replaces Formulation.make_preview_matrices   body.py:149-193
 * d_PM [batch][preview_rows][ng+no]: for every definition, in definition
 * order, the rows of [Mg | Mo] (Formulation.PM[var] = (Mg, Mo)).
 * Like every entry that launches with a plan's tables: MPCASM_ERR_ARG when the
 * current device is not the one the plan was created on.  (Until the entries
 * shared that check this one had none and launched there; ABI 1004 as before.)
 */
int mpcasm_preview_matrices(const mpcasm_plan* plan, const double* const* h_src,
                            const int64_t* h_src_stride, double* d_PM, int batch,
                            void* stream);

/* f2  batched preview --------------------------------------------------------
 * Replaces Formulation.preview(given, optim, variable)   body.py:209-219
 * for every definition at once: d_out[batch][preview_rows] =
 *   Mg @ given + Mo @ optim  with d_PM as written by mpcasm_preview_matrices.
 */
int mpcasm_preview(const double* d_PM, const double* d_given, const double* d_optim,
                   double* d_out, int batch, int rows, int ng, int no, void* stream);

/* f2, straight from the sources: the same rows without a preview matrix in memory.
 * Replaces Formulation.preview(given, optim, variable)   body.py:209-219
 * for every definition at once: d_out[batch][preview_rows] = Mg @ given + Mo @ optim, every row
 * evaluated as its combination of base rows (rows of the horizon matrices times [given ; optim],
 * kept on chip).  h_src / h_src_stride as for mpcasm_assemble; a plan compiled with lti=[...]
 * takes the groups' (A, B) in the same slots and needs d_work (mpcasm_workspace_bytes) for the
 * horizon tables it generates first. */
int mpcasm_preview_direct(const mpcasm_plan* plan, const double* const* h_src,
                          const int64_t* h_src_stride, const double* d_given, const double* d_optim,
                          double* d_out, void* d_work, int batch, void* stream);

/* f2  goal distances --------------------------------------------------------------
 * Replaces Formulation.goal_distance(given, optim, goal_name)   body.py:221-228
 * (and full_goal_distance, :230-234: the sum over the goals) for a batch, from the rows
 * mpcasm_preview_direct / mpcasm_preview wrote:
 *   d_out[b][g] = sum over the terms t of goal g (one per axis)
 *                 sum_{r < rows_t} (d_preview[b][row0_t + r] - d_params[b][aim_t])^2
 * d_terms: nterms records of 4 int32 -- goal, row0, rows, aim's parameter slot.  As in the
 * reference the whole variable counts, whatever the goal's schedule or L. */
int mpcasm_goal_distance(const double* d_preview, int64_t preview_stride, const double* d_params,
                         int64_t n_params, const int32_t* d_terms, int nterms, int ngoals,
                         double* d_out, int batch, void* stream);

/* ... and the same distances straight from the sources, without the rows ever leaving the chip:
 * what full_goal_distance needs after a solve (body.py:230-234) -- 8 bytes per goal and instance
 * instead of 8 bytes per row of every definition.  Arguments as mpcasm_preview_direct + the goal
 * table of mpcasm_goal_distance; d_out[batch][ngoals].  MPCASM_ERR_LIMIT when the plan does not run
 * on the kernel that does this (sources of an instance's own, more than 16 terms, rows of one
 * instance beyond LDS): take the rows with mpcasm_preview_direct and call mpcasm_goal_distance. */
int mpcasm_preview_goal_distance(const mpcasm_plan* plan, const double* const* h_src,
                                 const int64_t* h_src_stride, const double* d_given,
                                 const double* d_optim, const double* d_params, const int32_t* d_terms,
                                 int nterms, int ngoals, double* d_out, void* d_work, int batch,
                                 void* stream);

/* Diagnostic, needs no device: which kernel mpcasm_preview_direct (ngoals == 0) or
 * mpcasm_preview_goal_distance (its nterms, ngoals) launches for these tables -- validated as
 * mpcasm_plan_create does -- when the sources have the strides h_src_stride (as for mpcasm_assemble:
 * 0 for a source the batch shares; may be NULL when the plan has no source).  The launches take the same
 * decision from the same function, MPCASM_PREVIEW_NO_BLOCKS included.  out[0]: MPCASM_PREVIEW_*;
 * out[1..4]: the template arguments E1, R1, E2, R2 of the kernel's instantiation (entries per base row,
 * base rows per thread, entries per definition row, definition rows per thread; 0 on the direct
 * kernel); out[5]: 1 when the kernel writes the goal distances itself; out[6]: dynamic LDS bytes of a
 * workgroup; out[7]: 1 when that is more than 64 KB (the whole-LDS attribute is set before the launch).
 * MPCASM_ERR_LIMIT exactly where the launch would return it (out is zeroed): for the distances, the
 * caller then takes the rows and mpcasm_goal_distance. */
enum { MPCASM_PREVIEW_NONE = 0 /* no rows: nothing is launched */, MPCASM_PREVIEW_DIRECT = 1,
       MPCASM_PREVIEW_STAGED = 2 /* the plan's tables in registers, the streams in LDS */,
       MPCASM_PREVIEW_BLOCKED = 3 /* ... every stream shared by the batch: four instances at a time */ };
int mpcasm_preview_route(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                         const int64_t* h_src_stride, int nterms, int ngoals, int32_t out[8]);

/* Diagnostic, needs no device: what mpcasm_assemble launches for the tables of a plan with a dynamics compiled
 * as ltv (the sweep kernel; tables validated as mpcasm_plan_create does).  The launch takes the decision from
 * the same function.  out[0]: CPT, the columns a thread owns (1, 2, 4); out[1]: 1 for the instantiation with
 * the system's sizes as constants (3 states, 1 input, 2 axes), else 0; out[2]: 1 when a thread's two columns
 * are neighbours (PAIR); out[3]: 1 when the weights of G's lines are kept per line (a limit whose arrow
 * changes from line to line), 0 per limit; out[4]: the regular lines, 0 .. 4 (the first lines of every step
 * that belong to the same limits, a row further down G per step); out[5]: LR, the lines of a step fetched at
 * once where no line is regular (8, 4, 2 by CPT); out[6]: dynamic LDS bytes of a workgroup; out[7]: 1 when
 * that is more than 64 KB.  MPCASM_ERR_LIMIT exactly where the launch returns it (out is zeroed): more than
 * 1024 unknowns, a system beyond 4 states / 4 inputs / 4 axes, LDS beyond a CU's.  MPCASM_ERR_ARG for a plan
 * that does not run on the sweep kernel. */
int mpcasm_sweep_route(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab, int32_t out[8]);

/* Diagnostic, needs no device: what mpcasm_fill_su launches for `batch` systems of these sizes (ltv: 0 / 1) when
 * d_S and d_U are both 16-byte aligned (aligned16 = 1) or not (0: the QUAD and LTV_ROW kernels and the LTI
 * kernel's PAD form are passed over; the kernels that take the launch instead still store 16-byte words where
 * N n is even, at addresses that are then only 8-byte aligned).  The launch takes the decision from the same function, MPCASM_FILL_MIN_WAVES (read once per
 * process) included.  out[0]: the kernel, MPCASM_FILL_*; out[1]: its integer template argument -- NS, the
 * number of states as a constant, for QUAD, LTV_ROW and LTV_BLOCK (there 0 = any), TPI, the threads per system
 * (64 or 256), for LTI and LTV, 0 otherwise; out[2]: flags, MPCASM_FILL_GENERIC | MPCASM_FILL_PAD (the LTI
 * kernel's template arguments) | MPCASM_FILL_WHOLE_LINES (QUAD: rows of U are whole 128-byte lines and leave
 * with nontemporal stores); out[3]: systems per wavefront (QUAD, TINY; else 0); out[4]: QUAD: log2 of the
 * lanes that share a short row (rows per store instruction = 64 >> out[4]); out[5]: workgroups; out[6]:
 * dynamic LDS bytes of a workgroup; out[7]: 1 when that is more than 64 KB.  MPCASM_ERR_LIMIT exactly where
 * the launch returns it (out is zeroed): one system's tables beyond the 156 KB of LDS a workgroup is granted
 * (a quad-kernel shape beyond them goes to the kernels behind it), or per-step systems of more than 256 states.
 * MPCASM_ERR_ARG as mpcasm_fill_su (batch < 1 here: an empty batch launches nothing). */
enum { MPCASM_FILL_QUAD = 1 /* n <= 4: recurrence in registers, several systems per wavefront */,
       MPCASM_FILL_TINY = 2 /* n (m + n) <= 32: several systems per wavefront, recurrence in LDS */,
       MPCASM_FILL_LTI = 3, MPCASM_FILL_LTV_ROW = 4 /* per-step, n <= 4: a wavefront per system */,
       MPCASM_FILL_LTV_BLOCK = 5 /* per-step, a workgroup per system, every step's matrices in LDS */,
       MPCASM_FILL_LTV_WAVE = 6 /* per-step, a wavefront per system, step matrices fetched a step ahead */,
       MPCASM_FILL_LTV = 7 };
enum { MPCASM_FILL_GENERIC = 1, MPCASM_FILL_PAD = 2, MPCASM_FILL_WHOLE_LINES = 4 };
int mpcasm_fill_route(int batch, int N, int n, int m, int ltv, int aligned16, int32_t out[8]);

/* Diagnostic, needs no device: what mpcasm_assemble launches for the tables of a plan that runs on the tiled
 * path (128 unknowns or more, not on chip, no dynamics compiled as ltv; tables validated as mpcasm_plan_create
 * does), for a launch of `batch` instances whose sources have the strides h_src_stride (as for mpcasm_assemble:
 * 0 for a source the batch shares; may be NULL when the plan has no source), that wants the halves `want`
 * (MPCASM_WANT_COST | MPCASM_WANT_CONSTRAINTS) under MPCASM_OPT_PATH `path` (0 .. 4; -1: the process-wide value).
 * The launch takes the decision from the same function.  out[0]: the form, MPCASM_TILED_*; scan form:
 * out[1]: 1 when the kernel makes its table and d itself (fused), 0 behind the pre-passes; out[2], out[3]: KP, CB
 * of the instantiation (Hessian terms and column blocks in registers); out[4]: 1 when the records of G's rows
 * ride in LDS; out[5]: 1 when results leave as whole 128-byte lines.  out[6]: dynamic LDS bytes of a workgroup
 * of the scan or the Toeplitz kernel; out[7]: 1 when that is more than 64 KB; out[8]: the pre-pass that makes
 * the horizon tables, MPCASM_TILED_TABLES_*; out[9]: TG of the shared-model form's kernel for P (4 .. 32; 0: P
 * not wanted or no weight); out[10]: 1 when only the lower block pairs of P are multiplied (Toeplitz, general
 * and shared form); out[11 .. 15]: 0.  MPCASM_ERR_LIMIT exactly where the launch returns it (out is zeroed):
 * a generated system beyond 64 states or n (m + n) > 2048, or one whose horizon tables the per-system pre-pass
 * (MPCASM_TILED_TABLES_SYSTEM) would make with more than 64 KB of dynamic LDS, (n n + 2 n (m + n) + 16 n m) 8
 * bytes -- nothing is launched -- that the fused scan form does not take.
 * MPCASM_ERR_ARG for a plan that does not run on the tiled path -- the persistent kernel takes a plan that
 * fits on chip first (input alignment, a property of the launch's pointers, is taken as given). */
enum { MPCASM_TILED_SCAN = 1, MPCASM_TILED_TOEPLITZ = 2, MPCASM_TILED_SHARED = 3, MPCASM_TILED_GENERAL = 4 };
enum { MPCASM_TILED_TABLES_NONE = 0, MPCASM_TILED_TABLES_SMALL = 1 /* a wavefront per few systems */,
       MPCASM_TILED_TABLES_SYSTEM = 2 /* a workgroup per system */ };
enum { MPCASM_WANT_COST = 1, MPCASM_WANT_CONSTRAINTS = 2 };
int mpcasm_tiled_route(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                       const int64_t* h_src_stride, int batch, int want, int path, int32_t out[16]);

/* Diagnostic, needs no device: which kernel family mpcasm_assemble (indexed = 0) or mpcasm_assemble_indexed
 * (indexed = 1) runs a launch of `batch` instances of these tables on (validated as mpcasm_plan_create does), under
 * MPCASM_OPT_PATH `path` (0 .. 4; -1: the process-wide value), when the launch's inputs meet the alignment the
 * persistent kernel's 16-byte loads assume (inputs_aligned = 1: `given`, the parameters and the sources it reads
 * that way 16-byte aligned with even strides) or not (0).  The launch takes the decision from the same function.
 * The order: the sweep kernel for a plan with a dynamics compiled as ltv; the persistent kernel when an instance
 * fits a CU's LDS, the inputs are aligned and `path` is 0 (any `path` for a plan compiled with lti=[...] or with
 * results in CSC form, which run nowhere else on chip); the tiled kernel for a wide problem unless `path` is 2;
 * the per-instance fused kernel while two workgroups fit a CU and `path` is at most 1; else the staged pipeline.
 * out[0]: MPCASM_KERNEL_* -- the persistent kernel always as MPCASM_KERNEL_RESIDENT (whether the launch takes the
 * kernel compiled for the plan depends on the batch, MPCASM_OPT_JIT and the runtime: mpcasm_plan_last_kernel may
 * say MPCASM_KERNEL_RESIDENT_JIT for the same route), the tiled path always as MPCASM_KERNEL_TILED (its form:
 * mpcasm_tiled_route); out[1]: dynamic LDS bytes of a workgroup of the persistent or the fused kernel, else 0;
 * out[2]: 1 when the persistent kernel hands P over directly at this batch, 0 through LDS (as out[0] / out[1] of
 * mpcasm_resident_lds_bytes); out[3]: 0.  MPCASM_ERR_LIMIT exactly where the launch returns it (out is zeroed):
 * rows of `given` by index off the persistent kernel, or a plan compiled with lti=[...] or with CSC results
 * that fits no kernel.  MPCASM_ERR_ARG: batch < 1, `path` out of range, a flag that is not 0 or 1. */
int mpcasm_assemble_route(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab, int batch,
                          int path, int inputs_aligned, int indexed, int32_t out[4]);

/* Diagnostic, needs no device: what the staged pipeline (MPCASM_KERNEL_STAGED: the route of MPCASM_OPT_PATH 2 and
 * of every plan no other kernel takes) launches for `batch` instances of the plan whose tables these are, with the
 * cost half (P, q), the constraint half (G, h) or both wanted (want_* = 0 / 1, not both 0).  The launch takes the
 * decision from the same function.  out[0]: the Hessian's kernel, MPCASM_STAGED_* (NONE: the cost is not wanted or
 * the plan has no unknown; BLOCK: a wavefront per 32 x 32 block of [P | q]; GEMM, from 128 unknowns on: a workgroup
 * per 128 x 128 block of P and the gradient by a kernel of its own); out[1]: MPCASM_STAGED_SYM (GEMM: only the
 * block pairs bi <= bj are computed, mirrored on store) | MPCASM_STAGED_WHOLE_LINES (rows of G leave as whole
 * cache lines: 16 | unknowns, constraints wanted) | the most axes of a limit << 8; out[2], out[3]: GEMM: the
 * blocks of 128 columns and the block pairs per instance; BLOCK: the block rows and block columns (q is the
 * column behind P); out[4] .. out[7]: workgroups of the composition of the workspace, the Hessian kernel, the
 * gradient kernel (GEMM only) and the constraint kernel (0: not launched).  Which branch of the constraint kernel
 * a row takes follows from the parity of the unknowns and that row's own axes (up to two: the unrolled pairs).
 * MPCASM_ERR_LIMIT exactly where the launch returns it, before anything is launched (out is zeroed): constraints
 * wanted and a limit of more than 8 axes.  MPCASM_ERR_ARG for a plan the pipeline cannot run (a dynamics
 * compiled as ltv, lti=[...], results in CSC form). */
enum { MPCASM_STAGED_NONE = 0, MPCASM_STAGED_BLOCK = 1, MPCASM_STAGED_GEMM = 2 };
enum { MPCASM_STAGED_SYM = 1, MPCASM_STAGED_WHOLE_LINES = 2 };
int mpcasm_staged_route(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab, int want_cost,
                        int want_constraints, int batch, int32_t out[8]);

/* f3  sparse hand-off -----------------------------------------------------------
 * Replaces the dense -> CSC conversion in front of the solver call of the walking loop
 *   Q = scipy.sparse.csc_matrix(Q); A = scipy.sparse.csc_matrix(A)
 *   python/use_examples/simple_functional_example/biped_mpc_loop.py:57-58
 * for a whole batch with ONE pattern: d_index[k] is the flat offset (row * cols + col)
 * of the k-th stored entry, in CSC order, of a structural sparsity pattern that the plan
 * compiler derives (mpcasm/plan.py: csc_pattern); entries of the pattern that happen to
 * be 0.0 in an instance are stored as explicit zeros, so the pattern -- indptr, indices,
 * shared by the batch, as OSQP's update_values wants it -- never changes.
 *   d_dst[b][k] = d_src[b * src_stride + d_index[k]]      k < nnz, b < batch
 */
int mpcasm_gather(const double* d_src, int64_t src_stride, const int32_t* d_index, int nnz,
                  double* d_dst, int batch, void* stream);

/* f4  batched box transforms ---------------------------------------------------
 * Replaces, for every instance of a batch at once, the per-tick geometry updates of a
 *   Box                                     python/mpc_interface/restrictions.py:380-486
 * on the facets' parameters inside d_params [batch][n_params] (the arrow, center and
 * extreme fields of the box's Constraints, restrictions.py:201-219 incl. normalize()):
 *   MPCASM_BOX_RECENTER   center  = arg[axes]                 recenter_in_TS   :380-388
 *   MPCASM_BOX_TRANSLATE  center += arg[axes]                 translate_in_TS  :411-415
 *   MPCASM_BOX_ROTATE     arrow_r = arrow_r . R^T, R = arg[axes][axes]   rotate_in_TS :436-455
 *   MPCASM_BOX_SCALE      extreme *= arg[0]  (new factor / old factor)   scale_box :474-478
 *   MPCASM_BOX_MARGIN     extreme -= arg[0] * ||arrow||_F     set_safety_margin :480-486
 * After ROTATE, SCALE and MARGIN rows whose extreme turned negative are flipped
 * (extreme, arrow -> -extreme, -arrow), as Constraint.normalize() does (:180-194).
 * d_facets: nfacets records of 7 int32 -- arrow offset, arrow rows, center offset, center
 * rows, extreme offset, extreme rows, axes -- offsets into one instance's parameters.
 * d_arg [batch][arg_stride] (arg_stride 0: one argument for all instances).
 */
enum { MPCASM_BOX_RECENTER = 0, MPCASM_BOX_TRANSLATE, MPCASM_BOX_ROTATE, MPCASM_BOX_SCALE,
       MPCASM_BOX_MARGIN };
int mpcasm_box_transform(double* d_params, int64_t n_params, int batch, const int32_t* d_facets,
                         int nfacets, int op, const double* d_arg, int64_t arg_stride,
                         void* stream);

/* f4, state space: replaces Box.recenter_in_SS / translate_in_SS            restrictions.py:390-404, 417-431
 * (through Constraint.SS_to_TS, :240-250) for the boxes whose facets carry an L -- those of
 * Box.state_space (:342-378: L = the facet's normal in the state space) and task-space boxes
 * built with L.  Per instance a state-space point p [ss_dim][axes] (one column per task-space
 * axis); facet f gets, per centre row r and axis a,
 *   MPCASM_BOX_RECENTER   center[r][a]  = sum_v L[f][a][r][v] p[v][a]
 *   MPCASM_BOX_TRANSLATE  center[r][a] += sum_v L[f][a][r][v] p[v][a]
 * d_L [nfacets][axes][lrows][ss_dim]: the facets' L matrices (the same for every instance:
 * they are part of the plan's structure); a facet's centre field must have lrows rows.
 * d_arg [batch][arg_stride] with arg_stride = ss_dim * axes (0: one point for all). */
int mpcasm_box_transform_ss(double* d_params, int64_t n_params, int batch,
                            const int32_t* d_facets, int nfacets, int op, const double* d_L,
                            int lrows, int ss_dim, const double* d_arg, int64_t arg_stride,
                            void* stream);

/* f3, the "or": the solve itself, batched ---------------------------------------------
 * Replaces, for every instance of a batch at once, the solver call of the walking loop
 *   self.optim = osqp_solve_qp(P=Q, q=q, G=A, h=h)
 *   python/use_examples/simple_functional_example/biped_mpc_loop.py:60
 * on the dense results of mpcasm_assemble where they lie:  min 1/2 x'Px + q'x  s.t.  Gx <= h  (no
 * equalities on this path, body.py:331).  `iters` iterations of OSQP's ADMM (Stellato et al., Math.
 * Prog. Comp. 12 (2020), Algorithm 1) with the steps rho, sigma, alpha (OSQP's defaults: 0.1, 1e-6,
 * 1.6) and without its problem scaling, adaptive rho and polishing:
 *   (P + sigma I + rho G'G) xt = sigma x - q + G'(rho z - y);  zt = G xt;  x+ = alpha xt + (1 - alpha) x
 *   z+ = min(alpha zt + (1 - alpha) z + y / rho, h);  y+ = y + rho (alpha zt + (1 - alpha) z - z+)
 * d_P [batch][no][no] (symmetric), d_q [batch][no], d_G [batch][nc][no], d_h [batch][nc].
 * d_x [batch][no], d_y [batch][nc], d_z [batch][nc]: the iterates -- read when warm != 0 (a walking
 * loop starts a tick from the last one's), else started from x = 0, y = 0, z = min(0, h); always
 * written.  d_res (may be NULL) [batch][2]: OSQP's residuals |Gx - z|_inf and |Px + q + G'y|_inf after
 * the last iteration -- the caller decides whether to iterate on.  An instance whose
 * P + sigma I + rho G'G is not positive definite gets NaNs.
 * d_kinv (may be NULL) [batch][no][no]: the inverse of P + sigma I + rho G'G.  kinv_valid == 0: written by this
 * call; != 0: READ instead of factoring -- for a caller whose P and G (and rho, sigma) did not change since the call
 * that wrote it: the same model and structure with a new `given` changes q and h only (body.py:236-302), and the
 * factorisation is the larger part of a call of a few dozen iterations.  MPCASM_ERR_LIMIT when one instance's
 * matrices do not fit on chip ((no + max(nc, no)) * (no | 1) + 8 no + 4 nc + 4 max(nc, no) doubles in 156 KB of LDS:
 * the biped up to N = 24 and beyond; not C3). */
int mpcasm_admm(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                const double* d_h, double* d_x, double* d_y, double* d_z, double* d_res, double rho,
                double sigma, double alpha, int iters, int warm, int batch, double* d_kinv, int kinv_valid,
                void* stream);

/* Per-instance outcome of mpcasm_qp_solve (OSQP's status values).  These are written to d_status on the
 * device; they are not return codes of a library function. */
enum {
  MPCASM_QP_SOLVED = 1,               /* both residuals within eps_abs + eps_rel * their scale       */
  MPCASM_QP_MAX_ITER = -2,            /* max_iter iterations without a verdict                        */
  MPCASM_QP_PRIMAL_INFEASIBLE = -3,   /* the step of y certifies that no x has Gx <= h                */
  MPCASM_QP_DUAL_INFEASIBLE = -4,     /* the step of x is a direction the cost falls along without end */
  MPCASM_QP_NON_CVX = -7              /* P + sigma I + rho G'G not positive definite, or rho <= 0       */
};

/* The solve to tolerance: mpcasm_admm's iteration (same operands, same iterates) with OSQP's stopping
 * rules and adaptive rho (Stellato et al. 2020, sections 3.4 and 5.2; no problem scaling, no polishing),
 * every instance on its own and nothing read back to the host -- a tick of the walking loop can be
 * captured in one graph.  After iteration k, when k % check_every == 0 or k == max_iter, with
 * infinity norms and dx = x_k - x_{k-1}, dy = max(y_k - y_{k-1}, 0):
 *   solved              |Gx - z| <= eps_abs + eps_rel max(|Gx|, |z|)  and
 *                       |Px + q + G'y| <= eps_abs + eps_rel max(|Px|, |G'y|, |q|)
 *   primal infeasible   |dy| > 1e-30, h'dy < -eps_prim_inf |dy|, |G'dy| < eps_prim_inf |dy|
 *   dual infeasible     |dx| > 1e-30, q'dx < -eps_dual_inf |dx|, |P dx| < eps_dual_inf |dx|,
 *                       max_i (G dx)_i < eps_dual_inf |dx|
 * tested in that order; the first that holds ends the instance (MPCASM_QP_*; d_iters[b] = k).  None within
 * max_iter: MPCASM_QP_MAX_ITER, d_iters[b] = max_iter.  All four eps may be 0 (no instance stops early).
 * adaptive_rho_interval > 0 (a multiple of check_every): at a check with k % adaptive_rho_interval == 0 that
 * decides nothing and is not the last iteration,
 *   rho' = rho sqrt((r_p / (max(|Gx|, |z|) + 1e-30)) / (r_d / (max(|Px|, |G'y|, |q|) + 1e-30)))
 * clipped to [1e-6, 1e6]; when rho' > 5 rho or rho' < rho / 5 the instance takes rho' (K formed, factored
 * and inverted again; x, y, z carry over).
 * d_rho [batch]: in, the step each instance starts with; out, the step it ended with.  A rho <= 0, or a
 * K that is not positive definite (at the start or after a change of rho): MPCASM_QP_NON_CVX, NaNs in
 * x, y, z, d_res and d_kinv.  d_status, d_iters [batch]; d_res (may be NULL) [batch][2]: |Gx - z| and
 * |Px + q + G'y| of the returned iterate.  The other operands are mpcasm_admm's, except that d_P is
 * read also with kinv_valid (the dual residual needs Px); with kinv_valid, d_kinv[b] must be the
 * inverse for d_rho[b] as passed in.  d_kinv (may be NULL) holds the inverse for the final rho on return:
 * the next tick on the same model passes d_kinv and d_rho back and factors nothing.
 * MPCASM_ERR_ARG: an eps not finite or < 0, max_iter < 0, check_every < 1, an adaptive_rho_interval < 0
 * or not a multiple of check_every, or what mpcasm_admm refuses; MPCASM_ERR_LIMIT as mpcasm_admm. */
int mpcasm_qp_solve(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                    const double* d_h, double* d_x, double* d_y, double* d_z, int warm, double* d_rho,
                    double sigma, double alpha, double eps_abs, double eps_rel, double eps_prim_inf,
                    double eps_dual_inf, int max_iter, int check_every, int adaptive_rho_interval,
                    int32_t* d_status, int32_t* d_iters, double* d_res, int batch, double* d_kinv,
                    int kinv_valid, void* stream);
/* Needs no device: the LDS bytes one instance of mpcasm_qp_solve (and of mpcasm_admm: the same layout)
 * takes for no unknowns and nc limits (*out; MPCASM_ERR_LIMIT too when that exceeds what a workgroup
 * may have). */
int mpcasm_qp_solve_lds_bytes(int no, int nc, int64_t* out);

/* The same solve for QPs whose matrices do not fit on chip (C3, C5, C4): replaces, like mpcasm_qp_solve,
 *   self.optim = osqp_solve_qp(P=Q, q=q, G=A, h=h)      biped_mpc_loop.py:60
 * with mpcasm_qp_solve's argument list, status codes, rules, iterates, warm start, d_rho, d_kinv /
 * kinv_valid reuse and per-instance outputs, nothing read back to the host.  G is read in place from d_G
 * once per iteration (not copied to LDS); K^-1 = (P + sigma I + rho G'G)^-1 lives in LDS when it fits
 * beside the vectors, else in d_kinv (see mpcasm_qp_solve_wide_info).  The one difference in the operands:
 * when K^-1 is not on chip for this (no, nc), d_kinv is REQUIRED (MPCASM_ERR_ARG if NULL) -- d_kinv[b] is then
 * the kernel's factorisation workspace, and on return holds the inverse for the final rho as mpcasm_qp_solve
 * promises.  The iterates equal mpcasm_qp_solve's up to rounding (sums in another order).
 * Size limit: no <= 512 and (3 nc + 23 no + 64) doubles (+ no (no | 1) with K^-1 on chip) within 156 KB of
 * LDS per instance -- every nc <= 2048 at no = 512, nc <= 2709 there; nc = 0 is allowed.  MPCASM_ERR_ARG as
 * mpcasm_qp_solve; MPCASM_ERR_LIMIT beyond the limit; nothing is launched on a refusal. */
int mpcasm_qp_solve_wide(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                         const double* d_h, double* d_x, double* d_y, double* d_z, int warm, double* d_rho,
                         double sigma, double alpha, double eps_abs, double eps_rel, double eps_prim_inf,
                         double eps_dual_inf, int max_iter, int check_every, int adaptive_rho_interval,
                         int32_t* d_status, int32_t* d_iters, double* d_res, int batch, double* d_kinv,
                         int kinv_valid, void* stream);
/* Needs no device: for one instance of mpcasm_qp_solve_wide with no unknowns and nc limits, the LDS bytes it
 * takes (*lds_bytes) and whether K^-1 lives in LDS (*kinv_on_chip = 1) or in d_kinv (0).  K^-1 is on chip when
 * no (no | 1) + 3 nc + 23 no + 64 doubles fit in 156 KB; the environment variable MPCASM_QP_WIDE_KINV, read at
 * every call, overrides that: "global" keeps K^-1 in d_kinv always, "lds" puts it on chip wherever it fits.
 * MPCASM_ERR_LIMIT beyond the size limit of mpcasm_qp_solve_wide (the other outputs still written). */
int mpcasm_qp_solve_wide_info(int no, int nc, int64_t* lds_bytes, int32_t* kinv_on_chip);

/* Soft limits, without slack unknowns: mpcasm_qp_solve and mpcasm_qp_solve_wide on
 *   min 1/2 x'Px + q'x + sum_i phi_i((Gx - h)_i)
 * where a hard row has phi_i = the indicator of t <= 0 and a soft row has phi_i(t) = 0 for t <= 0 and
 * lin_i t + 1/2 quad_i t^2 for t > 0.  This equals the slack QP  min ... + sum lin_i s_i + 1/2 quad_i s_i^2,
 * Gx - s <= h, s >= 0  in x and in the multipliers of the rows of G.  The argument lists are the hard entries'
 * plus d_soft_lin, d_soft_quad [batch][nc] at soft_stride doubles: soft_stride == nc means per instance, 0 means
 * one pair of rows for the whole batch, anything else is MPCASM_ERR_ARG; null vectors with nc > 0 are
 * MPCASM_ERR_ARG.  lin_i = +inf makes row i hard.  Everything else is the hard entry's: operands, outputs, warm
 * start, d_rho, d_kinv / kinv_valid (K, its factorisation and the inverse do not see the penalties: an inverse a
 * hard solve left serves a soft one and back), refusals.
 * The iteration is the hard one except the z update.  With v = alpha zt + (1 - alpha) z + y / rho:
 *   hard row, lin_i = +inf:  z+ = min(v, h) -- the hard entry's expression itself: with every lin = +inf every
 *                            output equals the hard entry's bit for bit;
 *   soft row:                z+ = v when v <= h, else z+ = h + max(0, (rho (v - h) - lin) / (rho + quad)).
 * y+ = y + rho (alpha zt + (1 - alpha) z - z+) is unchanged: it is a subgradient of phi at z+, so both residuals,
 * their scales, "solved" and the adaptive rho keep their meaning.
 * Primal infeasible: soft rows take no part -- their entry of the projected step dy is 0 in all three quantities
 * |dy|, h'dy, |G'dy|.  A certificate on the hard rows alone proves infeasibility whatever the soft rows do; with
 * every row soft the verdict cannot occur.  (While y climbs towards a large lin its step looks exactly like a
 * certificate: the masking is not optional.)
 * Dual infeasible: unchanged, over all rows.  It stays sound, because a direction along which no row rises is also
 * free of penalty; it no longer finds every unbounded instance (one whose cost falls along a direction that soft
 * rows rise along more slowly): an instance it misses ends as MPCASM_QP_MAX_ITER.
 * Bad penalties: an instance where any lin_i is NaN or < 0, or any quad_i is NaN, < 0 or +inf, is
 * MPCASM_QP_NON_CVX with NaN iterates, as for rho <= 0; decided on the device while the vectors are loaded, the
 * other instances of the launch are untouched.
 * mpcasm_qp_polish* must not follow on an instance with a violated soft row (its active-set model and its
 * z = min(Gx, h) are the hard problem's).  LDS: the hard entries' plus 2 nc doubles. */
int mpcasm_qp_solve_soft(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                         const double* d_h, double* d_x, double* d_y, double* d_z, int warm, double* d_rho,
                         double sigma, double alpha, double eps_abs, double eps_rel, double eps_prim_inf,
                         double eps_dual_inf, int max_iter, int check_every, int adaptive_rho_interval,
                         int32_t* d_status, int32_t* d_iters, double* d_res, int batch, double* d_kinv,
                         int kinv_valid, void* stream, const double* d_soft_lin, const double* d_soft_quad,
                         int64_t soft_stride);
/* Needs no device: mpcasm_qp_solve_lds_bytes for mpcasm_qp_solve_soft (MPCASM_ERR_LIMIT exactly where its launch
 * returns it). */
int mpcasm_qp_solve_soft_lds_bytes(int no, int nc, int64_t* out);
int mpcasm_qp_solve_wide_soft(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                              const double* d_h, double* d_x, double* d_y, double* d_z, int warm, double* d_rho,
                              double sigma, double alpha, double eps_abs, double eps_rel, double eps_prim_inf,
                              double eps_dual_inf, int max_iter, int check_every, int adaptive_rho_interval,
                              int32_t* d_status, int32_t* d_iters, double* d_res, int batch, double* d_kinv,
                              int kinv_valid, void* stream, const double* d_soft_lin, const double* d_soft_quad,
                              int64_t soft_stride);
/* Needs no device: mpcasm_qp_solve_wide_info for mpcasm_qp_solve_wide_soft (5 nc + 23 no + 64 doubles, + no (no | 1)
 * with K^-1 on chip, within the same 156 KB: near the edge K^-1 may be on chip for the hard entry and in d_kinv for
 * this one, and the size limit is tighter -- nc <= 1625 at no = 512, where the hard entry takes 2048). */
int mpcasm_qp_solve_wide_soft_info(int no, int nc, int64_t* lds_bytes, int32_t* kinv_on_chip);

/* Per-instance outcome of mpcasm_qp_polish, written to d_polish on the device. */
enum {
  MPCASM_POLISH_DONE = 1,      /* the polished point replaced the iterate                                  */
  MPCASM_POLISH_SKIPPED = 0,   /* not a solved instance, or more active rows than unknowns: nothing written */
  MPCASM_POLISH_REJECTED = -1  /* a pivot not positive, or the polished point is not the better one          */
};

/* Solution polishing, the step OSQP takes after its iteration has stopped -- what
 *   self.optim = osqp_solve_qp(P=Q, q=q, G=A, h=h)      biped_mpc_loop.py:60
 * does with polishing on (Stellato et al. 2020, section 4 "Solution polishing") -- for a batch of iterates of
 * mpcasm_qp_solve (which itself does not polish): the same operands in the same layouts, every instance on its
 * own, nothing read back, the call can be captured in a graph.  Per instance b, in order:
 *   skipped    d_status != NULL and d_status[b] != MPCASM_QP_SOLVED (the instance is not read: NON_CVX holds
 *              NaN), or the guessed active set has na > no rows: d_polish[b] = MPCASM_POLISH_SKIPPED and
 *              x, y, z, d_res[b] are not written
 *   active set row i iff h_i - z_i < y_i (OSQP's test with l = -inf, u = h); G_A, h_A the na active rows
 *   solve      K = [[P, G_A'], [G_A, 0]], g = [-q; h_A], dK = diag(delta I_no, -delta I_na):
 *              t = (K + dK)^-1 g, then refine_iters times t += (K + dK)^-1 (g - K t), the residual from K as it
 *              is, with P and G as given.  OSQP's defaults: delta = 1e-6, refine_iters = 3.  Block elimination
 *              with two Cholesky factorisations, P + delta I = L L' and G_A (P + delta I)^-1 G_A' + delta I; a
 *              pivot that is not positive: MPCASM_POLISH_REJECTED
 *   point      x^ = t[:no]; y^ = t[no:] on the active rows, 0 elsewhere; z^ = min(G x^, h)
 *   accept     with r_p = |Gx - z|, r_d = |Px + q + G'y| of the iterate passed in (computed here) and r^_p, r^_d
 *              of the polished point, infinity norms: OSQP's rule
 *                (r^_p < r_p and r^_d < r_d) or (r^_p < r_p and r_d < 1e-10) or (r^_d < r_d and r_p < 1e-10)
 *              AND every y^_i >= 0 -- a departure from OSQP, whose rule does not see a multiplier's sign
 *              (DESIGN.md).  Accepted: x, y, z <- x^, y^, z^, d_res[b] = (r^_p, r^_d), MPCASM_POLISH_DONE.
 *              Otherwise MPCASM_POLISH_REJECTED and x, y, z, d_res[b] keep their bits; a NaN anywhere fails
 *              every comparison.
 * d_status (may be NULL: every instance is polished) [batch] int32, mpcasm_qp_solve's; d_polish [batch] int32;
 * d_res (may be NULL) [batch][2].
 * Size limit: one instance takes 4 no (no | 1) + 13 no + 4 nc + 16 + ceil(no / 2) doubles of LDS (four
 * matrices -- P + delta I and its factor, the factor's inverse, G_A, the Schur complement -- the vectors and
 * the partial sums), rounded up to even; MPCASM_ERR_LIMIT, nothing launched, beyond 156 KB: the biped up to
 * N = 24 and (65, 70) fit, C3 does not.  MPCASM_ERR_ARG, before any device call: delta not finite or <= 0,
 * refine_iters < 0, batch < 0, no < 1, nc < 0, a null d_P, d_q, d_x, d_polish (with nc > 0: d_G, d_h, d_y,
 * d_z).  batch == 0: MPCASM_OK. */
int mpcasm_qp_polish(int no, int nc, const double* d_P, const double* d_q, const double* d_G, const double* d_h,
                     double* d_x, double* d_y, double* d_z, const int32_t* d_status, double delta,
                     int refine_iters, int32_t* d_polish, double* d_res, int batch, void* stream);
/* Needs no device: the LDS bytes one instance of mpcasm_qp_polish takes (*out; MPCASM_ERR_LIMIT too when that
 * exceeds what a workgroup may have). */
int mpcasm_qp_polish_lds_bytes(int no, int nc, int64_t* out);

/* The most workgroups one launch of mpcasm_qp_polish_wide has: two per CU of an MI355X. */
#define MPCASM_POLISH_WIDE_CAP 512

/* The same polishing for QPs whose matrices do not fit on chip (C3, C5, C4), the iterates of
 * mpcasm_qp_solve_wide: mpcasm_qp_polish's operands, steps, rule, sign test, verdicts and untouched outputs, per
 * instance exactly as stated above.  G and P are read in place; the matrices of the KKT solve live in d_work, a
 * device workspace of the caller's that is sized per WORKGROUP, not per instance: the launch has
 * min(batch, MPCASM_POLISH_WIDE_CAP) workgroups, workgroup w takes the instances w, w + workgroups, ... and reuses
 * its slice.  A slice is three no x no matrices -- (P + delta I)^-1, Y = G_A (P + delta I)^-1 and
 * (Y G_A' + delta I)^-1, each inverse formed in place from a Cholesky factorisation (a pivot that is not positive:
 * MPCASM_POLISH_REJECTED) -- and a solve of the KKT system is four matrix-vector products with them.  The points
 * equal mpcasm_qp_polish's up to rounding (another method for the same system), not bit for bit.
 * Workspace: workgroups * (3 no^2, rounded up to even) doubles; d_work 16-byte aligned, its contents neither
 * read from an earlier call nor meaningful after this one.  Two calls that may run at once need a workspace each.
 * LDS: one workgroup takes 14 no + 4 nc + 16 + ceil(no / 2) doubles, rounded up to even (the vectors, the partial
 * sums, the active rows).
 * Size limit: no <= 512 and that LDS within 156 KB -- every nc <= 2048 at every such no (nc <= 3132 at no = 512),
 * what mpcasm_qp_solve_wide takes; nc = 0 is allowed.  MPCASM_ERR_LIMIT beyond it, nothing launched.
 * MPCASM_ERR_ARG, before any device call: mpcasm_qp_polish's cases, a null d_work, a d_work that is not 16-byte
 * aligned, work_bytes smaller than mpcasm_qp_polish_wide_info reports for (no, nc, batch).  batch == 0: MPCASM_OK. */
int mpcasm_qp_polish_wide(int no, int nc, const double* d_P, const double* d_q, const double* d_G, const double* d_h,
                          double* d_x, double* d_y, double* d_z, const int32_t* d_status, double delta,
                          int refine_iters, int32_t* d_polish, double* d_res, int batch, void* d_work,
                          size_t work_bytes, void* stream);
/* Needs no device: for mpcasm_qp_polish_wide on batch instances with no unknowns and nc limits, the LDS bytes of a
 * workgroup (*lds_bytes), the bytes of workspace the call needs (*work_bytes) and the workgroups it launches
 * (*workgroups = min(batch, MPCASM_POLISH_WIDE_CAP)), by the formulas above.  The environment variable
 * MPCASM_QP_POLISH_WIDE_GROUPS, read at every call of either entry, lowers the cap to its value (1 ... the cap: a
 * tuning aid, tools/bench_qp_polish_wide.py).  MPCASM_ERR_LIMIT beyond the size limit (the outputs still written);
 * MPCASM_ERR_ARG for no < 1, nc < 0, batch < 0 or a null output. */
int mpcasm_qp_polish_wide_info(int no, int nc, int batch, int64_t* lds_bytes, int64_t* work_bytes,
                               int32_t* workgroups);

/* Per-instance outcome of mpcasm_qp_sens, written to d_verdict on the device. */
enum {
  MPCASM_SENS_DONE = 1,      /* u, w (and lres, gP, gG where asked for) were written                       */
  MPCASM_SENS_SKIPPED = 0,   /* not a solved instance, or more active rows than unknowns: nothing written */
  MPCASM_SENS_SINGULAR = -1  /* a pivot of the regularised KKT system is not positive: nothing written     */
};

/* The sensitivity of solved QPs -- how x* and y* move when q, h, P, G move -- for a batch of iterates of
 * mpcasm_qp_solve, best polished ones: at a strictly complementary solution with active rows A the KKT
 * conditions are  P x + q + G_A'y_A = 0,  G_A x = h_A,  so the forward and the adjoint derivative are both one
 * solve with the polish's symmetric  K = [[P, G_A'], [G_A, 0]]  and a right-hand side [rx; ry] of the caller's.
 * With [u; w_A] = K^-1 [rx; ry_A] and w = 0 off the active set:
 *   adjoint (rx = dL/dx, ry = dL/dy)    dL/dq = -u,  dL/dh = w,  dL/dP = -1/2 (u x' + x u')  (P symmetric),
 *                                       row i of dL/dG = -(y_i u' + w_i x') on active rows, 0 elsewhere
 *   forward (rx = -(dq + dP x + dG_A'y_A), ry = dh - dG x)      dx = u,  dy = w
 * Same layouts as mpcasm_qp_polish, every instance on its own, nothing read back, the call can be captured in a
 * graph; P, G, h, x, y, z are only read.  Per instance b, in order:
 *   skipped    d_status != NULL and d_status[b] != MPCASM_QP_SOLVED (the instance is not read: NON_CVX holds
 *              NaN), or the guessed active set has na > no rows: d_verdict[b] = MPCASM_SENS_SKIPPED and no other
 *              output is written
 *   active set row i iff h_i - z_i < y_i, the polish's test
 *   solve      r = [rx; ry on the active rows], dK = diag(delta I_no, -delta I_na);  t = (K + dK)^-1 r, then
 *              refine_iters times  t += (K + dK)^-1 (r - K t), the residual from K as it is, with P and G as
 *              given.  The polish's factorisations and defaults (delta = 1e-6, refine_iters = 3); a pivot that is
 *              not positive: MPCASM_SENS_SINGULAR and no other output is written
 *   results    d_u[b] = t[:no]; d_w[b] = t[no:] on the active rows and exactly 0 on every other row (all nc
 *              entries are written); d_lres[b] = |r - K t|_inf after the last refinement -- at a weakly active row
 *              or with dependent active rows K is singular, w depends on delta, and this residual is the sign to
 *              read; d_verdict[b] = MPCASM_SENS_DONE
 *   gradients  where d_gP / d_gG are not NULL they are written whole:  d_gP[b] = -1/2 (u x' + x u'),  row i of
 *              d_gG[b] = -(y_i u' + w_i x') on active rows and exact zeros elsewhere; x, y the iterate's as passed
 * d_rx, d_u [batch][no]; d_ry, d_w [batch][nc]; d_gP [batch][no][no]; d_gG [batch][nc][no]; d_verdict [batch] int32;
 * d_lres [batch]; d_status (may be NULL: every instance is taken) as for mpcasm_qp_polish.  d_gP, d_gG, d_lres may
 * be NULL.  No output may overlap an input.
 * Size limit: mpcasm_qp_polish's, and its LDS (the same layout: rx, t and the iterate where the polish keeps q, its
 * residuals and the polished point).  MPCASM_ERR_LIMIT beyond it, nothing launched.  MPCASM_ERR_ARG, before any
 * device call: delta not finite or <= 0, refine_iters < 0, batch < 0, no < 1, nc < 0, a null d_P, d_x, d_rx, d_u,
 * d_verdict (with nc > 0: d_G, d_h, d_y, d_z, d_ry, d_w).  batch == 0: MPCASM_OK. */
int mpcasm_qp_sens(int no, int nc, const double* d_P, const double* d_G, const double* d_h, const double* d_x,
                   const double* d_y, const double* d_z, const int32_t* d_status, const double* d_rx,
                   const double* d_ry, double delta, int refine_iters, double* d_u, double* d_w, double* d_gP,
                   double* d_gG, int32_t* d_verdict, double* d_lres, int batch, void* stream);
/* Needs no device: the LDS bytes one instance of mpcasm_qp_sens takes, mpcasm_qp_polish_lds_bytes' figure and
 * verdict. */
int mpcasm_qp_sens_lds_bytes(int no, int nc, int64_t* out);

/* The same sensitivity for QPs whose matrices do not fit on chip, the iterates of mpcasm_qp_solve_wide:
 * mpcasm_qp_sens's operands, steps, verdicts and untouched outputs with mpcasm_qp_polish_wide's method, launch
 * (min(batch, MPCASM_POLISH_WIDE_CAP) workgroups striding the batch), workspace (workgroups * (3 no^2, rounded up
 * to even) doubles, d_work 16-byte aligned, nothing kept between calls), LDS and size limit.  u and w equal
 * mpcasm_qp_sens's up to rounding, not bit for bit.  MPCASM_ERR_ARG, before any device call: mpcasm_qp_sens's
 * cases, a null d_work, a d_work that is not 16-byte aligned, work_bytes smaller than mpcasm_qp_sens_wide_info
 * reports for (no, nc, batch).  batch == 0: MPCASM_OK. */
int mpcasm_qp_sens_wide(int no, int nc, const double* d_P, const double* d_G, const double* d_h, const double* d_x,
                        const double* d_y, const double* d_z, const int32_t* d_status, const double* d_rx,
                        const double* d_ry, double delta, int refine_iters, double* d_u, double* d_w, double* d_gP,
                        double* d_gG, int32_t* d_verdict, double* d_lres, int batch, void* d_work, size_t work_bytes,
                        void* stream);
/* Needs no device: mpcasm_qp_polish_wide_info's three figures and verdict, for mpcasm_qp_sens_wide (the environment
 * variable MPCASM_QP_POLISH_WIDE_GROUPS lowers the cap of both). */
int mpcasm_qp_sens_wide_info(int no, int nc, int batch, int64_t* lds_bytes, int64_t* work_bytes,
                             int32_t* workgroups);

/* The derivative of the assembly with respect to `given`, matrix-free -------------------------------------------
 * P and G of mpcasm_assemble do not depend on `given`; q and h are affine in it.  With cMg, cMo the rows of a
 * definition after schedule and L over the columns of `given` and of the unknowns:
 *   generate_qp_cost        body.py:266-302   q = sum over the cost terms  s w cMo_a' (cMg_b given - aim)
 *   generate_qp_constraint  body.py:236-264   h = extreme + arrow . center - sum over the axes arrow_i (cMg_i given)
 * so  dq = J_q d,  J_q = sum s w cMo_a' cMg_b  (s = 1/2 on the two terms of a crossed cost; a cost on a free
 * variable itself contributes nothing), and -- the sign convention --  dh = -cMg d:  J_h = -sum_i diag(arrow_i)
 * cMg_i.  These entries apply J = [J_q ; J_h] (mpcasm_assemble_jvp: the tangential predictor's dq, dh for a change
 * d of `given`) and J' (mpcasm_assemble_vjp: dL/dgiven from dL/dq, dL/dh) without a preview matrix or a Jacobian
 * in memory: one workgroup-resident pass per instance over the plan's own tables (csrc/adjoint.hip), deterministic
 * -- no floating-point atomics; an instance's result does not depend on the batch or on its place in it.
 * plan, h_src, h_src_stride, d_params [batch][n_params], d_work as for mpcasm_preview_direct / mpcasm_assemble (a
 * plan compiled with lti=[...] takes the groups' (A, B) and needs d_work for the horizon tables it generates first).
 *   mpcasm_assemble_jvp   d_dgiven [batch][ng] -> d_dq [batch][no], d_dh [batch][nc]; a NULL output is skipped
 *   mpcasm_assemble_vjp   d_gq [batch][no], d_gh [batch][nc] -> d_ggiven [batch][ng] = J_q' gq + J_h' gh; a NULL
 *                         cotangent is zero: d_ggiven is then the other half's alone
 * MPCASM_ERR_ARG: both halves NULL, a null d_dgiven / d_ggiven, sources, d_params or d_work where the plan needs
 * them, another device than the plan's.  MPCASM_ERR_LIMIT: a plan compiled with ltv=[...] (no S, U: its adjoint is
 * the sweep's backward recursion), or one instance beyond the LDS of a CU.  ng == 0 or batch == 0: MPCASM_OK,
 * nothing written.  The parameters are not differentiated.  The first of these calls on a plan derives the
 * transposed index from the plan's tables and uploads it (a device allocation and a blocking copy, under a mutex in
 * the handle; freed by mpcasm_plan_destroy): make it before capturing a graph.  Later calls only launch. */
int mpcasm_assemble_jvp(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                        const double* d_params, const double* d_dgiven, double* d_dq, double* d_dh, void* d_work,
                        int batch, void* stream);
int mpcasm_assemble_vjp(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                        const double* d_params, const double* d_gq, const double* d_gh, double* d_ggiven,
                        void* d_work, int batch, void* stream);
/* Needs no device: what the two entries above launch for these tables -- validated as mpcasm_plan_create does --
 * when the sources have the strides h_src_stride (may be NULL when the plan has no source).  out[0]: dynamic LDS
 * bytes of a workgroup; out[1]: 1 when that is more than 64 KB (the whole-LDS attribute is set before the launch);
 * out[2]: words of the transposed index derived from the tables and kept with the plan handle; out[3]: workgroups
 * resident per CU (the launch's grid is min(batch, CUs * out[3])).  MPCASM_ERR_LIMIT exactly where the launches
 * return it (out is zeroed): both take the decision from the same function. */
int mpcasm_assemble_adjoint_info(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                                 const int64_t* h_src_stride, int32_t out[4]);

/* The derivative of the assembly with respect to the parameters, matrix-free -----------------------------------
 * dL/dparams [batch][n_params] for the cotangent of (P, q, G, h) that mpcasm_qp_sens stands for,
 *   gP = -1/2 (u x' + x u')     gq = -u     gG_R = -(y_R u' + w_R x')     gh = w
 * from d_x, d_u [batch][no] and d_y, d_w [batch][nc] (y with zeros off the active set; mpcasm_qp_sens writes w so),
 * without the dense gP, gG, a preview matrix or a row of the workspace in memory.  With V = [V_g | V_o] the
 * workspace rows (csrc/plan_tables.h), s = 1/2 under GT_FLAG_HALF, t = params[b] and the three row vectors
 * r_x = V_o x, r_u = V_o u, r_g = V_g given, the result is the sum of
 *   gterm (a, b, n, wp, dd, ap), not diagonal:  P += w V_o[a]' V_o[b] (GT_FLAG_P),  q += s w V_o[a]' (V_g[dd] given - aim)
 *     g[wp] += [GT_FLAG_P] (-1/2) sum_k (r_u[a+k] r_x[b+k] + r_x[a+k] r_u[b+k])  -  s sum_k r_u[a+k] (r_g[dd+k] - t[ap])
 *     g[ap] += s t[wp] sum_k r_u[a+k]
 *   GT_FLAG_DIAG gterm, column c = GT_AOFF + k, coefficient coef_k:  P[c][c] += w coef^2,  q[c] += -w coef aim
 *     g[wp] += sum_k coef_k (-coef_k u_c x_c + t[ap] u_c)          g[ap] += t[wp] sum_k coef_k u_c
 *   limit, line R = LM_OUT0 + l, axis i, row = LX_ROWOFF + (LX_ROWS == 1 ? 0 : l):
 *   G_R = sum_i arrow_Ri V_o[row],  h_R = extreme_R + sum_i arrow_Ri center_Ri - sum_i arrow_Ri r_g[row]
 *     g[arrow_Ri]  += -(y_R r_u[row] + w_R r_x[row]) + w_R (t[center_Ri] - r_g[row])
 *     g[center_Ri] += w_R t[arrow_Ri]                               g[extreme_R] += w_R
 * (a field of one row is broadcast over the lines: its gradient sums over them).  Every slot is written; one that
 * no record names is exactly 0.0.  One workgroup-resident pass per instance (csrc/adjoint.hip): every slot is
 * gathered by the lanes that own it through a parameter index derived from the plan's tables by the first call (a
 * device allocation and a blocking copy, under the handle's mutex, freed by mpcasm_plan_destroy: make that call
 * before capturing a graph) -- no floating-point atomics, two calls give identical bits, an instance's row does not
 * depend on the batch or on its place in it.
 * plan, h_src, h_src_stride, d_params, d_work as for mpcasm_assemble_vjp.  d_given [batch][ng], NULL when ng == 0.
 * d_verdict [batch] may be NULL; otherwise an instance whose verdict is not MPCASM_SENS_DONE gets an exactly zero
 * row and none of its vectors is read.  MPCASM_ERR_ARG: a null operand the plan needs, another device than the
 * plan's.  MPCASM_ERR_LIMIT: a plan compiled with ltv=[...], or one instance beyond the LDS of a CU.  batch == 0 or
 * n_params == 0: MPCASM_OK, nothing written. */
int mpcasm_assemble_params_vjp(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                               const double* d_params, const double* d_given, const double* d_x, const double* d_u,
                               const double* d_y, const double* d_w, const int32_t* d_verdict, double* d_gparams,
                               void* d_work, int batch, void* stream);
/* Needs no device: what mpcasm_assemble_params_vjp launches for these tables; the four words mean what
 * mpcasm_assemble_adjoint_info's do (out[2]: words of the parameter index).  MPCASM_ERR_LIMIT exactly where the
 * launch returns it (out is zeroed): both take the decision from the same function. */
int mpcasm_assemble_params_vjp_info(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                                    const int64_t* h_src_stride, int32_t out[4]);

/* The loop's warm start  last tick's solution, moved one sample along, as this tick's start ----------------
 * A receding-horizon loop solves, every tick, nearly the QP of the tick before with the horizon moved on by one
 * sample; mpcasm_qp_solve and mpcasm_qp_solve_wide take `warm`, d_rho in/out and the iterates.  These two entries
 * are the piece in between, for a loop whose structure (no, nc) changes from tick to tick and whose instances sit
 * at other positions of other launches every tick.  Nothing is read back; both can be captured in a graph.
 *
 * The *warm store* is the caller's: one record per row (per walker, in walker order), as four device arrays
 *   d_store_x    [store_rows][store_no] doubles   x, padded with zeros to store_no
 *   d_store_y    [store_rows][store_nc] doubles   y, padded with zeros to store_nc
 *   d_store_rho  [store_rows] doubles             the step the solve ended with
 *   d_store_meta [store_rows][2] int32            the solve's status (MPCASM_QP_*), and a tag of the caller's choice
 * 8-byte aligned; 1 <= store_no <= 512, 0 <= store_nc <= 2048 (d_store_y may be NULL when store_nc == 0).
 *
 * mpcasm_qp_warm_store, after a solve: instance b of a launch (no <= store_no, nc <= store_nc; d_x [count][no],
 * d_y [count][nc], d_rho [count], d_status [count]) is written into row d_index[b] of the store with `tag`, the
 * padding zeroed.  x, y and rho are stored bit for bit, and every instance is stored whatever its status: a stale
 * record never survives a tick (mpcasm_qp_warm_start judges the status).  d_index (count entries; NULL: instance
 * b is row b, store_rows >= count) follows the contract of mpcasm_next_given: DISTINCT entries in [0, store_rows),
 * vouched for by the host that builds them; an entry outside that range is skipped.  nc == 0: d_y may be NULL.
 *
 * mpcasm_qp_warm_start, before a solve: writes the iterates d_x [count][no], d_y, d_z [count][nc] and the step
 * d_rho [count] the solve starts from (pass them to mpcasm_qp_solve with warm = 1), and d_warm [count] int32: 1
 * where the instance starts warm, 0 where cold.  It reads this tick's assembled d_G [count][nc][no] and d_h
 * [count][nc] where they lie, the store, d_index (as above; an entry outside [0, store_rows) makes the instance
 * cold) and two int32 device tables: d_col_src [no], entries in [-1, store_no), and d_row_src [nc], entries in
 * [-1, store_nc) -- where unknown i and row j of this QP were in the record, -1: nowhere.  An entry outside its
 * range counts as -1; nothing is read out of range whatever the tables and the index hold.
 * Instance b with the record r = d_index[b] is WARM when all of these hold:
 *   the record's tag equals expect_tag;  bit MPCASM_QP_BIT(status) of warm_mask is set;
 *   its rho is finite and inside [1e-6, 1e6] (the range of the solve's adaptive rho);
 *   every value it gathers is finite (a NaN in a column no table entry names does not matter).
 * Then  x0[i] = d_col_src[i] >= 0 ? X[r][d_col_src[i]] : 0  and y0 likewise through d_row_src (copies, bit for
 * bit),  z0 = min(G_b x0, h_b)  and  rho0 = rho[r].  Otherwise COLD:  x0 = 0, y0 = 0, z0 = min(0, h_b),
 * rho0 = rho_cold -- exactly what mpcasm_qp_solve(warm = 0) starts from, so one launch with warm = 1 serves warm
 * and cold instances alike.  nc == 0 is allowed: d_G, d_h, d_y, d_z, d_row_src may then be NULL.
 * G is read once, in place (16-byte loads where no is even and d_G is 16-byte aligned, else 8-byte loads).
 *
 * Both: sizes up to mpcasm_qp_solve_wide's, no <= 512 and nc <= 2048.  MPCASM_ERR_ARG, before any device call:
 * no < 1, nc < 0, count < 0, store_rows < 0, store_no < 1, store_nc < 0, a size beyond those limits, a null
 * operand that is not excused above, a rho_cold that is not finite; for the store also no > store_no,
 * nc > store_nc, and a NULL d_index with store_rows < count.  count == 0: MPCASM_OK, no device needed. */
int mpcasm_qp_warm_store(int no, int nc, const double* d_x, const double* d_y, const double* d_rho,
                         const int32_t* d_status, int tag, double* d_store_x, double* d_store_y, double* d_store_rho,
                         int32_t* d_store_meta, int64_t store_rows, int store_no, int store_nc, const int32_t* d_index,
                         int count, void* stream);
int mpcasm_qp_warm_start(int no, int nc, const double* d_G, const double* d_h, const double* d_store_x,
                         const double* d_store_y, const double* d_store_rho, const int32_t* d_store_meta,
                         int64_t store_rows, int store_no, int store_nc, const int32_t* d_index,
                         const int32_t* d_col_src, const int32_t* d_row_src, int expect_tag, uint32_t warm_mask,
                         double rho_cold, double* d_x, double* d_y, double* d_z, double* d_rho, int32_t* d_warm,
                         int count, void* stream);

/* f2 + the loop  the next tick's `given` from a solution ------------------------------------------------
 * Replaces, for a batch of walkers, the end of every tick of the walking loop
 *   preview_all + update_given_collector       biped_mpc_loop.py:62-65, 81-92
 *   (Formulation.preview, body.py:209-219, of the rows the update reads, and arrange_given of the
 *    next decide_actions, biped_mpc_loop.py:54)
 * without the rows of the definitions ever leaving the chip and without a trip to the host.
 *
 * A *given map* says, per column c of `given`, what the column becomes:
 *   h_rows[c] = r >= 0               row r of the plan's preview program (the rows mpcasm_preview_direct
 *                                    writes: definition v at mpcasm/plan.py's pm_rows[v])
 *   h_rows[c] = MPCASM_GIVEN_CONST   the constant h_values[c] (finite)
 *   h_rows[c] = MPCASM_GIVEN_KEEP    left as it is
 * mpcasm_given_map_compile turns that into the map's words for this plan (host only, no device call):
 * the records plus the list of the base rows the named rows combine, worked out once.  *words = the
 * number of int32 words; h_map == NULL asks for that number only, a smaller capacity is MPCASM_ERR_ARG.
 * The caller copies the words to the device (d_map) and keeps them for as many ticks as it likes.
 * MPCASM_ERR_ARG: ng is not the plan's, a row outside the preview program, a CONST without a finite
 * value; MPCASM_ERR_LIMIT: a plan mpcasm_preview_direct refuses (compiled with ltv=[...], or whose
 * column tables do not cover it). */
enum { MPCASM_GIVEN_KEEP = -1, MPCASM_GIVEN_CONST = -2 };
int mpcasm_given_map_compile(const mpcasm_plan* plan, const int32_t* h_rows, const double* h_values, int ng,
                             int32_t* h_map, int64_t capacity, int64_t* words);

/* For count instances b: the new values of the map's columns from row d_index[b] of d_given (rows x ng) and
 * row b of d_optim (count x no), written IN PLACE into row d_index[b] of d_given -- the whole row is read
 * before any of it is written.  Only the base rows the named rows combine are evaluated, on chip, in the
 * order mpcasm_preview_direct evaluates them.  Sources, strides and d_work as for mpcasm_preview_direct
 * (instance b reads row b of a per-instance source).
 * d_index (count entries; NULL: instance b is row b, rows >= count): the entries of one call must be
 * DISTINCT and lie in [0, rows).  The host that builds the index checks that (the kernel skips an entry
 * outside [0, rows) but cannot see two instances writing one row).
 * d_status (count entries, e.g. mpcasm_qp_solve's; NULL: all apply) and apply_mask: instance b writes only
 * when bit MPCASM_QP_BIT(d_status[b]) of apply_mask is set; otherwise its row stays exactly as it was.
 * d_map / map_words: the words of mpcasm_given_map_compile for THIS plan; a map that does not match the
 * plan's sizes, or is not such a map, writes nothing.  MPCASM_ERR_LIMIT as mpcasm_given_map_compile. */
#define MPCASM_QP_BIT(status) (1u << ((status) < 0 ? -(status) : (status)))
int mpcasm_next_given(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                      double* d_given, int64_t rows, const double* d_optim, const int32_t* d_index,
                      const int32_t* d_status, uint32_t apply_mask, const int32_t* d_map, int64_t map_words,
                      void* d_work, int count, void* stream);

/* The loop's commands  per-walker commands into the parameter rows of a launch ------------------------------
 * Replaces, for a batch of walkers, the start of every tick of the walking loop
 *   Formulation.update(**kargs)                       body.py:142-147   (the user's callbacks)
 *   tools.update_stepping_area / find_step_centers    tools.py:149-165
 *   Cost.update(aim=, weight=)                        goal.py:106
 *   Constraint.update(center=, extreme=)              restrictions.py:201
 * where what changes is a number the user commands per walker (a target velocity, where to step): a *parameter
 * map* from a command vector per walker to elements of the parameter rows mpcasm_assemble reads, applied on the
 * device every tick, with nothing read back; it can be captured in the tick's graph, and a replay follows later
 * edits of the commands (their address is what the graph holds).
 *
 * d_params [>= batch][n_params] doubles: the parameter rows of the launch, instance b in row b.
 * d_cmd: the command table, row w at d_cmd + w cmd_stride, ncmd doubles each (cmd_stride == 0: one row shared by
 * the launch).  Instance b reads row w = d_index ? d_index[b] : b -- d_index (batch int32) follows the contract of
 * mpcasm_assemble_indexed: entries inside the command table, vouched for by the host that builds them, NOT checked
 * by the kernel.  d_sign (batch doubles, by position in the launch; may be NULL): a factor per instance, e.g. the
 * side (-1)^(step_count + 1) of tools.find_step_centers.
 * Record r is four int32 in d_recs, (dst, col, flags, 0), and two doubles in d_coef, (c0, c1).  It writes ONE
 * element of every instance's row:
 *   t = (flags & MPCASM_PMAP_SIGNED) ? c1 * d_sign[b] : c1
 *   v = t * d_cmd[w cmd_stride + col]
 *   d_params[b n_params + dst] = (flags & MPCASM_PMAP_CONST) ? c0 + v : v
 * every operation rounded on its own (no fused multiply-add): a restatement on the host gives the same bits, and
 * with c1 and the sign in {+1, -1} the element is the host's side * alternation * length exactly.
 * Nothing else is written: elements no record names, and rows >= batch, keep their bits.  A record with dst
 * outside [0, n_params), col outside [0, ncmd) or a flag bit other than the two writes nothing, and so does a
 * SIGNED record of a launch without d_sign (the given map's rule: a wrong table writes nothing it should not).
 * The records of one map must name DISTINCT dst -- the caller's contract (mpcasm/engine.py param_map_records
 * enforces it); two records on one element leave either value.
 * MPCASM_ERR_ARG, before any device call: a null d_params; with nrecs > 0 a null d_recs, d_coef or d_cmd;
 * n_params < 1, nrecs < 0, ncmd < 1, batch < 0, cmd_stride < 0 or 0 < cmd_stride < ncmd.
 * batch == 0 or nrecs == 0: MPCASM_OK, nothing launched, no device needed. */
enum { MPCASM_PMAP_SIGNED = 1, MPCASM_PMAP_CONST = 2 };
int mpcasm_params_map(double* d_params, int64_t n_params, const int32_t* d_recs, const double* d_coef, int nrecs,
                      const double* d_cmd, int64_t cmd_stride, int ncmd, const int32_t* d_index,
                      const double* d_sign, int batch, void* stream);

/* f2 + the loop, per-step dynamics  the preview rows and the next `given` of a plan compiled with ltv=[...] ----
 * Replaces, for a batch whose dynamics differ from step to step and from instance to instance
 * (x_{k+1} = A_k x_k + B_k u_k: the plans the sweep kernel assembles),
 *   Formulation.preview                         python/mpc_interface/body.py:209-219
 *   preview_all + update_given_collector        biped_mpc_loop.py:62-95
 * mpcasm_preview_direct, mpcasm_given_map_compile and mpcasm_next_given keep answering MPCASM_ERR_LIMIT for
 * such a plan: they read horizon matrices, and it has none.  Nor does it need any: every unknown is an input of
 * its one system, every given value an initial state, so the rows of a definition are the given values or the
 * unknowns themselves, or c . x_{k+1} along the forward recursion, and the next given is x_1 of every axis --
 * O(N n (n + m)) per axis, (A_k, B_k) read once from the plan's two ltv source slots (A (N, n, n), B (N, n, m)
 * per instance; stride 0: shared), the rows written once, no workspace.
 *
 * The *row table* says what every row of the preview program is (the rows mpcasm_preview_direct would write:
 * definition v at mpcasm/plan.py's pm_rows[v]).  h_recs: nrec records of MPCASM_ROLL_REC_WORDS int32, in the
 * order of the rows, each a run of rows
 *   kind, first row, rows, axis, k0, kstep, index of c in h_cvec, 0
 *   MPCASM_ROLL_GIVEN   row i of the run = given[k0 + i kstep]                      (bit for bit)
 *   MPCASM_ROLL_OPTIM   row i of the run = optim[k0 + i kstep]                      (bit for bit)
 *   MPCASM_ROLL_STATE   row i of the run = c . x_{k0 + i kstep + 1} of the axis     (c: SW_NMAX = 4 doubles, 0 beyond n)
 * mpcasm/plan.py rollout_rows derives them from the plan.  h_sizes: what the records were made for --
 * states, inputs, steps, axes, rows of the preview program, ng, no.  Host only, no device call, no plan handle:
 * the tables are validated as mpcasm_plan_create does.  *words = the number of int32 words; h_table == NULL asks
 * for that number only, a smaller capacity is MPCASM_ERR_ARG.  The caller copies the words to the device.
 * MPCASM_ERR_ARG: tables of a plan without a dynamics compiled as ltv, h_sizes that are not the plan's, records
 * that do not cover every row exactly once in order, an index outside the plan's sizes, a c that is not finite;
 * MPCASM_ERR_LIMIT: more than 4096 words of records and combinations. */
enum { MPCASM_ROLL_GIVEN = 0, MPCASM_ROLL_OPTIM = 1, MPCASM_ROLL_STATE = 2 };
#define MPCASM_ROLL_REC_WORDS 8
int mpcasm_ltv_rollout_compile(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                               const int32_t h_sizes[7], const int32_t* h_recs, int nrec, const double* h_cvec,
                               int ncvec, int32_t* h_table, int64_t capacity, int64_t* words);

/* The rows (Formulation.preview, body.py:209-219, of every definition): for count instances b, from row
 * d_index[b] of d_given (rows x ng; NULL: row b, rows >= count) and row b of d_optim (count x no), row b of d_out
 * (count x preview rows, 8-byte aligned).  d_table / table_words: the words of mpcasm_ltv_rollout_compile for
 * THIS plan; a table whose header does not match the plan's sizes, or that is no such table, writes nothing.
 * h_src / h_src_stride as for mpcasm_assemble.  MPCASM_ERR_ARG for a plan without a dynamics compiled as ltv
 * (mpcasm_preview_direct is for those); MPCASM_ERR_LIMIT when one instance does not fit in a CU's LDS. */
int mpcasm_ltv_rollout(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                       const double* d_given, int64_t rows, const double* d_optim, const int32_t* d_index,
                       const int32_t* d_table, int64_t table_words, double* d_out, int count, void* stream);

/* The next tick's given (update_given_collector, biped_mpc_loop.py:62-95): x_1 = A_0 x_0 + B_0 u_0 of every
 * axis, written IN PLACE into row d_index[b] of d_given -- the row is read before any of it is written; only
 * A_0, B_0 and the first sample of every input are read.  d_index, d_status, apply_mask: exactly as for
 * mpcasm_next_given (distinct entries in [0, rows), checked by the host that builds them; an instance writes only
 * when bit MPCASM_QP_BIT(d_status[b]) of apply_mask is set, else its row stays as it was; NULL status: all
 * apply).  d_table and the return codes as for mpcasm_ltv_rollout. */
int mpcasm_ltv_advance(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                       double* d_given, int64_t rows, const double* d_optim, const int32_t* d_index,
                       const int32_t* d_status, uint32_t apply_mask, const int32_t* d_table, int64_t table_words,
                       int count, void* stream);

/* Needs no device: the geometry of the launch mpcasm_ltv_rollout (rows_out = 1) or mpcasm_ltv_advance
 * (rows_out = 0) makes for count instances of the plan with these tables (validated as mpcasm_plan_create does)
 * and a row table of table_words words -- the one function the launch itself takes it from.  A workgroup takes
 * *group consecutive instances: as many as fit in 52 KB of LDS beside the table, at most 8, at most count, at
 * least 1; *lds_bytes its dynamic LDS (the shared part + *group times what an instance stages); *workgroups =
 * ceil(count / *group).  The plan's tables and not a plan handle, as mpcasm_ltv_rollout_compile: a handle needs a
 * device.  The launch's own answers: MPCASM_ERR_ARG for a plan without a dynamics compiled as ltv, a
 * table_words that is no row table's, a negative count, rows_out not 0 or 1, a null output; MPCASM_ERR_LIMIT when
 * one instance does not fit in a CU's LDS.  count == 0: MPCASM_OK, all three 0. */
int mpcasm_ltv_rollout_info(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                            int64_t table_words, int rows_out, int count, int32_t* group, int64_t* lds_bytes,
                            int32_t* workgroups);

/* Pre-stabilised (closed-loop) prediction for a dynamics compiled as ltv ---------------------------------------
 * Condensing x_{k+1} = A_k x_k + B_k u_k over an unstable plant and a long horizon loses the Hessian's digits
 * before a solver sees it.  With u_k = K_k x_k + v_k the unknowns of the plan are v and its recursions run on
 *   A_cl_k = A_k + B_k K_k
 * bound in A's source slot: mpcasm_assemble, mpcasm_ltv_rollout and mpcasm_ltv_advance are unchanged (the advance
 * with A_cl_0 and v_0 gives the true x_1 = A_0 x_0 + B_0 u_0).  On these matrices a cost or limit on the input
 * variable is one on v, the deviation from the feedback law; costs and limits on states are what they were.  Costs
 * and limits on the true u are had from the plant augmented by one delay (mpcasm_ltv_augment, below), in which u is
 * a state.
 * Sizes: 1 <= n <= 4 states, 1 <= m <= 4 inputs (the sweep kernel's), else MPCASM_ERR_LIMIT; a null or misaligned
 * pointer or a negative size or stride: MPCASM_ERR_ARG.
 *
 * The gains, by a backward Riccati sweep over every instance's own sequence: A (batch, T, n, n), B (batch, T, n,
 * m), a_stride / b_stride doubles between instances (0: one sequence shared); Q (n, n) and R (m, m) symmetric,
 * shared by the batch; d_PT (n, n) the terminal P, NULL: Q.  For k = T - 1 .. 0, in this order,
 *   S = R + B_k^T P B_k (the upper triangle, mirrored);  S = L L^T;  K_k = -S^-1 (B_k^T P A_k) by the two triangular
 *   solves;  A_cl_k = A_k + B_k K_k;  P <- Q + A_k^T (P A_cl_k);  P <- (P + P^T) / 2.
 * d_K (batch, T, m, n), d_Acl (batch, T, n, n; NULL: not wanted), d_info (batch) int32: -1, or the step k whose
 * pivot was not positive (NaN too) -- that step's K and A_cl and every earlier step's are NaN, the later ones
 * stand.  One lane per instance: the batch is the parallelism. */
int mpcasm_ltv_lqr(int n, int m, int T, int batch, const double* d_A, int64_t a_stride, const double* d_B,
                   int64_t b_stride, const double* d_Q, const double* d_R, const double* d_PT, double* d_K,
                   double* d_Acl, int32_t* d_info, void* stream);

/* A_cl = A + B K (batch, T, n, n) for gains the caller brings: K at d_K + b k_stride + k k_step_stride, (m, n) --
 * strides (k_stride, k_step_stride) = (0, 0): one gain; (m n, 0): one per instance; (T m n, m n): one per instance
 * and step.  A, B and their strides as for mpcasm_ltv_lqr. */
int mpcasm_ltv_close(int n, int m, int T, int batch, const double* d_A, int64_t a_stride, const double* d_B,
                     int64_t b_stride, const double* d_K, int64_t k_stride, int64_t k_step_stride, double* d_Acl,
                     void* stream);

/* The closed loop with the true input as a state: z_k = [x_k ; u_{k-1}] (n + m states), input v,
 *   z_{k+1} = At_k z_k + Bt_k v_k,   At_k = [[A_k + B_k K_k, 0], [K_k, 0]],   Bt_k = [[B_k], [I_m]]
 * so that sample k of the last m states is z_{k+1}[n:] = K_k x_k + v_k = u_k: a formulation written on (At, Bt)
 * puts costs and limits on the true input as costs and limits on a state, and mpcasm_assemble, mpcasm_ltv_rollout
 * and mpcasm_ltv_advance run on it unchanged (the advance leaves x_1 in the first n slots of an axis and u_0 in the
 * last m).  A, B, K and their strides exactly as for mpcasm_ltv_close.  d_At (batch, T, n + m, n + m), d_Bt (batch,
 * T, n + m, m), d_Kt (batch, T, m, n + m) = [K_k | 0], what mpcasm_ltv_true_inputs takes on the augmented plan
 * (NULL: not wanted).  The A + B K block is summed in mpcasm_ltv_close's order (A first, then the products by FMA):
 * on the same data it is that entry's result bit for bit; the K blocks and B are copies, every other element is
 * exactly +0.0 or 1.0.  The initial u_{-1} of an axis must be finite and is otherwise without influence (its
 * columns of At are zero).  n + m > 4 (the sweep kernel's states), or n or m not in 1 .. 4: MPCASM_ERR_LIMIT; a
 * null (d_Kt excepted) or misaligned pointer, a negative size or stride: MPCASM_ERR_ARG; T == 0 or batch == 0:
 * MPCASM_OK, nothing launched -- all decided on the host.  One lane per output element, one launch. */
int mpcasm_ltv_augment(int n, int m, int T, int batch, const double* d_A, int64_t a_stride, const double* d_B,
                       int64_t b_stride, const double* d_K, int64_t k_stride, int64_t k_step_stride, double* d_At,
                       double* d_Bt, double* d_Kt, void* stream);

/* The true inputs of a plan compiled with ltv= whose two source slots hold the closed-loop window (A_cl (N, n, n),
 * B (N, n, m) per instance): for every instance b and axis, along x_{k+1} = A_cl_k x_k + B_k v_k from the axis'
 * initial state in row d_index[b] of d_given (rows x ng; NULL: row b, rows >= count) with v the axis' unknowns in
 * row b of d_optim (count x no), u_k = K_k x_k + v_k for all N steps into d_out (count, axes, N, m).  d_K: the
 * window's gains (N, m, n) per instance, k_stride doubles between instances (0: shared).  The axes, the column of
 * the initial state and the columns of the inputs come from the plan's sweep tables, as for mpcasm_ltv_advance; an
 * instance whose index lies outside d_given writes nothing.  h_src / h_src_stride as for mpcasm_assemble.
 * MPCASM_ERR_ARG for a plan without a dynamics compiled as ltv. */
int mpcasm_ltv_true_inputs(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                           const double* d_K, int64_t k_stride, const double* d_given, int64_t rows,
                           const double* d_optim, const int32_t* d_index, double* d_out, int count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCASM_H */
