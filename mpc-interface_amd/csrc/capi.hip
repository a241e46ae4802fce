// capi.hip -- extern "C" boundary of libmpcasm.so (declared in include/mpcasm.h).
// Argument checking, the upload of a checked plan and kernel dispatch; no kernel code, and no plan checking
// either: that is plan_check.cpp, reached from here through host_plan.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "jit.h"
#include "kernels.h"

using namespace mpcasm;

namespace mpcasm {
Options g_options;
}

// mpcasm_plan_set_option: a plan's own choice of path / per-plan compilation / workgroups per CU / workgroups per
// launch (-1: the process-wide value of mpcasm_set_option)
struct PlanOptions {
  int path = -1, jit = -1, per_cu = -1, grid = -1;
};

namespace {

thread_local int g_last_hip = 0;

// an index a plan derives from its host tables and keeps on its device (adjoint.hip): built and uploaded once, by
// whichever call comes first, under the plan's index_mutex -- held across build and upload
template <class Index>
struct DeviceIndex {
  int rc = 1;   // what that attempt returned (1: not tried yet)
  int hip = 0;  // ... and its hipError_t, published again by every call that meets the failure
  Index index;
  int32_t* d_words = nullptr;

  int get(std::mutex& mutex, const PlanDev& dev, const int32_t* h_itab,
          int (*build)(const PlanDev&, const int32_t*, Index*), const Index** out) {
    std::lock_guard<std::mutex> lock(mutex);
    if (rc == 1) {
      rc = build(dev, h_itab, &index);
      if (rc == MPCASM_OK) {
        const size_t bytes = std::max<size_t>(index.words.size(), 1) * sizeof(int32_t);
        hipError_t e = hipMalloc(&d_words, bytes);
        if (e == hipSuccess && !index.words.empty())
          e = hipMemcpy(d_words, index.words.data(), index.words.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
          release();
          rc = MPCASM_ERR_HIP;
          hip = (int)e;
        }
        index.view.idx = d_words;
      }
    }
    if (rc == MPCASM_ERR_HIP) g_last_hip = hip;
    *out = &index;
    return rc;
  }
  void release() {
    if (d_words) (void)hipFree(d_words);
    d_words = nullptr;
  }
};

}  // namespace

struct mpcasm_plan {
  PlanDev dev;
  int32_t* d_itab;
  double* d_dtab;
  int device;
  int num_cus;
  std::vector<int32_t> h_itab;  // host copy: what a specialised kernel is generated from (jit.hip)
  PlanOptions opt;
  // mpcasm_plan_last_kernel: what the latest mpcasm_assemble launched (two threads on one plan: the last writer)
  mutable std::atomic<int> last_kernel{0};
  // the transposed index of mpcasm_assemble_jvp / _vjp and the parameter index of mpcasm_assemble_params_vjp
  mutable std::mutex index_mutex;
  mutable DeviceIndex<AdjointIndex> adj;
  mutable DeviceIndex<ParamsIndex> par;
};

namespace {

int hip_fail(hipError_t e) {
  g_last_hip = (int)e;
  return MPCASM_ERR_HIP;
}
// what an entry returns after a launch (err is read only where the launch set it)
int launched(int rc, const hipError_t& err) {
  if (rc == MPCASM_ERR_HIP) g_last_hip = (int)err;
  return rc;
}

// every option, once: its id, the least and the greatest value mpcasm_set_option takes, the process-wide value and,
// for the four a plan may set for itself, the plan's own (mpcasm_plan_set_option takes -1 beside the range)
struct OptionRow {
  int id, least, greatest;
  std::atomic<int> Options::*wide;
  int PlanOptions::*own;
};
constexpr OptionRow OPTION_TABLE[] = {
    {MPCASM_OPT_PATH, 0, 4, &Options::path, &PlanOptions::path},
    {MPCASM_OPT_PHASE_MASK, INT_MIN, INT_MAX, &Options::phase_mask, nullptr},
    {MPCASM_OPT_P_DIRECT, 0, 2, &Options::p_direct, nullptr},
    {MPCASM_OPT_JIT, 0, 2, &Options::jit, &PlanOptions::jit},
    {MPCASM_OPT_RESIDENT_PER_CU, 0, 16, &Options::per_cu, &PlanOptions::per_cu},
    {MPCASM_OPT_JIT_FETCH_RUNS, 0, FS_MAX, &Options::fetch_runs, nullptr},
    {MPCASM_OPT_RESIDENT_GRID, 0, 1 << 20, &Options::grid, &PlanOptions::grid},
};
const OptionRow* option_row(int id) {
  for (const OptionRow& row : OPTION_TABLE)
    if (row.id == id) return &row;
  return nullptr;
}

// the options a launch of `plan` runs under, or with plan == nullptr the process-wide ones: the only place where
// "the plan's own value, else the process-wide one" is written
LaunchOptions launch_options(const mpcasm_plan* plan) {
  const auto pick = [plan](int PlanOptions::*own, const std::atomic<int>& wide) {
    return plan && plan->opt.*own >= 0 ? plan->opt.*own : wide.load(std::memory_order_relaxed);
  };
  const Options& g = g_options;
  return LaunchOptions{pick(&PlanOptions::path, g.path),     pick(&PlanOptions::jit, g.jit),
                       pick(&PlanOptions::per_cu, g.per_cu), pick(&PlanOptions::grid, g.grid),
                       g.phase_mask.load(std::memory_order_relaxed), g.fetch_runs.load(std::memory_order_relaxed)};
}

// ---- the checks the QP entries share (every one of them decided before any device call) -------------------
bool qp_sizes_ok(int no, int nc) { return no >= 1 && nc >= 0 && no <= (1 << 12) && nc <= (1 << 16); }
bool qp_pointers_ok(const QpBatch& b) {
  return b.P && b.q && b.x && (b.nc == 0 || (b.G && b.h && b.y && b.z));
}
bool qp_steps_ok(double sigma, double alpha) { return sigma > 0.0 && alpha > 0.0 && alpha < 2.0; }
bool qp_solve_settings_ok(const QpSolve& s) {
  for (double eps : {s.eps_abs, s.eps_rel, s.eps_prim_inf, s.eps_dual_inf})
    if (!(eps >= 0.0) || !std::isfinite(eps)) return false;
  return s.max_iter >= 0 && s.check_every >= 1 && s.adaptive_rho_interval >= 0 &&
         s.adaptive_rho_interval % s.check_every == 0 && qp_steps_ok(s.sigma, s.alpha);
}
bool qp_polish_settings_ok(const QpPolish& p) {
  return p.refine_iters >= 0 && p.delta > 0.0 && std::isfinite(p.delta);
}

bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// ---- what the entries are composed of, each in its own order ------------------------
// the plan's tables (and its compiled kernels) live on the device it was created on
bool on_plan_device(const mpcasm_plan* plan) {
  int current = -1;
  return hipGetDevice(&current) == hipSuccess && current == plan->device;
}

// a plan with sources and no table of them (an entry whose OK or LIMIT answers come first asks this early)
bool sources_missing(const PlanDev& d, const void* h_src, const int64_t* h_src_stride) {
  return d.nsrc != 0 && (!h_src || !h_src_stride);
}
// the sources of a launch: every one there, no stride negative
int plan_sources(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride, SrcTable* out) {
  if (sources_missing(plan->dev, h_src, h_src_stride)) return MPCASM_ERR_ARG;
  memset(out, 0, sizeof(*out));
  for (int s = 0; s < plan->dev.nsrc; ++s) {
    if (!h_src[s] || h_src_stride[s] < 0) return MPCASM_ERR_ARG;
    out->ptr[s] = h_src[s];
    out->stride[s] = h_src_stride[s];
  }
  return MPCASM_OK;
}
// ... and of a host-only query, which decides by the strides alone
int stride_table(const PlanDev& d, const int64_t* h_src_stride, SrcTable* out) {
  if (d.nsrc != 0 && !h_src_stride) return MPCASM_ERR_ARG;
  memset(out, 0, sizeof(*out));
  for (int s = 0; s < d.nsrc; ++s) {
    if (h_src_stride[s] < 0) return MPCASM_ERR_ARG;
    out->stride[s] = h_src_stride[s];
  }
  return MPCASM_OK;
}

// the streams a launch reads (eff) where the plan was compiled with lti=: its horizon tables are made in the
// workspace, so it needs one.  lti_prepass: the pre-pass of n instances; lti_refusals: what it refuses, nothing
// launched (for an entry that builds an index between the two)
int lti_prepass(const mpcasm_plan* plan, const SrcTable& src, void* d_work, int n, void* stream, SrcTable* eff) {
  if (plan->dev.t_nlti != 0 && !d_work) return MPCASM_ERR_ARG;
  hipError_t err;
  const int rc = launch_lti_tables(plan->dev, src, static_cast<double*>(d_work), n, plan->h_itab.data(), eff,
                                   static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}
int lti_refusals(const mpcasm_plan* plan, const SrcTable& src, void* d_work, SrcTable* eff) {
  if (plan->dev.t_nlti != 0 && !d_work) return MPCASM_ERR_ARG;
  return lti_effective_sources(plan->dev, src, static_cast<double*>(d_work), plan->h_itab.data(), eff);
}

// the table pointers of a host-only query (and of mpcasm_plan_create); the entry checks its own pointers and
// scalars beside them, zeroes its results, and goes on to host_plan: ERR_ARG leaves the results as they were
bool tables_missing(const int32_t* h_itab, const double* h_dtab, size_t n_dtab) {
  return !h_itab || (n_dtab && !h_dtab);
}
// the tables checked (plan_check.cpp), then their view, with the persistent kernel's hand-over of P chosen
int host_plan(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab, PlanDev* d) {
  const int rc = validate_plan(h_itab, h_dtab, n_itab, n_dtab);
  if (rc != MPCASM_OK) return rc;
  memset(d, 0, sizeof *d);
  plan_view(h_itab, d);
  d->rs_p_direct = d->rs_ok ? resident_choose_p_direct(*d, g_options.p_direct.load(std::memory_order_relaxed)) : 0;
  // the CSC form of P is read out of its LDS copy: such a plan has no other way
  if (d->csc_pnnz != 0 && d->rs_ok) d->rs_p_direct = resident_choose_p_direct(*d, 2);
  return MPCASM_OK;
}

// out[0..3] of the two infos of the assembly's derivative
template <class Index>
void index_info(const Index& index, int32_t out[4]) {
  out[0] = (int32_t)index.lds;
  out[1] = index.lds > 64 * 1024;
  out[2] = (int32_t)index.words.size();
  out[3] = index.per_cu;
}

// how a compile entry ends: the size alone for a caller that passes no buffer, else the words copied out
int words_out(const std::vector<int32_t>& made, int32_t* h_out, int64_t capacity, int64_t* words) {
  *words = (int64_t)made.size();
  if (h_out == nullptr) return MPCASM_OK;
  if (capacity < (int64_t)made.size()) return MPCASM_ERR_ARG;
  memcpy(h_out, made.data(), made.size() * sizeof(int32_t));
  return MPCASM_OK;
}

}  // namespace

extern "C" {

int mpcasm_abi_version(void) { return 1004; }

int mpcasm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int mpcasm_last_hip(void) { return g_last_hip; }

int mpcasm_set_option(int option, int value) {
  const OptionRow* row = option_row(option);
  if (!row || value < row->least || value > row->greatest) return MPCASM_ERR_ARG;
  (g_options.*row->wide).store(value, std::memory_order_relaxed);
  return MPCASM_OK;
}

int mpcasm_plan_set_option(mpcasm_plan* plan, int option, int value) {
  if (!plan) return MPCASM_ERR_ARG;
  const OptionRow* row = option_row(option);
  if (!row || !row->own || (value != -1 && (value < row->least || value > row->greatest))) return MPCASM_ERR_ARG;
  plan->opt.*row->own = value;
  return MPCASM_OK;
}

const char* mpcasm_status_string(int status) {
  switch (status) {
    case MPCASM_OK: return "ok";
    case MPCASM_ERR_ARG: return "invalid argument";
    case MPCASM_ERR_PLAN: return "malformed plan tables";
    case MPCASM_ERR_HIP: return "HIP runtime error";
    case MPCASM_ERR_NODEVICE: return "no HIP device";
    case MPCASM_ERR_LIMIT: return "problem exceeds a kernel limit";
    default: return "unknown status";
  }
}

int mpcasm_fill_su(const double* d_A, const double* d_B, double* d_S, double* d_U, int batch,
                   int N, int n, int m, int ltv, void* stream) {
  if (!d_A || !d_B || !d_S || !d_U) return MPCASM_ERR_ARG;
  if (batch < 0 || N < 1 || n < 1 || m < 1 || (ltv != 0 && ltv != 1)) return MPCASM_ERR_ARG;
  if (batch == 0) return MPCASM_OK;
  if (mpcasm_device_count() == 0) return MPCASM_ERR_NODEVICE;
  hipError_t err;
  const int rc = launch_fill_su(d_A, d_B, d_S, d_U, batch, N, n, m, ltv,
                                static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_fill_route(int batch, int N, int n, int m, int ltv, int aligned16, int32_t out[8]) {
  if (!out) return MPCASM_ERR_ARG;
  memset(out, 0, 8 * sizeof(int32_t));
  if (batch < 1 || N < 1 || n < 1 || m < 1 || (ltv != 0 && ltv != 1) || (aligned16 != 0 && aligned16 != 1))
    return MPCASM_ERR_ARG;
  FillChoice c;
  const int rc = fill_choose(batch, N, n, m, ltv, aligned16 != 0, &c);
  if (rc != MPCASM_OK) return rc;
  out[0] = c.kernel;
  out[1] = c.arg;
  out[2] = (c.generic ? MPCASM_FILL_GENERIC : 0) | (c.pad ? MPCASM_FILL_PAD : 0) |
           (c.whole_lines ? MPCASM_FILL_WHOLE_LINES : 0);
  out[3] = c.spw;
  out[4] = c.lshift;
  out[5] = c.grid;
  out[6] = (int32_t)c.lds;
  out[7] = c.lds > 64 * 1024;
  return MPCASM_OK;
}

int mpcasm_plan_create(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                       mpcasm_plan** out_plan) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !out_plan) return MPCASM_ERR_ARG;
  *out_plan = nullptr;
  PlanDev view;
  const int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, &view);
  if (rc != MPCASM_OK) return rc;
  // a CSC plan runs on the persistent kernel with P in LDS, or not at all
  if ((view.csc_pnnz != 0 || view.csc_gnnz != 0) &&
      (view.rs_p_direct != 0 || resident_lds_bytes(view) == 0 || resident_lds_bytes(view) > RESIDENT_LDS_LIMIT))
    return MPCASM_ERR_LIMIT;
  if (mpcasm_device_count() == 0) return MPCASM_ERR_NODEVICE;

  mpcasm_plan* plan = new (std::nothrow) mpcasm_plan();
  if (!plan) return MPCASM_ERR_ARG;
  hipError_t e;
  if ((e = hipGetDevice(&plan->device)) != hipSuccess) {
    delete plan;
    return hip_fail(e);
  }
  plan->d_itab = nullptr;
  plan->d_dtab = nullptr;
  const size_t dbytes = (n_dtab ? n_dtab : 1) * sizeof(double);
  if ((e = hipMalloc(&plan->d_itab, n_itab * sizeof(int32_t))) != hipSuccess ||
      (e = hipMalloc(&plan->d_dtab, dbytes)) != hipSuccess ||
      (e = hipMemcpy(plan->d_itab, h_itab, n_itab * sizeof(int32_t), hipMemcpyHostToDevice)) !=
          hipSuccess ||
      (n_dtab && (e = hipMemcpy(plan->d_dtab, h_dtab, n_dtab * sizeof(double),
                                hipMemcpyHostToDevice)) != hipSuccess)) {
    if (plan->d_itab) (void)hipFree(plan->d_itab);
    if (plan->d_dtab) (void)hipFree(plan->d_dtab);
    delete plan;
    return hip_fail(e);
  }
  plan->dev = view;
  plan->dev.itab = plan->d_itab;
  plan->dev.dtab = plan->d_dtab;
  plan->h_itab.assign(h_itab, h_itab + n_itab);
  {
    hipDeviceProp_t prop;
    plan->num_cus = 256;
    if (hipGetDeviceProperties(&prop, plan->device) == hipSuccess && prop.multiProcessorCount > 0)
      plan->num_cus = prop.multiProcessorCount;
  }
  *out_plan = plan;
  return MPCASM_OK;
}

int mpcasm_resident_lds_bytes(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                              int64_t out[2]) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !out) return MPCASM_ERR_ARG;
  PlanDev d;
  const int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, &d);
  if (rc != MPCASM_OK) return rc;
  for (int direct = 0; direct < 2; ++direct) {
    d.rs_p_direct = 1 - direct;  // out[0]: P direct, out[1]: P in LDS
    out[direct] = (int64_t)resident_lds_bytes(d);
  }
  return MPCASM_OK;
}

int mpcasm_jit_check(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                     char* log, size_t log_capacity) {
  if (tables_missing(h_itab, h_dtab, n_dtab)) return MPCASM_ERR_ARG;
  if (log && log_capacity) log[0] = 0;
  PlanDev d;
  const int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, &d);
  if (rc != MPCASM_OK) return rc;
  if (!d.rs_ok) return MPCASM_ERR_LIMIT;
  std::vector<char> code;
  std::string text;
  // (both forms of the P hand-over when the size of a launch picks one)
  const int small = resident_p_direct_for(d, 1), large = resident_p_direct_for(d, 1 << 30);
  int out = MPCASM_OK;
  if (!jit_available()) {
    text = "libhiprtc.so could not be loaded";
    out = MPCASM_ERR_LIMIT;
  } else {
    for (int form : {small, large}) {
      if (form == large && small != large && out != MPCASM_OK) break;
      d.rs_p_direct = form;
      // (through the disk cache, as a launch would: a second check of the same plan compiles nothing)
      out = jit_code_for(jit_spec_header(d, h_itab, launch_options(nullptr).fetch_runs), false, 0xBF, &code, &text) ? MPCASM_OK : MPCASM_ERR_HIP;
      if (small == large) break;
    }
  }
  if (log && log_capacity) {
    strncpy(log, text.c_str(), log_capacity - 1);
    log[log_capacity - 1] = 0;
  }
  return out;
}

int mpcasm_fetch_segments(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                          int limit, int32_t* out, size_t capacity, int64_t* n_words) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !n_words || (capacity && !out) || limit < 0) return MPCASM_ERR_ARG;
  PlanDev d;
  const int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, &d);
  if (rc != MPCASM_OK) return rc;
  if (!d.rs_ok) return MPCASM_ERR_LIMIT;
  const std::vector<int32_t> words = jit_fetch_plan(d, h_itab, limit);
  *n_words = (int64_t)words.size();
  if (words.size() > capacity) return MPCASM_ERR_LIMIT;
  if (!words.empty()) memcpy(out, words.data(), words.size() * sizeof(int32_t));
  return MPCASM_OK;
}

int mpcasm_jit_stats(int64_t out[3]) {
  if (!out) return MPCASM_ERR_ARG;
  long v[3];
  jit_stats(v);
  out[0] = v[0];
  out[1] = v[1];
  out[2] = v[2];
  return MPCASM_OK;
}

int mpcasm_plan_prepare(const mpcasm_plan* plan, int batch) {
  if (!plan || batch < 0 || !on_plan_device(plan)) return MPCASM_ERR_ARG;
  const LaunchOptions opt = launch_options(plan);
  AssembleRoute r;
  // (nothing is compiled per plan for the other kernels; input alignment is taken as given)
  if (assemble_route(plan->dev, batch, opt, true, false, &r) != MPCASM_OK || r.kernel != MPCASM_KERNEL_RESIDENT)
    return MPCASM_OK;
  PlanDev p = plan->dev;
  p.rs_p_direct = r.p_direct;
  // (a failure: the ahead-of-time kernel)
  (void)jit_kernel_for(p, plan->h_itab.data(), plan->device, batch, r.lds, opt.jit, opt.phase_mask, opt.fetch_runs);
  return MPCASM_OK;
}

int mpcasm_plan_destroy(mpcasm_plan* plan) {
  if (!plan) return MPCASM_OK;
  jit_forget(plan->d_itab);
  plan->adj.release();
  plan->par.release();
  hipError_t e1 = hipFree(plan->d_itab);
  hipError_t e2 = hipFree(plan->d_dtab);
  delete plan;
  if (e1 != hipSuccess) return hip_fail(e1);
  if (e2 != hipSuccess) return hip_fail(e2);
  return MPCASM_OK;
}

int mpcasm_plan_sizes(const mpcasm_plan* plan, int64_t out[8]) {
  if (!plan || !out) return MPCASM_ERR_ARG;
  const PlanDev& d = plan->dev;
  out[0] = d.ng; out[1] = d.no; out[2] = d.nc; out[3] = d.nparams;
  out[4] = d.nsrc; out[5] = d.rtot; out[6] = d.ldv; out[7] = d.pmrows;
  return MPCASM_OK;
}

int mpcasm_plan_csc_sizes(const mpcasm_plan* plan, int64_t out[2]) {
  if (!plan || !out) return MPCASM_ERR_ARG;
  out[0] = plan->dev.csc_pnnz;
  out[1] = plan->dev.csc_gnnz;
  return MPCASM_OK;
}

int mpcasm_workspace_bytes(const mpcasm_plan* plan, int batch, size_t* out_bytes) {
  if (!plan || !out_bytes || batch < 0) return MPCASM_ERR_ARG;
  // the staged pipeline's workspace; never less than the cycle stamps of the diagnostic
  // persistent kernel take (8 wavefronts x 8 counters per resident workgroup for the phases
  // of the instance loop, as many again for the set-up)
  const size_t groups = (size_t)std::min<long>(batch, (long)plan->num_cus * 8);
  const size_t stamps = 2 * groups * 8 * 8 * sizeof(uint64_t);
  // a wide problem on the tiled kernel needs d and the generated horizon tables only -- unless the
  // options in force send it down the staged pipeline (a test hook): ask again after changing them
  const int path = launch_options(plan).path;
  if (sweep_eligible(plan->dev)) {  // (everything in LDS)
    *out_bytes = stamps;
    return MPCASM_OK;
  }
  if (tiled_eligible(plan->dev) && path != 2) {
    *out_bytes = std::max(tiled_workspace_bytes(plan->dev, batch), stamps);
    return MPCASM_OK;
  }
  // (the generated horizon tables of mpcasm_preview_direct fit in either case)
  *out_bytes = std::max(std::max(assemble_workspace_bytes(plan->dev, batch),
                                 tiled_workspace_bytes(plan->dev, batch)), stamps);
  return MPCASM_OK;
}

static int assemble_impl(const mpcasm_plan* plan, const double* const* h_src,
                         const int64_t* h_src_stride, const double* d_params, const double* d_given,
                         const int32_t* d_given_index, double* d_P, double* d_q, double* d_G, double* d_h,
                         void* d_work, int batch, void* stream) {
  if (!plan || batch < 0) return MPCASM_ERR_ARG;
  if (batch == 0) return MPCASM_OK;  // nothing to do (empty buffers may be null)
  const PlanDev& d = plan->dev;
  if ((d.nparams && !d_params) || (d.ng && !d_given)) return MPCASM_ERR_ARG;
  if ((d_P == nullptr) != (d_q == nullptr) || (d_G == nullptr) != (d_h == nullptr))
    return MPCASM_ERR_ARG;
  if (d.rtot && !d_work && !d.sw_ok) return MPCASM_ERR_ARG;
  if (!on_plan_device(plan)) return MPCASM_ERR_ARG;
  // results leave the chip in 16-byte stores
  if (misaligned(d_P, 15) || misaligned(d_q, 15) || misaligned(d_G, 15) || misaligned(d_h, 15)) return MPCASM_ERR_ARG;
  SrcTable src;
  int rc = plan_sources(plan, h_src, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  if (d_given_index != nullptr) {
    // the index of `given`'s rows rides in the last slot of the source table (resident.hip)
    if (d.nsrc >= MAX_SOURCES || d.ng == 0) return MPCASM_ERR_LIMIT;
    src.ptr[MAX_SOURCES - 1] = reinterpret_cast<const double*>(d_given_index);
    src.stride[MAX_SOURCES - 1] = -1;
  }
  hipError_t err;
  int kernel = MPCASM_KERNEL_NONE;
  const AssembleCall call{src, d_params, d_given, d_P, d_q, d_G, d_h, d_work, batch,
                          static_cast<hipStream_t>(stream), plan->num_cus, plan->device, plan->h_itab.data(),
                          d_given_index != nullptr, launch_options(plan), &err, &kernel};
  rc = launch_assemble(d, call);
  if (rc == MPCASM_OK) plan->last_kernel.store(kernel, std::memory_order_relaxed);
  return launched(rc, err);
}

int mpcasm_assemble(const mpcasm_plan* plan, const double* const* h_src,
                    const int64_t* h_src_stride, const double* d_params, const double* d_given,
                    double* d_P, double* d_q, double* d_G, double* d_h, void* d_work, int batch,
                    void* stream) {
  return assemble_impl(plan, h_src, h_src_stride, d_params, d_given, nullptr, d_P, d_q, d_G, d_h, d_work,
                       batch, stream);
}

int mpcasm_assemble_indexed(const mpcasm_plan* plan, const double* const* h_src,
                            const int64_t* h_src_stride, const double* d_params, const double* d_given,
                            const int32_t* d_given_index, double* d_P, double* d_q, double* d_G,
                            double* d_h, void* d_work, int batch, void* stream) {
  if (!d_given_index) return MPCASM_ERR_ARG;
  return assemble_impl(plan, h_src, h_src_stride, d_params, d_given, d_given_index, d_P, d_q, d_G, d_h,
                       d_work, batch, stream);
}

int mpcasm_plan_last_kernel(const mpcasm_plan* plan) {
  return plan ? plan->last_kernel.load(std::memory_order_relaxed) : MPCASM_ERR_ARG;
}

int mpcasm_preview_matrices(const mpcasm_plan* plan, const double* const* h_src,
                            const int64_t* h_src_stride, double* d_PM, int batch, void* stream) {
  if (!plan || !d_PM || batch < 0) return MPCASM_ERR_ARG;
  if (sources_missing(plan->dev, h_src, h_src_stride)) return MPCASM_ERR_ARG;
  if (plan->dev.rs_nlti != 0 || plan->dev.sw_ok) return MPCASM_ERR_LIMIT;  // the plan has no S, U to read
  if (batch == 0) return MPCASM_OK;
  if (!on_plan_device(plan)) return MPCASM_ERR_ARG;
  SrcTable src;
  int rc = plan_sources(plan, h_src, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  hipError_t err;
  rc = launch_preview_matrices(plan->dev, src, d_PM, batch, static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_preview(const double* d_PM, const double* d_given, const double* d_optim, double* d_out,
                   int batch, int rows, int ng, int no, void* stream) {
  if (!d_PM || !d_out || batch < 0 || rows < 0 || ng < 0 || no < 0) return MPCASM_ERR_ARG;
  if ((ng && !d_given) || (no && !d_optim)) return MPCASM_ERR_ARG;
  if (batch == 0 || rows == 0) return MPCASM_OK;
  hipError_t err;
  const int rc = launch_preview(d_PM, d_given, d_optim, d_out, batch, rows, ng, no,
                                static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_preview_direct(const mpcasm_plan* plan, const double* const* h_src,
                          const int64_t* h_src_stride, const double* d_given, const double* d_optim,
                          double* d_out, void* d_work, int batch, void* stream) {
  if (!plan || !d_out || batch < 0) return MPCASM_ERR_ARG;
  const PlanDev& d = plan->dev;
  if (sources_missing(d, h_src, h_src_stride) || (d.ng && !d_given) || (d.no && !d_optim)) return MPCASM_ERR_ARG;
  if (batch == 0 || d.pmrows == 0) return MPCASM_OK;
  if (d.sw_ok) return MPCASM_ERR_LIMIT;  // (per-step dynamics: no horizon tables to preview from)
  if (!on_plan_device(plan)) return MPCASM_ERR_ARG;
  SrcTable src, eff;
  int rc = plan_sources(plan, h_src, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  rc = lti_prepass(plan, src, d_work, batch, stream, &eff);
  if (rc != MPCASM_OK) return rc;
  hipError_t err;
  rc = launch_preview_direct(d, eff, d_given, d_optim, d_out, batch, plan->num_cus,
                             static_cast<hipStream_t>(stream), &err, plan->h_itab.data());
  return launched(rc, err);
}

namespace {
// the plan's transposed index on its device, and (mpcasm_assemble_params_vjp) its parameter index
int plan_adjoint_index(const mpcasm_plan* plan, const AdjointIndex** out) {
  return plan->adj.get(plan->index_mutex, plan->dev, plan->h_itab.data(), adjoint_build_index, out);
}
int plan_params_index(const mpcasm_plan* plan, const ParamsIndex** out) {
  return plan->par.get(plan->index_mutex, plan->dev, plan->h_itab.data(), params_adjoint_build_index, out);
}

// JVP: in_x = d, out_x = dq, out_h = dh;  VJP: in_x = gq, in_h = gh, out_x = ggiven
int adjoint_impl(const mpcasm_plan* plan, bool vjp, const double* const* h_src, const int64_t* h_src_stride,
                 const double* d_params, const double* in_x, const double* in_h, double* out_x, double* out_h,
                 void* d_work, int batch, void* stream) {
  if (!plan || batch < 0) return MPCASM_ERR_ARG;
  const PlanDev& d = plan->dev;
  if (vjp ? (!in_x && !in_h) : (!out_x && !out_h)) return MPCASM_ERR_ARG;
  if (d.sw_ok) return MPCASM_ERR_LIMIT;  // (per-step dynamics: no S, U; the adjoint is the sweep's backward recursion)
  if (batch == 0 || d.ng == 0) return MPCASM_OK;
  if ((d.nparams && !d_params) || (vjp ? !out_x : !in_x) || !on_plan_device(plan)) return MPCASM_ERR_ARG;
  SrcTable src, eff;
  int rc = plan_sources(plan, h_src, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  rc = lti_refusals(plan, src, d_work, &eff);  // (before the index is built for nothing)
  if (rc != MPCASM_OK) return rc;
  const AdjointIndex* index;
  rc = plan_adjoint_index(plan, &index);
  if (rc != MPCASM_OK) return rc;
  rc = lti_prepass(plan, src, d_work, batch, stream, &eff);
  if (rc != MPCASM_OK) return rc;
  hipError_t err;
  rc = launch_assemble_adjoint(d, eff, *index, vjp, d_params, in_x, in_h, out_x, out_h, batch, plan->num_cus,
                               static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}
}  // namespace

int mpcasm_assemble_jvp(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                        const double* d_params, const double* d_dgiven, double* d_dq, double* d_dh, void* d_work,
                        int batch, void* stream) {
  return adjoint_impl(plan, false, h_src, h_src_stride, d_params, d_dgiven, nullptr, d_dq, d_dh, d_work, batch,
                      stream);
}

int mpcasm_assemble_vjp(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                        const double* d_params, const double* d_gq, const double* d_gh, double* d_ggiven,
                        void* d_work, int batch, void* stream) {
  return adjoint_impl(plan, true, h_src, h_src_stride, d_params, d_gq, d_gh, d_ggiven, nullptr, d_work, batch,
                      stream);
}

namespace {
// what the host-only queries about a plan with horizon matrices share (the two infos of the assembly's derivative,
// mpcasm_preview_route): the tables checked and viewed, the strides taken -- missing ones before, negative ones
// after the refusal of a plan compiled with ltv= -- and what the pre-pass of a plan compiled with lti= refuses
int horizon_query_plan(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                       const int64_t* h_src_stride, PlanDev* d, SrcTable* eff) {
  int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, d);
  if (rc != MPCASM_OK) return rc;
  if (d->nsrc && !h_src_stride) return MPCASM_ERR_ARG;
  if (d->sw_ok) return MPCASM_ERR_LIMIT;  // (as mpcasm_preview_direct, adjoint_impl)
  SrcTable src;
  rc = stride_table(*d, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  return lti_effective_sources(*d, src, nullptr, h_itab, eff);
}
}  // namespace

int mpcasm_assemble_params_vjp(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                               const double* d_params, const double* d_given, const double* d_x, const double* d_u,
                               const double* d_y, const double* d_w, const int32_t* d_verdict, double* d_gparams,
                               void* d_work, int batch, void* stream) {
  if (!plan || batch < 0) return MPCASM_ERR_ARG;
  const PlanDev& d = plan->dev;
  if (d.sw_ok) return MPCASM_ERR_LIMIT;  // (per-step dynamics: no S, U; the adjoint is the sweep's backward recursion)
  if (batch == 0 || d.nparams == 0) return MPCASM_OK;
  if (!d_params || !d_gparams || (d.ng && !d_given) || (d.no && (!d_x || !d_u)) || (d.nc && (!d_y || !d_w)) ||
      !on_plan_device(plan))
    return MPCASM_ERR_ARG;
  SrcTable src, eff;
  int rc = plan_sources(plan, h_src, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  rc = lti_refusals(plan, src, d_work, &eff);  // (before an index is built for nothing)
  if (rc != MPCASM_OK) return rc;
  const AdjointIndex* adj;
  rc = plan_adjoint_index(plan, &adj);
  if (rc != MPCASM_OK) return rc;
  const ParamsIndex* index;
  rc = plan_params_index(plan, &index);
  if (rc != MPCASM_OK) return rc;
  rc = lti_prepass(plan, src, d_work, batch, stream, &eff);
  if (rc != MPCASM_OK) return rc;
  hipError_t err;
  rc = launch_assemble_params_adjoint(d, eff, *adj, *index, d_params, d_given, d_x, d_u, d_y, d_w, d_verdict,
                                      d_gparams, batch, plan->num_cus, static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_assemble_params_vjp_info(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                                    const int64_t* h_src_stride, int32_t out[4]) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !out) return MPCASM_ERR_ARG;
  memset(out, 0, 4 * sizeof(int32_t));
  PlanDev d;
  SrcTable eff;
  const int rc = horizon_query_plan(h_itab, n_itab, h_dtab, n_dtab, h_src_stride, &d, &eff);
  if (rc != MPCASM_OK) return rc;
  AdjointIndex adj;
  const int first = adjoint_build_index(d, h_itab, &adj);
  if (first != MPCASM_OK) return first;
  ParamsIndex index;
  const int built = params_adjoint_build_index(d, h_itab, &index);
  if (built != MPCASM_OK) return built;
  index_info(index, out);
  return MPCASM_OK;
}

int mpcasm_assemble_adjoint_info(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                                 const int64_t* h_src_stride, int32_t out[4]) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !out) return MPCASM_ERR_ARG;
  memset(out, 0, 4 * sizeof(int32_t));
  PlanDev d;
  SrcTable eff;
  const int rc = horizon_query_plan(h_itab, n_itab, h_dtab, n_dtab, h_src_stride, &d, &eff);
  if (rc != MPCASM_OK) return rc;
  AdjointIndex index;
  const int built = adjoint_build_index(d, h_itab, &index);
  if (built != MPCASM_OK) return built;
  index_info(index, out);
  return MPCASM_OK;
}

int mpcasm_preview_route(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                         const int64_t* h_src_stride, int nterms, int ngoals, int32_t out[8]) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !out || nterms < 0 || ngoals < 0) return MPCASM_ERR_ARG;
  memset(out, 0, 8 * sizeof(int32_t));
  PlanDev d;
  SrcTable eff;
  const int rc = horizon_query_plan(h_itab, n_itab, h_dtab, n_dtab, h_src_stride, &d, &eff);
  if (rc != MPCASM_OK) return rc;
  return preview_route(d, eff, h_itab, nterms, ngoals, out);
}

int mpcasm_sweep_route(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab, int32_t out[8]) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !out) return MPCASM_ERR_ARG;
  memset(out, 0, 8 * sizeof(int32_t));
  PlanDev d;
  const int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, &d);
  if (rc != MPCASM_OK) return rc;
  if (!sweep_eligible(d)) return MPCASM_ERR_ARG;  // (no dynamics compiled as ltv: another kernel's plan)
  SweepChoice c;
  const int choice = sweep_choose(d, h_itab, &c);
  if (choice != MPCASM_OK) return choice;
  out[0] = c.cpt;
  out[1] = c.specialised;
  out[2] = c.pair;
  out[3] = c.per_line;
  out[4] = c.reg_lines;
  out[5] = sweep_lines_ahead(c.cpt);
  out[6] = (int32_t)c.lds;
  out[7] = c.lds > 64 * 1024;
  return MPCASM_OK;
}

int mpcasm_tiled_route(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                       const int64_t* h_src_stride, int batch, int want, int path, int32_t out[16]) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !out || batch < 1 || path < -1 || path > 4 || want < 1 || want > 3)
    return MPCASM_ERR_ARG;
  memset(out, 0, 16 * sizeof(int32_t));
  PlanDev d;
  int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, &d);
  if (rc != MPCASM_OK) return rc;
  SrcTable src;
  rc = stride_table(d, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  LaunchOptions opt = launch_options(nullptr);
  if (path >= 0) opt.path = path;
  AssembleRoute r;
  if (assemble_route(d, batch, opt, true, false, &r) != MPCASM_OK || r.kernel != MPCASM_KERNEL_TILED)
    return MPCASM_ERR_ARG;
  d.rs_p_direct = r.p_direct;
  TiledChoice c;
  const int choice = tiled_choose(d, src, h_itab, opt.path, batch, (want & MPCASM_WANT_COST) != 0,
                                  (want & MPCASM_WANT_CONSTRAINTS) != 0, true, true, &c);
  if (choice != MPCASM_OK) return choice;
  out[0] = c.form;
  out[1] = c.fused;
  out[2] = c.kp;
  out[3] = c.cb;
  out[4] = c.rows_in_lds;
  out[5] = c.whole_lines;
  out[6] = (int32_t)c.lds;
  out[7] = c.lds > 64 * 1024;
  out[8] = c.tables;
  out[9] = c.tg;
  out[10] = c.sym;
  return MPCASM_OK;
}

int mpcasm_assemble_route(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab, int batch,
                          int path, int inputs_aligned, int indexed, int32_t out[4]) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !out || batch < 1 || path < -1 || path > 4 ||
      (inputs_aligned != 0 && inputs_aligned != 1) || (indexed != 0 && indexed != 1))
    return MPCASM_ERR_ARG;
  memset(out, 0, 4 * sizeof(int32_t));
  PlanDev d;
  int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, &d);
  if (rc != MPCASM_OK) return rc;
  LaunchOptions opt = launch_options(nullptr);
  if (path >= 0) opt.path = path;
  AssembleRoute r;
  rc = assemble_route(d, batch, opt, inputs_aligned != 0, indexed != 0, &r);
  if (rc != MPCASM_OK) return rc;
  out[0] = r.kernel;
  out[1] = (int32_t)r.lds;
  out[2] = r.p_direct;
  return MPCASM_OK;
}

int mpcasm_staged_route(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab, int want_cost,
                        int want_constraints, int batch, int32_t out[8]) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !out || batch < 1 || (want_cost != 0 && want_cost != 1) ||
      (want_constraints != 0 && want_constraints != 1) || (!want_cost && !want_constraints))
    return MPCASM_ERR_ARG;
  memset(out, 0, 8 * sizeof(int32_t));
  PlanDev d;
  int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, &d);
  if (rc != MPCASM_OK) return rc;
  // a plan the pipeline can run at all: what MPCASM_OPT_PATH 2 reaches it with (not a dynamics compiled as ltv,
  // no horizon matrices generated from (A, B), no CSC results)
  LaunchOptions opt = launch_options(nullptr);
  opt.path = 2;
  AssembleRoute r;
  if (assemble_route(d, batch, opt, false, false, &r) != MPCASM_OK || r.kernel != MPCASM_KERNEL_STAGED)
    return MPCASM_ERR_ARG;
  StagedChoice c;
  rc = staged_choose(d, want_cost != 0, want_constraints != 0, batch, &c);
  if (rc != MPCASM_OK) return rc;
  out[0] = c.hessian;
  out[1] = (c.sym ? MPCASM_STAGED_SYM : 0) | (c.whole_lines ? MPCASM_STAGED_WHOLE_LINES : 0) | (c.max_axes << 8);
  out[2] = c.hessian == MPCASM_STAGED_GEMM ? c.nb : c.nbr;
  out[3] = c.hessian == MPCASM_STAGED_GEMM ? c.npairs : c.nbc;
  out[4] = (int32_t)c.grid_k2;
  out[5] = (int32_t)c.grid_k3;
  out[6] = (int32_t)c.grid_gradient;
  out[7] = (int32_t)c.grid_k4;
  return MPCASM_OK;
}

int mpcasm_given_map_compile(const mpcasm_plan* plan, const int32_t* h_rows, const double* h_values, int ng,
                             int32_t* h_map, int64_t capacity, int64_t* words) {
  if (!plan || !h_rows || !words || capacity < 0) return MPCASM_ERR_ARG;
  const PlanDev& d = plan->dev;
  if (ng != d.ng) return MPCASM_ERR_ARG;
  if (d.sw_ok || !d.t_ci_ok) return MPCASM_ERR_LIMIT;  // (as mpcasm_preview_direct)
  for (int c = 0; c < ng; ++c) {
    const int r = h_rows[c];
    if (r == MPCASM_GIVEN_CONST ? (!h_values || !std::isfinite(h_values[c]))
                                : (r != MPCASM_GIVEN_KEEP && (r < 0 || r >= d.pmrows)))
      return MPCASM_ERR_ARG;
  }
  std::vector<int32_t> map;
  const int rc = compile_given_map(d, plan->h_itab.data(), h_rows, h_values, &map);
  if (rc != MPCASM_OK) return rc;
  return words_out(map, h_map, capacity, words);
}

int mpcasm_next_given(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                      double* d_given, int64_t rows, const double* d_optim, const int32_t* d_index,
                      const int32_t* d_status, uint32_t apply_mask, const int32_t* d_map, int64_t map_words,
                      void* d_work, int count, void* stream) {
  if (!plan || count < 0 || rows < 0 || map_words < 0) return MPCASM_ERR_ARG;
  const PlanDev& d = plan->dev;
  if (d.sw_ok || !d.t_ci_ok) return MPCASM_ERR_LIMIT;  // (as mpcasm_preview_direct)
  if (count == 0 || d.ng == 0) return MPCASM_OK;
  if (!d_given || !d_map || (d.no && !d_optim)) return MPCASM_ERR_ARG;
  if ((!d_index && rows < count) || !on_plan_device(plan)) return MPCASM_ERR_ARG;
  SrcTable src, eff;
  int rc = plan_sources(plan, h_src, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  rc = lti_prepass(plan, src, d_work, count, stream, &eff);
  if (rc != MPCASM_OK) return rc;
  hipError_t err;
  rc = launch_next_given(d, eff, d_map, map_words, d_given, rows, d_optim, d_index, d_status, apply_mask, count,
                         plan->num_cus, static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_ltv_rollout_compile(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                               const int32_t h_sizes[7], const int32_t* h_recs, int nrec, const double* h_cvec,
                               int ncvec, int32_t* h_table, int64_t capacity, int64_t* words) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !h_sizes || !h_recs || !words || nrec < 1 || ncvec < 0 ||
      (ncvec && !h_cvec) || capacity < 0)
    return MPCASM_ERR_ARG;
  PlanDev d;
  const int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, &d);
  if (rc != MPCASM_OK) return rc;
  if (!d.sw_ok) return MPCASM_ERR_ARG;  // (no dynamics compiled as ltv: mpcasm_preview_direct's plan)
  const int32_t have[7] = {d.sw_n, d.sw_m, d.sw_horizon, d.sw_naxes, d.pmrows, d.ng, d.no};
  if (memcmp(have, h_sizes, sizeof have) != 0) return MPCASM_ERR_ARG;
  std::vector<int32_t> table;
  const int made = compile_rollout_table(d, h_recs, nrec, h_cvec, ncvec, &table);
  if (made != MPCASM_OK) return made;
  return words_out(table, h_table, capacity, words);
}

namespace {
int rollout_impl(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride, double* d_given,
                 int64_t rows, const double* d_optim, const int32_t* d_index, const int32_t* d_status,
                 uint32_t apply_mask, const int32_t* d_table, int64_t table_words, double* d_out, int write_given,
                 int count, void* stream) {
  if (!plan || count < 0 || rows < 0 || table_words < 0) return MPCASM_ERR_ARG;
  const PlanDev& d = plan->dev;
  if (!d.sw_ok) return MPCASM_ERR_ARG;  // (a plan with horizon matrices: mpcasm_preview_direct / mpcasm_next_given)
  if (count == 0 || (!write_given && d.pmrows == 0)) return MPCASM_OK;
  if (!d_given || !d_optim || !d_table || !h_src || !h_src_stride || (!write_given && !d_out)) return MPCASM_ERR_ARG;
  if (!d_index && rows < count) return MPCASM_ERR_ARG;
  if (misaligned(d_out, 7) || !on_plan_device(plan)) return MPCASM_ERR_ARG;
  SrcTable src;
  int rc = plan_sources(plan, h_src, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  hipError_t err;
  rc = launch_ltv_rollout(d, src, d_table, table_words, d_given, rows, d_optim, d_index, d_status, apply_mask, d_out,
                          write_given, count, static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}
}  // namespace

int mpcasm_ltv_rollout(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                       const double* d_given, int64_t rows, const double* d_optim, const int32_t* d_index,
                       const int32_t* d_table, int64_t table_words, double* d_out, int count, void* stream) {
  return rollout_impl(plan, h_src, h_src_stride, const_cast<double*>(d_given), rows, d_optim, d_index, nullptr, 0u,
                      d_table, table_words, d_out, 0, count, stream);
}

int mpcasm_ltv_advance(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                       double* d_given, int64_t rows, const double* d_optim, const int32_t* d_index,
                       const int32_t* d_status, uint32_t apply_mask, const int32_t* d_table, int64_t table_words,
                       int count, void* stream) {
  return rollout_impl(plan, h_src, h_src_stride, d_given, rows, d_optim, d_index, d_status, apply_mask, d_table,
                      table_words, nullptr, 1, count, stream);
}

int mpcasm_ltv_rollout_info(const int32_t* h_itab, size_t n_itab, const double* h_dtab, size_t n_dtab,
                            int64_t table_words, int rows_out, int count, int32_t* group, int64_t* lds_bytes,
                            int32_t* workgroups) {
  if (tables_missing(h_itab, h_dtab, n_dtab) || !group || !lds_bytes || !workgroups || table_words < 0 ||
      (rows_out != 0 && rows_out != 1) || count < 0)
    return MPCASM_ERR_ARG;
  *group = 0;
  *lds_bytes = 0;
  *workgroups = 0;
  PlanDev d;
  const int rc = host_plan(h_itab, n_itab, h_dtab, n_dtab, &d);
  if (rc != MPCASM_OK) return rc;
  if (!d.sw_ok) return MPCASM_ERR_ARG;  // (as rollout_impl)
  if (count == 0 || (rows_out && d.pmrows == 0)) return MPCASM_OK;
  RolloutGeometry geo;
  const int made = ltv_rollout_geometry(d, table_words, rows_out != 0, count, &geo);
  if (made != MPCASM_OK) return made;
  *group = geo.group;
  *lds_bytes = (int64_t)geo.lds;
  *workgroups = (int32_t)geo.grid;
  return MPCASM_OK;
}

int mpcasm_ltv_lqr(int n, int m, int T, int batch, const double* d_A, int64_t a_stride, const double* d_B,
                   int64_t b_stride, const double* d_Q, const double* d_R, const double* d_PT, double* d_K,
                   double* d_Acl, int32_t* d_info, void* stream) {
  if (n < 1 || m < 1 || T < 0 || batch < 0 || a_stride < 0 || b_stride < 0) return MPCASM_ERR_ARG;
  if (n > SW_NMAX || m > SW_MMAX) return MPCASM_ERR_LIMIT;
  if (!d_A || !d_B || !d_Q || !d_R || !d_K || !d_info || misaligned(d_A, 7) || misaligned(d_B, 7) ||
      misaligned(d_Q, 7) || misaligned(d_R, 7) || misaligned(d_PT, 7) || misaligned(d_K, 7) ||
      misaligned(d_Acl, 7) || misaligned(d_info, 3))
    return MPCASM_ERR_ARG;
  hipError_t err;
  const int rc = launch_ltv_lqr(n, m, T, batch, d_A, a_stride, d_B, b_stride, d_Q, d_R, d_PT, d_K, d_Acl, d_info,
                                static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_ltv_close(int n, int m, int T, int batch, const double* d_A, int64_t a_stride, const double* d_B,
                     int64_t b_stride, const double* d_K, int64_t k_stride, int64_t k_step_stride, double* d_Acl,
                     void* stream) {
  if (n < 1 || m < 1 || T < 0 || batch < 0 || a_stride < 0 || b_stride < 0 || k_stride < 0 || k_step_stride < 0)
    return MPCASM_ERR_ARG;
  if (n > SW_NMAX || m > SW_MMAX) return MPCASM_ERR_LIMIT;
  if (!d_A || !d_B || !d_K || !d_Acl || misaligned(d_A, 7) || misaligned(d_B, 7) || misaligned(d_K, 7) ||
      misaligned(d_Acl, 7))
    return MPCASM_ERR_ARG;
  hipError_t err;
  const int rc = launch_ltv_close(n, m, T, batch, d_A, a_stride, d_B, b_stride, d_K, k_stride, k_step_stride, d_Acl,
                                  static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_ltv_augment(int n, int m, int T, int batch, const double* d_A, int64_t a_stride, const double* d_B,
                       int64_t b_stride, const double* d_K, int64_t k_stride, int64_t k_step_stride, double* d_At,
                       double* d_Bt, double* d_Kt, void* stream) {
  if (n < 0 || m < 0 || T < 0 || batch < 0 || a_stride < 0 || b_stride < 0 || k_stride < 0 || k_step_stride < 0)
    return MPCASM_ERR_ARG;
  if (n < 1 || m < 1 || n > SW_NMAX || m > SW_MMAX || n + m > SW_NMAX) return MPCASM_ERR_LIMIT;
  if (!d_A || !d_B || !d_K || !d_At || !d_Bt || misaligned(d_A, 7) || misaligned(d_B, 7) || misaligned(d_K, 7) ||
      misaligned(d_At, 7) || misaligned(d_Bt, 7) || misaligned(d_Kt, 7))
    return MPCASM_ERR_ARG;
  hipError_t err;
  const int rc = launch_ltv_augment(n, m, T, batch, d_A, a_stride, d_B, b_stride, d_K, k_stride, k_step_stride, d_At,
                                    d_Bt, d_Kt, static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_ltv_true_inputs(const mpcasm_plan* plan, const double* const* h_src, const int64_t* h_src_stride,
                           const double* d_K, int64_t k_stride, const double* d_given, int64_t rows,
                           const double* d_optim, const int32_t* d_index, double* d_out, int count, void* stream) {
  if (!plan || count < 0 || rows < 0 || k_stride < 0) return MPCASM_ERR_ARG;
  const PlanDev& d = plan->dev;
  if (!d.sw_ok) return MPCASM_ERR_ARG;  // (no dynamics compiled as ltv: as rollout_impl)
  if (count == 0) return MPCASM_OK;
  if (!d_K || !d_given || !d_optim || !d_out || !h_src || !h_src_stride || misaligned(d_K, 7) ||
      misaligned(d_given, 7) || misaligned(d_optim, 7) || misaligned(d_out, 7) || misaligned(d_index, 3))
    return MPCASM_ERR_ARG;
  if ((!d_index && rows < count) || !on_plan_device(plan)) return MPCASM_ERR_ARG;
  SrcTable src;
  int rc = plan_sources(plan, h_src, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  hipError_t err;
  rc = launch_ltv_true_inputs(d, src, d_K, k_stride, d_given, rows, d_optim, d_index, d_out, count,
                              static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_preview_goal_distance(const mpcasm_plan* plan, const double* const* h_src,
                                 const int64_t* h_src_stride, const double* d_given,
                                 const double* d_optim, const double* d_params, const int32_t* d_terms,
                                 int nterms, int ngoals, double* d_out, void* d_work, int batch,
                                 void* stream) {
  if (!plan || batch < 0 || nterms < 0 || ngoals < 0) return MPCASM_ERR_ARG;
  const PlanDev& d = plan->dev;
  if (batch == 0 || ngoals == 0) return MPCASM_OK;
  if (!d_out || sources_missing(d, h_src, h_src_stride) || (d.ng && !d_given) || (d.no && !d_optim) ||
      (nterms && (!d_terms || !d_params)))
    return MPCASM_ERR_ARG;
  if (d.sw_ok) return MPCASM_ERR_LIMIT;
  if (!on_plan_device(plan)) return MPCASM_ERR_ARG;
  SrcTable src, eff;
  int rc = plan_sources(plan, h_src, h_src_stride, &src);
  if (rc != MPCASM_OK) return rc;
  rc = lti_prepass(plan, src, d_work, batch, stream, &eff);
  if (rc != MPCASM_OK) return rc;
  hipError_t err;
  rc = launch_preview_goals(d, eff, d_given, d_optim, d_params, d.nparams, d_terms, nterms, ngoals, d_out,
                            batch, plan->num_cus, static_cast<hipStream_t>(stream), &err, plan->h_itab.data());
  return launched(rc, err);
}

int mpcasm_goal_distance(const double* d_preview, int64_t preview_stride, const double* d_params,
                         int64_t n_params, const int32_t* d_terms, int nterms, int ngoals,
                         double* d_out, int batch, void* stream) {
  if (batch < 0 || nterms < 0 || ngoals < 0 || preview_stride < 0 || n_params < 0) return MPCASM_ERR_ARG;
  if (batch == 0 || ngoals == 0) return MPCASM_OK;
  if (!d_preview || !d_out || (nterms && (!d_terms || !d_params))) return MPCASM_ERR_ARG;
  hipError_t err;
  const int rc = launch_goal_distance(d_preview, preview_stride, d_params, n_params, d_terms, nterms,
                                      ngoals, d_out, batch, static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_box_transform(double* d_params, int64_t n_params, int batch, const int32_t* d_facets,
                         int nfacets, int op, const double* d_arg, int64_t arg_stride,
                         void* stream) {
  if (batch < 0 || nfacets < 0 || n_params < 0 || arg_stride < 0 || op < MPCASM_BOX_RECENTER ||
      op > MPCASM_BOX_MARGIN)
    return MPCASM_ERR_ARG;
  if (batch == 0 || nfacets == 0) return MPCASM_OK;
  if (!d_params || !d_facets || !d_arg) return MPCASM_ERR_ARG;
  hipError_t err;
  const int rc = launch_box_transform(d_params, n_params, batch, d_facets, nfacets, op, d_arg,
                                      arg_stride, static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_box_transform_ss(double* d_params, int64_t n_params, int batch,
                            const int32_t* d_facets, int nfacets, int op, const double* d_L,
                            int lrows, int ss_dim, const double* d_arg, int64_t arg_stride,
                            void* stream) {
  if (batch < 0 || nfacets < 0 || n_params < 0 || arg_stride < 0 || lrows < 1 || ss_dim < 1 ||
      (op != MPCASM_BOX_RECENTER && op != MPCASM_BOX_TRANSLATE))
    return MPCASM_ERR_ARG;
  if (batch == 0 || nfacets == 0) return MPCASM_OK;
  if (!d_params || !d_facets || !d_L || !d_arg) return MPCASM_ERR_ARG;
  hipError_t err;
  const int rc = launch_box_transform_ss(d_params, n_params, batch, d_facets, nfacets, op, d_L,
                                         lrows, ss_dim, d_arg, arg_stride,
                                         static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_admm(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                const double* d_h, double* d_x, double* d_y, double* d_z, double* d_res, double rho,
                double sigma, double alpha, int iters, int warm, int batch, double* d_kinv, int kinv_valid,
                void* stream) {
  if (!qp_sizes_ok(no, nc) || batch < 0 || iters < 0 || !(rho > 0.0) || !qp_steps_ok(sigma, alpha)) return MPCASM_ERR_ARG;
  if (batch == 0) return MPCASM_OK;
  const QpBatch b{no, nc, batch, d_P, d_q, d_G, d_h, d_x, d_y, d_z};
  if (!qp_pointers_ok(b)) return MPCASM_ERR_ARG;
  if (kinv_valid != 0 && d_kinv == nullptr) return MPCASM_ERR_ARG;
  QpSolve s{};
  s.sigma = sigma, s.alpha = alpha, s.max_iter = iters, s.warm = warm != 0;
  s.kinv = d_kinv, s.kinv_valid = kinv_valid != 0, s.res = d_res;
  hipError_t err;
  return launched(launch_admm(b, rho, s, static_cast<hipStream_t>(stream), &err), err);
}

// the four mpcasm_qp_solve* entries: the same arguments, checked in the same order; the wide ones also ask their
// launch where K^-1 lives, before they look at the batch
// soft: the penalties of the _soft entries (NULL: the hard ones), their stride nc or 0
static int qp_solve_entry(bool wide, const QpSoft* soft, int no, int nc, const double* d_P, const double* d_q,
                          const double* d_G, const double* d_h, double* d_x, double* d_y, double* d_z, int warm,
                          double* d_rho, double sigma, double alpha, double eps_abs, double eps_rel,
                          double eps_prim_inf, double eps_dual_inf, int max_iter, int check_every,
                          int adaptive_rho_interval, int32_t* d_status, int32_t* d_iters, double* d_res, int batch,
                          double* d_kinv, int kinv_valid, void* stream) {
  const QpBatch b{no, nc, batch, d_P, d_q, d_G, d_h, d_x, d_y, d_z};
  const QpSolve s{{d_rho, d_status, d_iters, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, check_every,
                   adaptive_rho_interval},
                  sigma, alpha, max_iter, warm != 0, d_kinv, kinv_valid != 0, d_res};
  if (!qp_solve_settings_ok(s) || !qp_sizes_ok(b.no, b.nc) || b.batch < 0) return MPCASM_ERR_ARG;
  if (soft && soft->stride != 0 && soft->stride != b.nc) return MPCASM_ERR_ARG;
  int32_t on_chip = 1;
  if (wide) {
    const int limit = soft ? qp_solve_wide_soft_info(b.no, b.nc, nullptr, &on_chip)
                           : qp_solve_wide_info(b.no, b.nc, nullptr, &on_chip);
    if (limit != MPCASM_OK) return limit;
  }
  if (b.batch == 0) return MPCASM_OK;
  if (!qp_pointers_ok(b) || !s.rho || !s.status || !s.iters) return MPCASM_ERR_ARG;
  if (soft && b.nc > 0 && (!soft->lin || !soft->quad)) return MPCASM_ERR_ARG;
  if ((s.kinv_valid != 0 || on_chip == 0) && s.kinv == nullptr) return MPCASM_ERR_ARG;
  hipError_t err;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (soft)
    return launched(wide ? launch_qp_solve_wide_soft(b, s, *soft, st, &err) : launch_qp_solve_soft(b, s, *soft, st, &err),
                    err);
  return launched(wide ? launch_qp_solve_wide(b, s, st, &err) : launch_qp_solve(b, s, st, &err), err);
}
int mpcasm_qp_solve(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                    const double* d_h, double* d_x, double* d_y, double* d_z, int warm, double* d_rho,
                    double sigma, double alpha, double eps_abs, double eps_rel, double eps_prim_inf,
                    double eps_dual_inf, int max_iter, int check_every, int adaptive_rho_interval,
                    int32_t* d_status, int32_t* d_iters, double* d_res, int batch, double* d_kinv,
                    int kinv_valid, void* stream) {
  return qp_solve_entry(false, nullptr, no, nc, d_P, d_q, d_G, d_h, d_x, d_y, d_z, warm, d_rho, sigma, alpha,
                        eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, max_iter, check_every, adaptive_rho_interval,
                        d_status, d_iters, d_res, batch, d_kinv, kinv_valid, stream);
}

int mpcasm_qp_solve_lds_bytes(int no, int nc, int64_t* out) {
  if (!qp_sizes_ok(no, nc) || !out) return MPCASM_ERR_ARG;
  *out = (int64_t)admm_lds_bytes(no, nc);
  return *out > RESIDENT_LDS_LIMIT ? MPCASM_ERR_LIMIT : MPCASM_OK;
}

int mpcasm_qp_solve_wide(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                         const double* d_h, double* d_x, double* d_y, double* d_z, int warm, double* d_rho,
                         double sigma, double alpha, double eps_abs, double eps_rel, double eps_prim_inf,
                         double eps_dual_inf, int max_iter, int check_every, int adaptive_rho_interval,
                         int32_t* d_status, int32_t* d_iters, double* d_res, int batch, double* d_kinv,
                         int kinv_valid, void* stream) {
  return qp_solve_entry(true, nullptr, no, nc, d_P, d_q, d_G, d_h, d_x, d_y, d_z, warm, d_rho, sigma, alpha,
                        eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, max_iter, check_every, adaptive_rho_interval,
                        d_status, d_iters, d_res, batch, d_kinv, kinv_valid, stream);
}

int mpcasm_qp_solve_wide_info(int no, int nc, int64_t* lds_bytes, int32_t* kinv_on_chip) {
  if (!qp_sizes_ok(no, nc) || !lds_bytes || !kinv_on_chip) return MPCASM_ERR_ARG;
  return qp_solve_wide_info(no, nc, lds_bytes, kinv_on_chip);
}

int mpcasm_qp_solve_soft(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                         const double* d_h, double* d_x, double* d_y, double* d_z, int warm, double* d_rho,
                         double sigma, double alpha, double eps_abs, double eps_rel, double eps_prim_inf,
                         double eps_dual_inf, int max_iter, int check_every, int adaptive_rho_interval,
                         int32_t* d_status, int32_t* d_iters, double* d_res, int batch, double* d_kinv,
                         int kinv_valid, void* stream, const double* d_soft_lin, const double* d_soft_quad,
                         int64_t soft_stride) {
  const QpSoft soft{d_soft_lin, d_soft_quad, soft_stride};
  return qp_solve_entry(false, &soft, no, nc, d_P, d_q, d_G, d_h, d_x, d_y, d_z, warm, d_rho, sigma, alpha,
                        eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, max_iter, check_every, adaptive_rho_interval,
                        d_status, d_iters, d_res, batch, d_kinv, kinv_valid, stream);
}

int mpcasm_qp_solve_soft_lds_bytes(int no, int nc, int64_t* out) {
  if (!qp_sizes_ok(no, nc) || !out) return MPCASM_ERR_ARG;
  *out = (int64_t)admm_soft_lds_bytes(no, nc);
  return *out > RESIDENT_LDS_LIMIT ? MPCASM_ERR_LIMIT : MPCASM_OK;
}

int mpcasm_qp_solve_wide_soft(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                              const double* d_h, double* d_x, double* d_y, double* d_z, int warm, double* d_rho,
                              double sigma, double alpha, double eps_abs, double eps_rel, double eps_prim_inf,
                              double eps_dual_inf, int max_iter, int check_every, int adaptive_rho_interval,
                              int32_t* d_status, int32_t* d_iters, double* d_res, int batch, double* d_kinv,
                              int kinv_valid, void* stream, const double* d_soft_lin, const double* d_soft_quad,
                              int64_t soft_stride) {
  const QpSoft soft{d_soft_lin, d_soft_quad, soft_stride};
  return qp_solve_entry(true, &soft, no, nc, d_P, d_q, d_G, d_h, d_x, d_y, d_z, warm, d_rho, sigma, alpha,
                        eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, max_iter, check_every, adaptive_rho_interval,
                        d_status, d_iters, d_res, batch, d_kinv, kinv_valid, stream);
}

int mpcasm_qp_solve_wide_soft_info(int no, int nc, int64_t* lds_bytes, int32_t* kinv_on_chip) {
  if (!qp_sizes_ok(no, nc) || !lds_bytes || !kinv_on_chip) return MPCASM_ERR_ARG;
  return qp_solve_wide_soft_info(no, nc, lds_bytes, kinv_on_chip);
}

// the workspace of the two _wide entries behind the solve: past their size limit, then missing, misaligned or small
static int qp_wide_work(int no, int nc, int batch, const void* d_work, size_t work_bytes) {
  int64_t need = 0;
  const int limit = qp_polish_wide_info(no, nc, batch, nullptr, &need, nullptr);
  if (limit != MPCASM_OK) return limit;
  return !d_work || misaligned(d_work, 15) || work_bytes < (size_t)need ? MPCASM_ERR_ARG : MPCASM_OK;
}

// what the two polish entries decide alike: MPCASM_OK with *go set where there is something to launch
static int qp_polish_checks(const QpBatch& b, const QpPolish& p, bool* go) {
  *go = false;
  if (!qp_sizes_ok(b.no, b.nc) || b.batch < 0 || !qp_polish_settings_ok(p)) return MPCASM_ERR_ARG;
  if (b.batch == 0) return MPCASM_OK;
  if (!qp_pointers_ok(b) || !p.polish) return MPCASM_ERR_ARG;
  *go = true;
  return MPCASM_OK;
}

int mpcasm_qp_polish(int no, int nc, const double* d_P, const double* d_q, const double* d_G, const double* d_h,
                     double* d_x, double* d_y, double* d_z, const int32_t* d_status, double delta,
                     int refine_iters, int32_t* d_polish, double* d_res, int batch, void* stream) {
  const QpBatch b{no, nc, batch, d_P, d_q, d_G, d_h, d_x, d_y, d_z};
  const QpPolish p{d_status, delta, refine_iters, d_polish, d_res};
  bool go;
  const int rc = qp_polish_checks(b, p, &go);
  if (!go) return rc;
  hipError_t err;   // (past the LDS a workgroup may have: the launch's MPCASM_ERR_LIMIT)
  return launched(launch_qp_polish(b, p, static_cast<hipStream_t>(stream), &err), err);
}

int mpcasm_qp_polish_lds_bytes(int no, int nc, int64_t* out) {
  if (!qp_sizes_ok(no, nc) || !out) return MPCASM_ERR_ARG;
  *out = (int64_t)polish_lds_bytes(no, nc);
  return *out > RESIDENT_LDS_LIMIT ? MPCASM_ERR_LIMIT : MPCASM_OK;
}

int mpcasm_qp_polish_wide(int no, int nc, const double* d_P, const double* d_q, const double* d_G,
                          const double* d_h, double* d_x, double* d_y, double* d_z, const int32_t* d_status,
                          double delta, int refine_iters, int32_t* d_polish, double* d_res, int batch,
                          void* d_work, size_t work_bytes, void* stream) {
  const QpBatch b{no, nc, batch, d_P, d_q, d_G, d_h, d_x, d_y, d_z};
  const QpPolish p{d_status, delta, refine_iters, d_polish, d_res};
  bool go;
  const int rc = qp_polish_checks(b, p, &go);
  if (!go) return rc;
  const int work = qp_wide_work(no, nc, batch, d_work, work_bytes);
  if (work != MPCASM_OK) return work;
  hipError_t err;
  return launched(launch_qp_polish_wide(b, p, static_cast<double*>(d_work), static_cast<hipStream_t>(stream), &err),
                  err);
}

int mpcasm_qp_polish_wide_info(int no, int nc, int batch, int64_t* lds_bytes, int64_t* work_bytes,
                               int32_t* workgroups) {
  if (!qp_sizes_ok(no, nc) || batch < 0 || !lds_bytes || !work_bytes || !workgroups) return MPCASM_ERR_ARG;
  return qp_polish_wide_info(no, nc, batch, lds_bytes, work_bytes, workgroups);
}

// what the two sensitivity entries decide alike: MPCASM_OK with *go set where there is something to launch
static int qp_sens_checks(const QpSens& s, bool* go) {
  *go = false;
  const QpPolish settings{nullptr, s.delta, s.refine_iters, nullptr, nullptr};
  if (!qp_sizes_ok(s.no, s.nc) || s.batch < 0 || !qp_polish_settings_ok(settings)) return MPCASM_ERR_ARG;
  if (s.batch == 0) return MPCASM_OK;
  if (!s.P || !s.x || !s.rx || !s.u || !s.verdict) return MPCASM_ERR_ARG;
  if (s.nc > 0 && (!s.G || !s.h || !s.y || !s.z || !s.ry || !s.w)) return MPCASM_ERR_ARG;
  *go = true;
  return MPCASM_OK;
}

int mpcasm_qp_sens(int no, int nc, const double* d_P, const double* d_G, const double* d_h, const double* d_x,
                   const double* d_y, const double* d_z, const int32_t* d_status, const double* d_rx,
                   const double* d_ry, double delta, int refine_iters, double* d_u, double* d_w, double* d_gP,
                   double* d_gG, int32_t* d_verdict, double* d_lres, int batch, void* stream) {
  const QpSens s{no,   nc,    batch,        d_P, d_G, d_h,  d_x,  d_y,       d_z,   d_status,
                 d_rx, d_ry,  delta,        refine_iters,   d_u,  d_w,       d_gP,  d_gG,
                 d_verdict,   d_lres};
  bool go;
  const int rc = qp_sens_checks(s, &go);
  if (!go) return rc;
  hipError_t err;   // (past the LDS a workgroup may have: the launch's MPCASM_ERR_LIMIT)
  return launched(launch_qp_sens(s, static_cast<hipStream_t>(stream), &err), err);
}

int mpcasm_qp_sens_lds_bytes(int no, int nc, int64_t* out) { return mpcasm_qp_polish_lds_bytes(no, nc, out); }

int mpcasm_qp_sens_wide(int no, int nc, const double* d_P, const double* d_G, const double* d_h, const double* d_x,
                        const double* d_y, const double* d_z, const int32_t* d_status, const double* d_rx,
                        const double* d_ry, double delta, int refine_iters, double* d_u, double* d_w, double* d_gP,
                        double* d_gG, int32_t* d_verdict, double* d_lres, int batch, void* d_work, size_t work_bytes,
                        void* stream) {
  const QpSens s{no,   nc,    batch,        d_P, d_G, d_h,  d_x,  d_y,       d_z,   d_status,
                 d_rx, d_ry,  delta,        refine_iters,   d_u,  d_w,       d_gP,  d_gG,
                 d_verdict,   d_lres};
  bool go;
  const int rc = qp_sens_checks(s, &go);
  if (!go) return rc;
  const int work = qp_wide_work(no, nc, batch, d_work, work_bytes);
  if (work != MPCASM_OK) return work;
  hipError_t err;
  return launched(launch_qp_sens_wide(s, static_cast<double*>(d_work), static_cast<hipStream_t>(stream), &err), err);
}

int mpcasm_qp_sens_wide_info(int no, int nc, int batch, int64_t* lds_bytes, int64_t* work_bytes,
                             int32_t* workgroups) {
  return mpcasm_qp_polish_wide_info(no, nc, batch, lds_bytes, work_bytes, workgroups);
}

int mpcasm_qp_warm_store(int no, int nc, const double* d_x, const double* d_y, const double* d_rho,
                         const int32_t* d_status, int tag, double* d_store_x, double* d_store_y, double* d_store_rho,
                         int32_t* d_store_meta, int64_t store_rows, int store_no, int store_nc, const int32_t* d_index,
                         int count, void* stream) {
  if (no < 1 || nc < 0 || count < 0 || store_rows < 0 || store_no < 1 || store_nc < 0 || no > 512 || nc > 2048 ||
      store_no > 512 || store_nc > 2048 || no > store_no || nc > store_nc)
    return MPCASM_ERR_ARG;
  if (count == 0) return MPCASM_OK;
  if (!d_x || !d_rho || !d_status || !d_store_x || !d_store_rho || !d_store_meta || (nc > 0 && !d_y) ||
      (store_nc > 0 && !d_store_y) || (!d_index && store_rows < count))
    return MPCASM_ERR_ARG;
  hipError_t err;
  const int rc = launch_qp_warm_store(no, nc, d_x, d_y, d_rho, d_status, tag, d_store_x, d_store_y, d_store_rho,
                                      d_store_meta, store_rows, store_no, store_nc, d_index, count,
                                      static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_qp_warm_start(int no, int nc, const double* d_G, const double* d_h, const double* d_store_x,
                         const double* d_store_y, const double* d_store_rho, const int32_t* d_store_meta,
                         int64_t store_rows, int store_no, int store_nc, const int32_t* d_index,
                         const int32_t* d_col_src, const int32_t* d_row_src, int expect_tag, uint32_t warm_mask,
                         double rho_cold, double* d_x, double* d_y, double* d_z, double* d_rho, int32_t* d_warm,
                         int count, void* stream) {
  if (no < 1 || nc < 0 || count < 0 || store_rows < 0 || store_no < 1 || store_nc < 0 || no > 512 || nc > 2048 ||
      store_no > 512 || store_nc > 2048 || !std::isfinite(rho_cold))
    return MPCASM_ERR_ARG;
  if (count == 0) return MPCASM_OK;
  if (!d_store_x || !d_store_rho || !d_store_meta || !d_col_src || !d_x || !d_rho || !d_warm ||
      (nc > 0 && (!d_G || !d_h || !d_row_src || !d_y || !d_z)) || (nc > 0 && store_nc > 0 && !d_store_y))
    return MPCASM_ERR_ARG;
  hipError_t err;
  const int rc = launch_qp_warm_start(no, nc, d_G, d_h, d_store_x, d_store_y, d_store_rho, d_store_meta, store_rows,
                                      store_no, store_nc, d_index, d_col_src, d_row_src, expect_tag, warm_mask,
                                      rho_cold, d_x, d_y, d_z, d_rho, d_warm, count,
                                      static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_params_map(double* d_params, int64_t n_params, const int32_t* d_recs, const double* d_coef, int nrecs,
                      const double* d_cmd, int64_t cmd_stride, int ncmd, const int32_t* d_index,
                      const double* d_sign, int batch, void* stream) {
  if (!d_params || n_params < 1 || nrecs < 0 || ncmd < 1 || batch < 0 || cmd_stride < 0 ||
      (cmd_stride > 0 && cmd_stride < ncmd) || (nrecs > 0 && (!d_recs || !d_coef || !d_cmd)))
    return MPCASM_ERR_ARG;
  if (batch == 0 || nrecs == 0) return MPCASM_OK;
  hipError_t err;
  const int rc = launch_params_map(d_params, n_params, d_recs, d_coef, nrecs, d_cmd, cmd_stride, ncmd, d_index,
                                   d_sign, batch, static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

int mpcasm_gather(const double* d_src, int64_t src_stride, const int32_t* d_index, int nnz,
                  double* d_dst, int batch, void* stream) {
  if (nnz < 0 || batch < 0 || src_stride < 0) return MPCASM_ERR_ARG;
  if (nnz == 0 || batch == 0) return MPCASM_OK;
  if (!d_src || !d_index || !d_dst) return MPCASM_ERR_ARG;
  hipError_t err;
  const int rc = launch_gather(d_src, src_stride, d_index, nnz, d_dst, batch,
                               static_cast<hipStream_t>(stream), &err);
  return launched(rc, err);
}

}  // extern "C"

namespace mpcasm {

hipError_t allow_whole_lds(const void* fn) {
  static std::mutex mutex;
  static std::vector<std::pair<const void*, int>> done;
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mutex);
  for (const auto& d : done)
    if (d.first == fn && d.second == device) return hipSuccess;
  // (the runtime of this image refuses the CU's full 160 KiB -- hipErrorInvalidValue -- and grants
  // 156 KiB, what the kernels' own limit RESIDENT_LDS_LIMIT asks for: the larger one first, for a
  // runtime that gives it)
  for (int bytes : {CU_LDS_BYTES, RESIDENT_LDS_LIMIT}) {
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) {
      done.emplace_back(fn, device);
      return e;
    }
    (void)hipGetLastError();
  }
  return e;
}

}  // namespace mpcasm
