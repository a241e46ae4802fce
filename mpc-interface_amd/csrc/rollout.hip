// rollout.hip -- f2 and the end of the tick for a dynamics compiled as ltv (sweep.hip's plans): the preview rows
// of a solution and the next tick's `given`, by the forward recursion x_{k+1} = A_k x_k + B_k u_k -- WITHOUT a
// horizon matrix and without a workspace in HBM.
//
// Reference semantics: Formulation.preview (body.py:209-219) is Mg given + Mo optim for every definition; on the
// horizon matrices of tools.extend_matrices (tools.py:14-33) row k of a state is x_{k+1}, so on a plan the sweep
// kernel takes -- every unknown an input of the one system, every given value an initial state, every definition's
// row a fixed combination of ONE step's states (or the given values / the unknowns themselves) -- the rows are
//     a copy of `given`                       (the initial states: x0_*)
//     a copy of an input's block of `optim`   (the unknowns themselves)
//     c . x_{k+1}                             (states and outputs)
// and the next tick's given (biped_mpc_loop.py:62-95 with per-step dynamics) is x_1 of every axis.  The route
// through fill_su(ltv) + preview_rows writes and reads m N N n doubles per instance to say the same.
//
// A workgroup takes `group` consecutive instances (sized from the plan: what they stage shares the workgroup's
// LDS):
//   1. stage  every instance's A (N, n, n), B (N, n, m) and its row of optim into LDS: each byte read once, 16
//             bytes per lane, consecutive lanes consecutive pieces (an instance's blocks are contiguous; a block
//             that starts on an odd double is read from the 16-byte boundary inside it); its row of given -- at
//             most 16 doubles -- by 8-byte loads, one element per lane;
//   2. chain  one lane per (instance, axis) runs the recursion out of LDS, in fp64 FMAs, and parks the
//             trajectory x_1 .. x_N in LDS (by state, along k: the next phase reads it with stride 1);
//   3. rows   all lanes form the rows of the row table (mpcasm_ltv_rollout_compile) and store them in 16-byte
//             pieces along k -- the instances of a workgroup are neighbours in `out`, so the whole workgroup
//             writes ONE contiguous run -- with the stores the other result-writing kernels use; and / or x_1
//             goes into the instance's row of `given` (mpcasm_ltv_advance: only A_0, B_0, u_0 are staged and
//             one step is run).
// The row table is a separate small device table (as a given map is): its header is held against the plan, and
// every index read from it against the plan's sizes; a table of another plan writes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "device_common.h"
#include "kernels.h"

namespace mpcasm {

namespace {

constexpr int RO_BLOCK = 256;
constexpr int RO_GROUP_MAX = 8;             // instances of one workgroup
constexpr int RO_GROUP_LDS = 52 * 1024;     // ... as many as fit in this (three workgroups share a CU's LDS)
constexpr int RO_TABLE_MAX = 4096;          // words of a row table behind its header (they are copied to LDS)

// Row table: header RT_HDR words, then rec [nrec][MPCASM_ROLL_REC_WORDS], then cvec [ncvec][SW_NMAX] doubles
// (low, high word).  The records lie in the order of the rows and cover every row of the preview program once.
enum { RT_MAGIC_W, RT_N, RT_M, RT_HORIZON, RT_NAXES, RT_PMROWS, RT_NG, RT_NO, RT_NREC, RT_NCVEC, RT_PAD0, RT_PAD1,
       RT_HDR };
constexpr int RT_MAGIC = 0x4C4F5231;  // "1ROL"
enum { RR_KIND, RR_ROW0, RR_COUNT, RR_AXIS, RR_K0, RR_KSTEP, RR_CVEC, RR_PAD };
static_assert(RR_PAD + 1 == MPCASM_ROLL_REC_WORDS, "record layout");

// LDS of a workgroup (doubles): the table's body, the rows of `given` the instances use (ints), then per instance
// [A | B | trajectory | optim | given], each part on an even offset.  `steps`: N, or 1 for the advance alone.
struct RollLds {
  int body, rowof, inst0;             // shared part
  int a, b, traj, opt, giv, per;      // per instance
};
__host__ __device__ inline int even(int x) { return x + (x & 1); }
__host__ __device__ inline RollLds roll_lds(const PlanDev& p, int body_words, int steps, bool rows) {
  const int n = p.sw_n, m = p.sw_m;
  RollLds L;
  L.body = 0;
  L.rowof = even((body_words + 1) / 2);
  L.inst0 = L.rowof + RO_GROUP_MAX / 2;
  L.a = 0;
  L.b = L.a + even(steps * n * n);
  L.traj = L.b + even(steps * n * m);
  L.opt = L.traj + even(p.sw_naxes * n * steps);
  L.giv = L.opt + (rows ? even(p.no) : 0);
  L.per = L.giv + even(p.ng);
  if (((L.per >> 1) & 1) == 0) L.per += 2;   // (an odd number of 16-byte pieces: the instances' copies of one
  return L;                                  //  element of A lie in different banks)
}

struct RollArgs {
  const double* A;
  long long strideA;
  const double* B;
  long long strideB;
  const int32_t* table;
  long long table_words;
  double* given;          // (written only with write_given)
  long long rows;
  const double* optim;
  const int32_t* index;   // nullptr: instance b is row b
  const int32_t* status;  // nullptr: every instance applies
  unsigned apply_mask;
  double* out;            // nullptr: no rows (one step is run)
  int write_given;
  int count;
  int group;
};

// `cnt` doubles of every live instance g from src + (inst0 + g) * stride into its part of LDS: 16 bytes per lane
// from the 16-byte boundaries of the block (the element in front of the first, behind the last: one double)
__device__ __forceinline__ void stage(double* lds, int per, int off, const double* src, long long stride, long inst0,
                                      int live, int cnt, int tid) {
  const int pieces = cnt / 2 + 1;
  for (int w = tid; w < live * pieces; w += RO_BLOCK) {
    const int g = w / pieces, pc = w - g * pieces;
    const double* s = src + (inst0 + g) * stride;
    double* d = lds + (size_t)g * per + off;
    const int e = 2 * pc - (int)((reinterpret_cast<uintptr_t>(s) >> 3) & 1);
    if (e >= 0 && e + 1 < cnt) {
      const double2 v = *reinterpret_cast<const double2*>(s + e);
      d[e] = v.x;
      d[e + 1] = v.y;
    } else {
      if (e >= 0 && e < cnt) d[e] = s[e];
      if (e + 1 >= 0 && e + 1 < cnt) d[e + 1] = s[e + 1];
    }
  }
}

// the recursion of one (instance, axis): x <- A_k x + B_k u_k, k = 0 .. steps - 1, x_{k+1} parked at
// traj[i * steps + k].  u: the instance's optim (LDS, or global for the single step of the advance).
template <int NS, int MS>
__device__ __forceinline__ void roll_chain(const double* __restrict__ As, const double* __restrict__ Bs,
                                           const double* __restrict__ u, const int* ucol, const double* x0,
                                           double* __restrict__ traj, int steps) {
  double x[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) x[i] = x0[i];
  for (int k = 0; k < steps; ++k) {
    const double* Ak = As + k * NS * NS;
    const double* Bk = Bs + k * NS * MS;
    double uk[MS], y[NS];
#pragma unroll
    for (int j = 0; j < MS; ++j) uk[j] = u[ucol[j] + k];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      double acc = Ak[i * NS] * x[0];
#pragma unroll
      for (int s = 1; s < NS; ++s) acc = fma(Ak[i * NS + s], x[s], acc);
#pragma unroll
      for (int j = 0; j < MS; ++j) acc = fma(Bk[i * MS + j], uk[j], acc);
      y[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      x[i] = y[i];
      traj[i * steps + k] = y[i];
    }
  }
}

__global__ __launch_bounds__(RO_BLOCK) void ltv_rollout_kernel(PlanDev p, RollArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x;
  const int n = p.sw_n, m = p.sw_m, N = p.sw_horizon, naxes = p.sw_naxes, ng = p.ng, no = p.no, pmrows = p.pmrows;
  const int32_t* t = a.table;
  // (uniform: every thread of every workgroup takes the same way out)
  if (a.table_words < RT_HDR || t[RT_MAGIC_W] != RT_MAGIC || t[RT_N] != n || t[RT_M] != m || t[RT_HORIZON] != N ||
      t[RT_NAXES] != naxes || t[RT_PMROWS] != pmrows || t[RT_NG] != ng || t[RT_NO] != no)
    return;
  const int nrec = t[RT_NREC], ncvec = t[RT_NCVEC];
  if (nrec < 1 || ncvec < 0 || nrec > RO_TABLE_MAX || ncvec > RO_TABLE_MAX ||
      RT_HDR + (long long)MPCASM_ROLL_REC_WORDS * nrec + 2LL * SW_NMAX * ncvec != a.table_words ||
      a.table_words - RT_HDR > RO_TABLE_MAX)
    return;
  const int body_words = (int)(a.table_words - RT_HDR);
  const bool rows_out = a.out != nullptr;
  const int steps = rows_out ? N : 1;
  const RollLds L = roll_lds(p, body_words, steps, rows_out);
  int32_t* body = reinterpret_cast<int32_t*>(lds + L.body);
  const int32_t* rec = body;
  const double* cvec = reinterpret_cast<const double*>(body + MPCASM_ROLL_REC_WORDS * nrec);
  int32_t* rowof = reinterpret_cast<int32_t*>(lds + L.rowof);   // [group] the instance's row of given, or -1
  double* il = lds + L.inst0;
  const int32_t* axis = p.itab + p.off_sw_axis;
  const long inst0 = (long)blockIdx.x * a.group;
  const int live = (int)std::min<long>(a.group, a.count - inst0);
  if (live <= 0) return;

  // ---- 1. stage --------------------------------------------------------------------------------------------
  for (int w = tid; w < body_words; w += RO_BLOCK) body[w] = t[RT_HDR + w];
  stage(il, L.per, L.a, a.A, a.strideA, inst0, live, steps * n * n, tid);
  stage(il, L.per, L.b, a.B, a.strideB, inst0, live, steps * n * m, tid);
  if (rows_out) stage(il, L.per, L.opt, a.optim, no, inst0, live, no, tid);
  for (int w = tid; w < live * ng; w += RO_BLOCK) {
    const int g = w / ng, c = w - g * ng;
    const long row = a.index ? (long)a.index[inst0 + g] : inst0 + g;
    const bool ok = row >= 0 && row < a.rows;
    il[(size_t)g * L.per + L.giv + c] = ok ? a.given[row * ng + c] : 0.0;
    if (c == 0) rowof[g] = ok ? (int32_t)row : -1;
  }
  __syncthreads();

  // ---- 2. chain: lane (instance, axis) -----------------------------------------------------------------------
  if (tid < live * naxes) {
    const int g = tid / naxes, ax = tid - g * naxes;
    double* mine = il + (size_t)g * L.per;
    const int32_t* aw = axis + ax * SW_AXIS_WORDS;
    int ucol[SW_MMAX];
#pragma unroll
    for (int j = 0; j < SW_MMAX; ++j) ucol[j] = j < m ? aw[1 + j] : 0;
    const double* u = rows_out ? mine + L.opt : a.optim + (inst0 + g) * no;
    const double* x0 = mine + L.giv + aw[0];
    double* traj = mine + L.traj + ax * n * steps;
    switch (n * 8 + m) {
#define MPCASM_ROLL_CASE(NS, MS)                                               \
  case NS * 8 + MS:                                                            \
    roll_chain<NS, MS>(mine + L.a, mine + L.b, u, ucol, x0, traj, steps);      \
    break;
      MPCASM_ROLL_CASE(1, 1) MPCASM_ROLL_CASE(1, 2) MPCASM_ROLL_CASE(1, 3) MPCASM_ROLL_CASE(1, 4)
      MPCASM_ROLL_CASE(2, 1) MPCASM_ROLL_CASE(2, 2) MPCASM_ROLL_CASE(2, 3) MPCASM_ROLL_CASE(2, 4)
      MPCASM_ROLL_CASE(3, 1) MPCASM_ROLL_CASE(3, 2) MPCASM_ROLL_CASE(3, 3) MPCASM_ROLL_CASE(3, 4)
      MPCASM_ROLL_CASE(4, 1) MPCASM_ROLL_CASE(4, 2) MPCASM_ROLL_CASE(4, 3) MPCASM_ROLL_CASE(4, 4)
#undef MPCASM_ROLL_CASE
    }
  }
  __syncthreads();

  // ---- 3. rows: element e of the workgroup's run of `out` = row e % pmrows of instance e / pmrows -------------
  if (rows_out) {
    auto value = [&](int e, double& v) -> bool {
      const int g = e / pmrows, r = e - g * pmrows;
      if (rowof[g] < 0) return false;
      int lo = 0, hi = nrec;                       // the last record that starts at or in front of row r
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rec[mid * MPCASM_ROLL_REC_WORDS + RR_ROW0] <= r) lo = mid; else hi = mid;
      }
      const int32_t* rc = rec + lo * MPCASM_ROLL_REC_WORDS;
      const int i = r - rc[RR_ROW0];
      if (i < 0 || i >= rc[RR_COUNT]) return false;
      const int k = rc[RR_K0] + i * rc[RR_KSTEP];
      const double* mine = il + (size_t)g * L.per;
      switch (rc[RR_KIND]) {
        case MPCASM_ROLL_GIVEN:
          if (k < 0 || k >= ng) return false;
          v = mine[L.giv + k];
          return true;
        case MPCASM_ROLL_OPTIM:
          if (k < 0 || k >= no) return false;
          v = mine[L.opt + k];
          return true;
        case MPCASM_ROLL_STATE: {
          const int ax = rc[RR_AXIS], cv = rc[RR_CVEC];
          if (k < 0 || k >= N || ax < 0 || ax >= naxes || cv < 0 || cv >= ncvec) return false;
          const double* c = cvec + cv * SW_NMAX;
          const double* x = mine + L.traj + ax * n * N + k;
          double acc = c[0] * x[0];
          for (int s = 1; s < n; ++s) acc = fma(c[s], x[s * N], acc);
          v = acc;
          return true;
        }
        default:
          return false;
      }
    };
    double* ob = a.out + inst0 * pmrows;
    const int total = live * pmrows;
    const int head = (int)((reinterpret_cast<uintptr_t>(ob) >> 3) & 1);
    for (int w = tid; w < total / 2 + 1; w += RO_BLOCK) {
      const int e = 2 * w - head;
      double v0 = 0.0, v1 = 0.0;
      const bool ok0 = e >= 0 && e < total && value(e, v0);
      const bool ok1 = e + 1 < total && value(e + 1, v1);
      if (ok0 && ok1) {
        store_result(reinterpret_cast<double2*>(ob + e), double2{v0, v1});
      } else {
        if (ok0) store_result(ob + e, v0);
        if (ok1) store_result(ob + e + 1, v1);
      }
    }
  }
  // ---- ... and / or x_1 into the instance's row of given -------------------------------------------------------
  if (a.write_given)
    for (int w = tid; w < live * naxes * n; w += RO_BLOCK) {
      const int g = w / (naxes * n), r = w - g * naxes * n, ax = r / n, i = r - ax * n;
      const int row = rowof[g];
      if (row < 0) continue;
      if (a.status) {
        const int s = a.status[inst0 + g], bit = s < 0 ? -s : s;
        if (bit > 31 || !((a.apply_mask >> bit) & 1u)) continue;
      }
      a.given[(long)row * ng + axis[ax * SW_AXIS_WORDS] + i] =
          il[(size_t)g * L.per + L.traj + (ax * n + i) * steps];
    }
}

}  // namespace

// the words of a row table for plan `p` from the caller's records and combinations: every index a launch reads is
// checked here, once, against the plan
int compile_rollout_table(const PlanDev& p, const int32_t* recs, int nrec, const double* cvec, int ncvec,
                          std::vector<int32_t>* out) {
  if (nrec < 1 || ncvec < 0 || (long long)MPCASM_ROLL_REC_WORDS * nrec + 2LL * SW_NMAX * ncvec > RO_TABLE_MAX)
    return MPCASM_ERR_LIMIT;
  long long next = 0;
  for (int r = 0; r < nrec; ++r) {
    const int32_t* rc = recs + (size_t)r * MPCASM_ROLL_REC_WORDS;
    const long long cnt = rc[RR_COUNT], k0 = rc[RR_K0], k1 = k0 + (cnt - 1) * (long long)rc[RR_KSTEP];
    if (cnt < 1 || rc[RR_ROW0] != next) return MPCASM_ERR_ARG;   // (in the rows' order, every row once)
    next += cnt;
    long long width;
    switch (rc[RR_KIND]) {
      case MPCASM_ROLL_GIVEN: width = p.ng; break;
      case MPCASM_ROLL_OPTIM: width = p.no; break;
      case MPCASM_ROLL_STATE:
        width = p.sw_horizon;
        if (rc[RR_AXIS] < 0 || rc[RR_AXIS] >= p.sw_naxes || rc[RR_CVEC] < 0 || rc[RR_CVEC] >= ncvec)
          return MPCASM_ERR_ARG;
        break;
      default: return MPCASM_ERR_ARG;
    }
    if (k0 < 0 || k0 >= width || k1 < 0 || k1 >= width) return MPCASM_ERR_ARG;
  }
  if (next != p.pmrows) return MPCASM_ERR_ARG;
  for (int i = 0; i < ncvec * SW_NMAX; ++i)
    if (!std::isfinite(cvec[i]) || (i % SW_NMAX >= p.sw_n && cvec[i] != 0.0)) return MPCASM_ERR_ARG;
  out->assign({RT_MAGIC, p.sw_n, p.sw_m, p.sw_horizon, p.sw_naxes, p.pmrows, p.ng, p.no, nrec, ncvec, 0, 0});
  out->insert(out->end(), recs, recs + (size_t)nrec * MPCASM_ROLL_REC_WORDS);
  for (int i = 0; i < ncvec * SW_NMAX; ++i) {
    int32_t w[2];
    memcpy(w, &cvec[i], sizeof(double));
    out->insert(out->end(), {w[0], w[1]});
  }
  return MPCASM_OK;
}

// the geometry of a launch of `count` >= 1 instances, with the rows (all N steps, optim staged) or without (the
// advance: one step): the instances of a workgroup, its LDS bytes, the workgroups -- host only, what the launch
// below runs and mpcasm_ltv_rollout_info reports
int ltv_rollout_geometry(const PlanDev& p, long long table_words, bool rows_out, int count, RolloutGeometry* geo) {
  const int n = p.sw_n, m = p.sw_m, naxes = p.sw_naxes;
  if (n < 1 || n > SW_NMAX || m < 1 || m > SW_MMAX || naxes < 1 || naxes > SW_AXMAX) return MPCASM_ERR_LIMIT;
  if (table_words < RT_HDR || table_words - RT_HDR > RO_TABLE_MAX) return MPCASM_ERR_ARG;
  const RollLds L = roll_lds(p, (int)(table_words - RT_HDR), rows_out ? p.sw_horizon : 1, rows_out);
  const size_t shared = (size_t)L.inst0 * sizeof(double), per = (size_t)L.per * sizeof(double);
  if (shared + per > (size_t)RESIDENT_LDS_LIMIT) return MPCASM_ERR_LIMIT;
  int group = shared + per >= (size_t)RO_GROUP_LDS ? 1 : (int)((RO_GROUP_LDS - shared) / per);
  group = std::max(1, std::min({group, RO_GROUP_MAX, count}));
  geo->group = group;
  geo->lds = shared + group * per;
  geo->grid = (unsigned)((count + group - 1) / group);
  return MPCASM_OK;
}

int launch_ltv_rollout(const PlanDev& p, const SrcTable& src, const int32_t* table, long long table_words,
                       double* given, long long rows, const double* optim, const int32_t* index,
                       const int32_t* status, unsigned apply_mask, double* out, int write_given, int count,
                       hipStream_t stream, hipError_t* err) {
  *err = hipSuccess;
  if (count == 0) return MPCASM_OK;
  RolloutGeometry geo;
  const int rc = ltv_rollout_geometry(p, table_words, out != nullptr, count, &geo);
  if (rc != MPCASM_OK) return rc;
  const RollArgs a{src.ptr[p.sw_src_a], src.stride[p.sw_src_a], src.ptr[p.sw_src_b], src.stride[p.sw_src_b],
                   table, table_words, given, rows, optim, index, status, apply_mask, out, write_given, count,
                   geo.group};
  return launch_with_lds(ltv_rollout_kernel, geo.grid, RO_BLOCK, geo.lds, stream, err, p, a);
}

}  // namespace mpcasm
