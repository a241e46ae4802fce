// warm.hip -- the piece between two ticks of a closed loop (mpcasm_qp_warm_store, mpcasm_qp_warm_start): after a
// solve, every instance's x, y, rho and status go into the caller's warm store, one record per row (per walker);
// before the next solve, the iterates and the step it starts from are gathered from the store through two tables
// that say where each unknown and each row of this tick's QP was in the last one (the horizon moved on by a sample,
// the structure may have changed), or set to exactly what a cold mpcasm_qp_solve starts from.  include/mpcasm.h
// states the rule, tests/warm_restatement.py restates it.
//
// The store is four arrays: X [rows][store_no], Y [rows][store_nc], rho [rows], meta [rows][2] int32 (status, tag).
//
// warm_start_kernel: 256 threads serve ipw = 1, 2 or 4 instances (4, 2, 1 wavefronts each: the biped's G is 22 KB,
// two instances share a workgroup -- ws_ipw).  Per instance, in dynamic LDS: x0 [no], y0 [nc] and a flag.
//   1. the record's header is judged (tag, status bit, rho), by every thread alike;
//   2. x0 and y0 are gathered into LDS, a value that is not finite raises the flag;
//   3. behind a barrier the branch is known: x, y, rho and d_warm are written, and z -- cold min(0, h), warm
//      min(G x0, h) with G read in place, once, with plain loads (the solve reads the same G next): lpr = 16, 32 or
//      64 lanes along a row (64 / lpr rows side by side in a wavefront), four such rows in flight, 16-byte loads
//      where no is even and G starts on 16 bytes (every row then does), 8-byte loads otherwise.
// Nothing is read out of range whatever the tables and the index hold: an index outside the store makes the
// instance cold, a table entry outside its range counts as -1.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "kernels.h"

namespace mpcasm {

namespace {

constexpr int WS_BLOCK = 256;
constexpr int WS_ROWS = 4;   // rows (per group of lpr lanes) in flight: 2 measures the same, 8 a third slower

__host__ __device__ inline int ws_even(int n) { return n + (n & 1); }
// doubles of LDS one instance takes: x0, y0 (each on 16 bytes) and the flag
__host__ __device__ inline int ws_slot(int no, int nc) { return ws_even(no) + ws_even(nc) + 2; }

__device__ __forceinline__ bool ws_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

template <int VEC>
__global__ __launch_bounds__(WS_BLOCK) void warm_start_kernel(
    int no, int nc, const double* __restrict__ G, const double* __restrict__ h, const double* __restrict__ SX,
    const double* __restrict__ SY, const double* __restrict__ SR, const int32_t* __restrict__ SM, long store_rows,
    int store_no, int store_nc, const int32_t* __restrict__ index, const int32_t* __restrict__ col_src,
    const int32_t* __restrict__ row_src, int expect_tag, uint32_t warm_mask, double rho_cold, double* __restrict__ X,
    double* __restrict__ Y, double* __restrict__ Z, double* __restrict__ RHO, int32_t* __restrict__ WARM, int count,
    int ipw, int lpr) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tpi = WS_BLOCK / ipw;                 // threads of one instance: whole wavefronts
  const int local = threadIdx.x / tpi, t = threadIdx.x - local * tpi;
  const long inst = (long)blockIdx.x * ipw + local;
  const bool live = inst < count;
  double* xs = sm + (size_t)local * ws_slot(no, nc);
  double* ys = xs + ws_even(no);
  int* flag = reinterpret_cast<int*>(ys + ws_even(nc));

  // 1. the header
  long r = -1;
  bool head = false;
  double rho = rho_cold;
  if (live) {
    r = index ? (long)index[inst] : inst;
    if (r >= 0 && r < store_rows) {
      const int status = SM[2 * r], tag = SM[2 * r + 1];
      const int a = status < 0 ? -status : status;
      const double rv = SR[r];
      head = tag == expect_tag && a >= 0 && a < 32 && ((warm_mask >> a) & 1u) != 0 && rv >= 1e-6 && rv <= 1e6;
      if (head) rho = rv;   // (inside [1e-6, 1e6]: finite)
    }
  }
  if (t == 0) *flag = 0;
  __syncthreads();

  // 2. the gather
  if (head) {
    bool bad = false;
    for (int e = t; e < no; e += tpi) {
      const int s = col_src[e];
      const double v = (s >= 0 && s < store_no) ? SX[(size_t)r * store_no + s] : 0.0;
      bad = bad || !ws_finite(v);
      xs[e] = v;
    }
    for (int e = t; e < nc; e += tpi) {
      const int s = row_src[e];
      const double v = (s >= 0 && s < store_nc) ? SY[(size_t)r * store_nc + s] : 0.0;
      bad = bad || !ws_finite(v);
      ys[e] = v;
    }
    if (bad) atomicOr(flag, 1);
  }
  __syncthreads();
  if (!live) return;
  const bool warm = head && *flag == 0;

  // 3. the start
  double* xb = X + (size_t)inst * no;
  for (int e = t; e < no; e += tpi) xb[e] = warm ? xs[e] : 0.0;
  if (t == 0) {
    RHO[inst] = warm ? rho : rho_cold;
    WARM[inst] = warm ? 1 : 0;
  }
  if (nc == 0) return;
  double* yb = Y + (size_t)inst * nc;
  double* zb = Z + (size_t)inst * nc;
  const double* hb = h + (size_t)inst * nc;
  for (int e = t; e < nc; e += tpi) yb[e] = warm ? ys[e] : 0.0;
  if (!warm) {
    for (int e = t; e < nc; e += tpi) zb[e] = fmin(0.0, hb[e]);   // (what mpcasm_qp_solve(warm = 0) starts from)
    return;
  }
  const double* Gb = G + (size_t)inst * nc * no;
  const int wave = t >> 6, lane = t & 63, waves = tpi >> 6;
  const int side = 64 / lpr;                     // rows side by side in a wavefront
  const int sub = lane & (lpr - 1), rl = lane / lpr;
  for (int r0 = wave * side * WS_ROWS; r0 < nc; r0 += waves * side * WS_ROWS) {
    double acc[WS_ROWS];
#pragma unroll
    for (int u = 0; u < WS_ROWS; ++u) {
      acc[u] = 0.0;
      const int row = r0 + u * side + rl;
      if (row < nc) {
        const double* g = Gb + (size_t)row * no;
        if (VEC == 2) {
          double a1 = 0.0;
          for (int c = 2 * sub; c < no; c += 2 * lpr) {   // (no is even: c + 1 < no)
            const double2 gv = *reinterpret_cast<const double2*>(g + c);
            const double2 xv = *reinterpret_cast<const double2*>(xs + c);
            acc[u] = fma(gv.x, xv.x, acc[u]);
            a1 = fma(gv.y, xv.y, a1);
          }
          acc[u] += a1;
        } else {
          for (int c = sub; c < no; c += lpr) acc[u] = fma(g[c], xs[c], acc[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < WS_ROWS; ++u)
      for (int off = lpr >> 1; off > 0; off >>= 1) acc[u] += __shfl_xor(acc[u], off, 64);
#pragma unroll
    for (int u = 0; u < WS_ROWS; ++u) {
      const int row = r0 + u * side + rl;
      if (sub == 0 && row < nc) zb[row] = fmin(acc[u], hb[row]);
    }
  }
}

// instance b's x, y, rho, status and the launch's tag into row index[b] of the store, the padding zeroed; an
// index outside the store writes nothing
__global__ __launch_bounds__(WS_BLOCK) void warm_store_kernel(
    int no, int nc, const double* __restrict__ X, const double* __restrict__ Y, const double* __restrict__ RHO,
    const int32_t* __restrict__ status, int tag, double* __restrict__ SX, double* __restrict__ SY,
    double* __restrict__ SR, int32_t* __restrict__ SM, long store_rows, int store_no, int store_nc,
    const int32_t* __restrict__ index, int count, int ipw) {
  const int tpi = WS_BLOCK / ipw;
  const int local = threadIdx.x / tpi, t = threadIdx.x - local * tpi;
  const long inst = (long)blockIdx.x * ipw + local;
  if (inst >= count) return;
  const long r = index ? (long)index[inst] : inst;
  if (r < 0 || r >= store_rows) return;
  for (int e = t; e < store_no; e += tpi) SX[(size_t)r * store_no + e] = e < no ? X[(size_t)inst * no + e] : 0.0;
  for (int e = t; e < store_nc; e += tpi) SY[(size_t)r * store_nc + e] = e < nc ? Y[(size_t)inst * nc + e] : 0.0;
  if (t == 0) {
    SR[r] = RHO[inst];
    SM[2 * r] = status[inst];
    SM[2 * r + 1] = tag;
  }
}

// instances per workgroup: four (a wavefront each) up to 8 KB of G, two (two wavefronts each) up to 64 KB, else one.
// Measured at 4 096 instances of the biped's 36-wide bucket (22 KB of G): 36.8 / 31.6 / 45.5 us with 1 / 2 / 4 -- one
// wavefront alone walks an instance's rows in ten dependent passes.
// (MPCASM_QP_WARM_IPW = 1, 2 or 4, read at every call, overrides that: a tuning aid)
inline int ws_ipw(int no, int nc) {
  const char* env = getenv("MPCASM_QP_WARM_IPW");
  if (env != nullptr && (atoi(env) == 1 || atoi(env) == 2 || atoi(env) == 4)) return atoi(env);
  const long g = (long)no * nc;
  return g <= 1024 ? 4 : g <= 8192 ? 2 : 1;
}

}  // namespace

int launch_qp_warm_start(int no, int nc, const double* G, const double* h, const double* sx, const double* sy,
                         const double* srho, const int32_t* smeta, int64_t store_rows, int store_no, int store_nc,
                         const int32_t* index, const int32_t* col_src, const int32_t* row_src, int expect_tag,
                         uint32_t warm_mask, double rho_cold, double* x, double* y, double* z, double* rho,
                         int32_t* warm, int count, hipStream_t stream, hipError_t* err) {
  const int ipw = ws_ipw(no, nc);
  const size_t lds = (size_t)ipw * ws_slot(no, nc) * sizeof(double);   // (at most 20.5 KB: 512 + 2048 doubles)
  const bool vec2 = (no & 1) == 0 && (reinterpret_cast<uintptr_t>(G) & 15) == 0;
  const int per_lane = vec2 ? 2 : 1;
  const int lpr = no <= 16 * per_lane ? 16 : no <= 32 * per_lane ? 32 : 64;
  const unsigned grid = (unsigned)((count + ipw - 1) / ipw);
  return launch_with_lds(vec2 ? warm_start_kernel<2> : warm_start_kernel<1>, grid, WS_BLOCK, lds, stream, err, no, nc,
                         G, h, sx, sy, srho, smeta, (long)store_rows, store_no, store_nc, index, col_src, row_src,
                         expect_tag, warm_mask, rho_cold, x, y, z, rho, warm, count, ipw, lpr);
}

int launch_qp_warm_store(int no, int nc, const double* x, const double* y, const double* rho, const int32_t* status,
                         int tag, double* sx, double* sy, double* srho, int32_t* smeta, int64_t store_rows,
                         int store_no, int store_nc, const int32_t* index, int count, hipStream_t stream,
                         hipError_t* err) {
  const int ipw = store_no + store_nc <= 256 ? 4 : 1;
  const unsigned grid = (unsigned)((count + ipw - 1) / ipw);
  return launch_with_lds(warm_store_kernel, grid, WS_BLOCK, 0, stream, err, no, nc, x, y, rho, status, tag, sx, sy, srho,
                         smeta, (long)store_rows, store_no, store_nc, index, count, ipw);
}

}  // namespace mpcasm
