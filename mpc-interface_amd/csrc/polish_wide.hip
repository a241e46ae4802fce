// polish_wide.hip -- K6 for QPs whose matrices do not fit in one workgroup's LDS (mpcasm_qp_polish_wide): the
// five steps of polish.hip (polish_core.h has them, once) -- skip, active set, regularised KKT solve with refinement against the K that is not
// regularised, the polished point, OSQP's rule and the sign test (include/mpcasm.h states them, and
// tests/polish_restatement.py restates them) -- with G and P read in place and the matrices of the solve in a
// workspace of the caller's, for the shapes mpcasm_qp_solve_wide was built for (C3, C5, C4).
//
// One workgroup of four wavefronts per instance, as admm_wide.hip; the launch has min(batch, POLISH_WIDE_CAP)
// workgroups, workgroup w takes the instances w, w + grid, ... and reuses its slice of the workspace, so the
// workspace grows with the workgroups and not with the batch.  The vectors of length no and nc, the partial sums
// and the list of active rows live in LDS (polish_wide_lds).  A slice holds three no x no matrices, row-major
// with leading dimension no:
//     M1 = (P + delta I)^-1          potrf, trtri, lauum in place and mirrored: spd_inverse, admm_wide.hip's sequence
//     M2 = Y = G_A M1                na <= no rows; row a is one symmetric product with row idx[a] of G
//     M3 = (Y G_A' + delta I)^-1     the Schur complement's lower triangle, inverted by the same three steps
// and a solve of (K + dK) [dx; dy] = [r1; r2] is four matrix-vector products, none a dependent chain longer than
// a row:   a = M1 r1;  w = Y r1 - r2;  dy = M3 w;  dx = a - Y' dy.
// The residuals read P and G from memory, a wavefront per row, four rows in flight (qp_prims.h's rows_mv);
// G'y runs over the rows whose y is not zero.
//
// The workspace is written and read back by the same workgroup: its pointer is neither const nor restrict, and
// what this kernel wrote there is read only behind a workgroup barrier, with vector loads (the scalar cache does
// not see a vector store: admm_wide.hip's header).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "kernels.h"
#include "polish_core.h"
#include "sens_core.h"

namespace mpcasm {

namespace {

constexpr int PW_MAX_NO = 512;

struct PolishWideLds {
  int x, ya, r1, r2, u, w, s, q, d, rv, h, y, z, gx, pa, red, idx, total;
};
__host__ __device__ inline PolishWideLds polish_wide_lds(int no, int nc) {
  PolishWideLds L;
  L.x = 0;                  // x^ (first: the iterate's x)
  L.ya = L.x + no;          // y^ on the active rows, compact
  L.r1 = L.ya + no;
  L.r2 = L.r1 + no;
  L.u = L.r2 + no;          // a, then dx
  L.w = L.u + no;
  L.s = L.w + no;           // dy
  L.q = L.s + no;
  L.d = L.q + no;           // P x + q + G'y
  L.rv = L.d + no;          // the factorisations' column
  L.h = L.rv + no;
  L.y = L.h + nc;           // the iterate's y, then y^ on all rows
  L.z = L.y + nc;           // the iterate's z
  L.gx = L.z + nc;          // G x
  L.pa = L.gx + nc;         // [QP_WAVES][no] partial sums; a wavefront's row of Y
  L.red = L.pa + QP_WAVES * no;   // 16 doubles: reductions and verdicts
  L.idx = L.red + 16;       // no int32: the active rows, ascending
  L.total = L.idx + (no + 1) / 2;
  L.total += L.total & 1;
  return L;
}
// doubles of one workgroup's slice: three matrices, even (every slice starts on 16 bytes)
__host__ __device__ inline long polish_wide_slice(int no) {
  const long s = 3L * no * no;
  return s + (s & 1);
}

// wavefront `wave`'s quarter of out = M'v, M [rows][lda] in memory (symmetric M: of M v), v [rows] in LDS:
// pa[wave][j], j < cols, over the rows wave, wave + 4, ...; a lane a column, four rows in flight
__device__ __forceinline__ void cols_mv(const double* M, int lda, int rows, int cols, const double* v, double* pa,
                                        int lp, int lane, int wave) {
  for (int c0 = 0; c0 < cols; c0 += 64) {
    const int j = c0 + lane;
    if (j >= cols) continue;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int b = wave;
    for (; b + 3 * QP_WAVES < rows; b += 4 * QP_WAVES) {
      const double m0 = M[(size_t)b * lda + j], m1 = M[(size_t)(b + QP_WAVES) * lda + j];
      const double m2 = M[(size_t)(b + 2 * QP_WAVES) * lda + j], m3 = M[(size_t)(b + 3 * QP_WAVES) * lda + j];
      s0 = fma(m0, v[b], s0);
      s1 = fma(m1, v[b + QP_WAVES], s1);
      s2 = fma(m2, v[b + 2 * QP_WAVES], s2);
      s3 = fma(m3, v[b + 3 * QP_WAVES], s3);
    }
    for (; b < rows; b += QP_WAVES) s0 = fma(M[(size_t)b * lda + j], v[b], s0);
    pa[wave * lp + j] = (s0 + s1) + (s2 + s3);
  }
}

// polish_core.h's backend with G and P read in place: the three matrices of a workgroup's slice of the workspace
// and the four-product solve
struct SlicePolish {
  PolishVecs v;
  double *M1, *Ym, *M3, *ws, *rv;
  int no, tid, lane, wave;
  double delta;

  __device__ __forceinline__ SlicePolish(double* sm, double* slice, int no_, int nc, double delta_, int tid_, int lane_,
                                         int wave_)
      : no(no_), tid(tid_), lane(lane_), wave(wave_), delta(delta_) {
    const PolishWideLds L = polish_wide_lds(no, nc);
    M1 = slice, Ym = M1 + (size_t)no * no, M3 = Ym + (size_t)no * no, ws = sm + L.w, rv = sm + L.rv;
    v = PolishVecs{sm + L.x, sm + L.ya, sm + L.r1, sm + L.r2, sm + L.u,  sm + L.s,  sm + L.q,  sm + L.d,
                   sm + L.h, sm + L.y,  sm + L.z,  sm + L.gx, sm + L.pa, sm + L.red, reinterpret_cast<int*>(sm + L.idx)};
  }

  __device__ __forceinline__ bool build(const double* Pb, const double* Gb, int na) {
    const int* idx = v.idx;
    double* pa = v.pa;
    // ---- M1 = (P + delta I)^-1 ---------------------------------------------------------------------------------
    for (int e = tid; e < no * no; e += QP_BLOCK) {
      const int a = e / no, b = e - a * no;
      M1[e] = Pb[e] + (a == b ? delta : 0.0);
    }
    if (!spd_inverse(M1, no, no, rv, tid, lane, wave)) return false;

    // ---- Y = G_A M1: wavefront w forms the rows a = w + 4 t, four at a time over one sweep of M1's rows; the
    // entries of G's rows are the same in every lane ------------------------------------------------------------
    for (int a0 = wave; a0 < na; a0 += QP_WAVES * 4) {
      const double* g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int a = a0 + QP_WAVES * u;
        g[u] = Gb + (size_t)__builtin_amdgcn_readfirstlane(idx[a < na ? a : a0]) * no;   // (past na: row a0 again, dropped)
      }
      for (int c0 = 0; c0 < no; c0 += 64) {
        const int j = c0 + lane;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = 0; b < no; ++b) {
          const double m = j < no ? M1[(size_t)b * no + j] : 0.0;
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[u] = fma(g[u][b], m, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int a = a0 + QP_WAVES * u;
          if (a < na && j < no) Ym[(size_t)a * no + j] = acc[u];
        }
      }
    }
    __syncthreads();
    // ---- the lower triangle of S = Y G_A' + delta I: a wavefront a row a, its row of Y in LDS, four rows of G_A
    // in flight ------------------------------------------------------------------------------------------------
    for (int a = wave; a < na; a += QP_WAVES) {
      double* yr = pa + wave * no;
      for (int c = lane; c < no; c += 64) yr[c] = Ym[(size_t)a * no + c];
      for (int b0 = 0; b0 <= a; b0 += QP_ROWS) {
        double acc[QP_ROWS];
#pragma unroll
        for (int u = 0; u < QP_ROWS; ++u) {
          acc[u] = 0.0;
          if (b0 + u <= a) {
            const double* gr = Gb + (size_t)idx[b0 + u] * no;
            for (int c = lane; c < no; c += 64) acc[u] = fma(gr[c], yr[c], acc[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < QP_ROWS; ++u) acc[u] = wave_sum(acc[u]);
#pragma unroll
        for (int u = 0; u < QP_ROWS; ++u)
          if (lane == 0 && b0 + u <= a) M3[(size_t)a * no + b0 + u] = acc[u] + (b0 + u == a ? delta : 0.0);
      }
    }
    return spd_inverse(M3, na, no, rv, tid, lane, wave);
  }

  // a = M1 r1;  w = Y r1 - r2;  dy = M3 w;  dx = a - Y' dy
  __device__ __forceinline__ void kkt_solve(int na) {
    const double *r1 = v.r1, *r2 = v.r2;
    double *us = v.dx, *ss = v.dy, *pa = v.pa;
    cols_mv(M1, no, no, no, r1, pa, no, lane, wave);
    rows_mv(Ym, no, na, no, r1, ws, lane, wave);
    __syncthreads();
    for (int c = tid; c < no; c += QP_BLOCK) us[c] = sum4(pa, no, c);            // a = M1 r1
    for (int a = tid; a < na; a += QP_BLOCK) ws[a] -= r2[a];                     // w = Y r1 - r2
    __syncthreads();
    cols_mv(M3, no, na, na, ws, pa, no, lane, wave);
    __syncthreads();
    for (int a = tid; a < na; a += QP_BLOCK) ss[a] = sum4(pa, no, a);            // dy = M3 w
    __syncthreads();
    cols_mv(Ym, no, na, no, ss, pa, no, lane, wave);
    __syncthreads();
    for (int c = tid; c < no; c += QP_BLOCK) us[c] -= sum4(pa, no, c);           // dx = a - Y' dy
    __syncthreads();
  }
};

__global__ __launch_bounds__(QP_BLOCK) void polish_wide_kernel(
    int no, int nc, const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ G,
    const double* __restrict__ h, double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Z,
    const int32_t* __restrict__ status, double delta, int refine_iters, int32_t* __restrict__ polish,
    double* __restrict__ res, int batch, double* work, long slice) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  SlicePolish be(sm, work + (size_t)blockIdx.x * slice, no, nc, delta, tid, lane, wave);
  for (long inst = blockIdx.x; inst < batch; inst += gridDim.x) {
    const int verdict = polish_instance(be, inst, no, nc, P, q, G, h, X, Y, Z, status, refine_iters, res, tid, lane, wave);
    if (tid == 0) polish[inst] = verdict;
    __syncthreads();   // (the next instance writes the LDS and the slice this one may still be reading)
  }
}

// mpcasm_qp_sens_wide: sens_core.h's steps on the same back-end, the same slices and the same geometry
__global__ __launch_bounds__(QP_BLOCK) void sens_wide_kernel(QpSens s, double* work, long slice) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  SlicePolish be(sm, work + (size_t)blockIdx.x * slice, s.no, s.nc, s.delta, tid, lane, wave);
  for (long inst = blockIdx.x; inst < s.batch; inst += gridDim.x) {
    const int verdict = sens_instance(be, inst, s, tid, lane, wave);
    if (tid == 0) s.verdict[inst] = verdict;
    __syncthreads();   // (the next instance writes the LDS and the slice this one may still be reading)
  }
}

}  // namespace

int qp_polish_wide_info(int no, int nc, int batch, int64_t* lds_bytes, int64_t* work_bytes, int32_t* workgroups) {
  const size_t lds = (size_t)polish_wide_lds(no, nc).total * sizeof(double);
  // (MPCASM_QP_POLISH_WIDE_GROUPS, read at every call: fewer workgroups than the cap, a tuning aid)
  int cap = POLISH_WIDE_CAP;
  const char* env = getenv("MPCASM_QP_POLISH_WIDE_GROUPS");
  if (env != nullptr && atoi(env) >= 1 && atoi(env) < cap) cap = atoi(env);
  const int grid = batch < cap ? batch : cap;
  if (lds_bytes) *lds_bytes = (int64_t)lds;
  if (work_bytes) *work_bytes = (int64_t)grid * polish_wide_slice(no) * (int64_t)sizeof(double);
  if (workgroups) *workgroups = grid;
  return no > PW_MAX_NO || lds > (size_t)RESIDENT_LDS_LIMIT ? MPCASM_ERR_LIMIT : MPCASM_OK;
}

int launch_qp_polish_wide(const QpBatch& b, const QpPolish& p, double* work, hipStream_t stream, hipError_t* err) {
  int64_t lds = 0;
  int32_t grid = 0;
  const int rc = qp_polish_wide_info(b.no, b.nc, b.batch, &lds, nullptr, &grid);
  if (rc != MPCASM_OK) return rc;
  return launch_with_lds(polish_wide_kernel, (unsigned)grid, QP_BLOCK, (size_t)lds, stream, err, b.no, b.nc, b.P, b.q,
                         b.G, b.h, b.x, b.y, b.z, p.status, p.delta, p.refine_iters, p.polish, p.res, b.batch, work,
                         polish_wide_slice(b.no));
}

int launch_qp_sens_wide(const QpSens& s, double* work, hipStream_t stream, hipError_t* err) {
  int64_t lds = 0;
  int32_t grid = 0;
  const int rc = qp_polish_wide_info(s.no, s.nc, s.batch, &lds, nullptr, &grid);
  if (rc != MPCASM_OK) return rc;
  return launch_with_lds(sens_wide_kernel, (unsigned)grid, QP_BLOCK, (size_t)lds, stream, err, s, work,
                         polish_wide_slice(s.no));
}

}  // namespace mpcasm
