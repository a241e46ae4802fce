// polish_wide.hip -- K6 for QPs whose matrices do not fit in one workgroup's LDS (mpcasm_qp_polish_wide): the
// five steps of polish.hip -- skip, active set, regularised KKT solve with refinement against the K that is not
// regularised, the polished point, OSQP's rule and the sign test (include/mpcasm.h states them, and
// tests/polish_restatement.py restates them) -- with G and P read in place and the matrices of the solve in a
// workspace of the caller's, for the shapes mpcasm_qp_solve_wide was built for (C3, C5, C4).
//
// One workgroup of four wavefronts per instance, as admm_wide.hip; the launch has min(batch, POLISH_WIDE_CAP)
// workgroups, workgroup w takes the instances w, w + grid, ... and reuses its slice of the workspace, so the
// workspace grows with the workgroups and not with the batch.  The vectors of length no and nc, the partial sums
// and the list of active rows live in LDS (polish_wide_lds).  A slice holds three no x no matrices, row-major
// with leading dimension no:
//     M1 = (P + delta I)^-1          potrf, trtri, lauum in place and mirrored: admm_wide.hip's sequence, restated
//     M2 = Y = G_A M1                na <= no rows; row a is one symmetric product with row idx[a] of G
//     M3 = (Y G_A' + delta I)^-1     the Schur complement's lower triangle, inverted by the same three steps
// and a solve of (K + dK) [dx; dy] = [r1; r2] is four matrix-vector products, none a dependent chain longer than
// a row:   a = M1 r1;  w = Y r1 - r2;  dy = M3 w;  dx = a - Y' dy.
// The residuals read P and G from memory, a wavefront per row, four rows in flight (polish.hip's rows_times_x);
// G'y runs over the rows whose y is not zero.
//
// The workspace is written and read back by the same workgroup: its pointer is neither const nor restrict, and
// what this kernel wrote there is read only behind a workgroup barrier, with vector loads (the scalar cache does
// not see a vector store: admm_wide.hip's header).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "kernels.h"

namespace mpcasm {

namespace {

constexpr int PW_BLOCK = 256;
constexpr int PW_WAVES = PW_BLOCK / 64;
constexpr int PW_ROWS = 4;   // rows a wavefront keeps in flight
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
  L.pa = L.gx + nc;         // [PW_WAVES][no] partial sums; a wavefront's row of Y
  L.red = L.pa + PW_WAVES * no;   // 16 doubles: reductions and verdicts
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

// the larger of two, a NaN on either side kept (fmax drops it: a NaN must fail every comparison of the rule)
__device__ __forceinline__ double nmax(double a, double b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// A [n][lda], symmetric positive definite, its lower triangle read: A^-1 in place, both triangles (potrf: A = L L';
// trtri: L^-1 in place; lauum: A^-1 = L^-T L^-1 in place; the upper triangle mirrored) -- LAPACK's order, unblocked,
// a barrier per step.  rv: n doubles of LDS.  false when a pivot is not positive (a NaN among them): A is then
// not an inverse.  A may be memory this workgroup wrote: every read of it is behind a barrier.
__device__ inline bool spd_inverse(double* A, int n, int lda, double* rv, int tid, int lane, int wave) {
  __syncthreads();
  bool good = true;
  for (int k = 0; k < n; ++k) {
    const double dkk = A[(size_t)k * lda + k];
    good = good && dkk > 0.0;
    const double d = sqrt(dkk > 0.0 ? dkk : 1.0);
    __syncthreads();
    for (int i = k + tid; i < n; i += PW_BLOCK) {
      const double v = i == k ? d : A[(size_t)i * lda + k] / d;
      A[(size_t)i * lda + k] = v;
      rv[i] = v;
    }
    __syncthreads();
    for (int i = k + 1 + wave; i < n; i += PW_WAVES) {
      const double li = rv[i];
      for (int j = k + 1 + lane; j <= i; j += 64) A[(size_t)i * lda + j] = fma(-li, rv[j], A[(size_t)i * lda + j]);
    }
    __syncthreads();
  }
  if (!good) return false;   // (every thread read the same pivots)
  for (int j = n - 1; j >= 0; --j) {
    const double ljj = A[(size_t)j * lda + j];
    for (int i = j + 1 + tid; i < n; i += PW_BLOCK) rv[i] = A[(size_t)i * lda + j];
    __syncthreads();
    const double ajj = 1.0 / ljj;
    for (int i = j + 1 + wave; i < n; i += PW_WAVES) {
      double sacc = 0.0;
      for (int k = j + 1 + lane; k <= i; k += 64) sacc = fma(A[(size_t)i * lda + k], rv[k], sacc);
      sacc = wave_sum(sacc);
      if (lane == 0) A[(size_t)i * lda + j] = -ajj * sacc;
    }
    if (tid == 0) A[(size_t)j * lda + j] = ajj;
    __syncthreads();
  }
  for (int i = 0; i < n; ++i) {
    for (int k = i + tid; k < n; k += PW_BLOCK) rv[k] = A[(size_t)k * lda + i];
    __syncthreads();
    for (int b = tid; b <= i; b += PW_BLOCK) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      int k = i;
      for (; k + 4 <= n; k += 4) {
        s0 = fma(rv[k], A[(size_t)k * lda + b], s0);
        s1 = fma(rv[k + 1], A[(size_t)(k + 1) * lda + b], s1);
        s2 = fma(rv[k + 2], A[(size_t)(k + 2) * lda + b], s2);
        s3 = fma(rv[k + 3], A[(size_t)(k + 3) * lda + b], s3);
      }
      for (; k < n; ++k) s0 = fma(rv[k], A[(size_t)k * lda + b], s0);
      A[(size_t)i * lda + b] = (s0 + s1) + (s2 + s3);   // (only this thread reads (i, b))
    }
    __syncthreads();
  }
  for (int e = tid; e < n * n; e += PW_BLOCK) {
    const int a = e / n, b = e - a * n;
    if (b > a) A[(size_t)a * lda + b] = A[(size_t)b * lda + a];
  }
  __syncthreads();
  return true;
}

// out[r] = M[r] . x, r < rows, M [rows][lda] in memory, x [cols] in LDS: a wavefront takes four rows at a time, the
// lanes along them (polish.hip's rows_times_x)
__device__ __forceinline__ void rows_mv(const double* M, int lda, int rows, int cols, const double* x, double* out,
                                        int lane, int wave) {
  for (int r0 = wave * PW_ROWS; r0 < rows; r0 += PW_WAVES * PW_ROWS) {
    double acc[PW_ROWS];
#pragma unroll
    for (int u = 0; u < PW_ROWS; ++u) {
      acc[u] = 0.0;
      if (r0 + u < rows)
        for (int c = lane; c < cols; c += 64) acc[u] = fma(M[(size_t)(r0 + u) * lda + c], x[c], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < PW_ROWS; ++u) acc[u] = wave_sum(acc[u]);
#pragma unroll
    for (int u = 0; u < PW_ROWS; ++u)
      if (lane == 0 && r0 + u < rows) out[r0 + u] = acc[u];
  }
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
    for (; b + 3 * PW_WAVES < rows; b += 4 * PW_WAVES) {
      const double m0 = M[(size_t)b * lda + j], m1 = M[(size_t)(b + PW_WAVES) * lda + j];
      const double m2 = M[(size_t)(b + 2 * PW_WAVES) * lda + j], m3 = M[(size_t)(b + 3 * PW_WAVES) * lda + j];
      s0 = fma(m0, v[b], s0);
      s1 = fma(m1, v[b + PW_WAVES], s1);
      s2 = fma(m2, v[b + 2 * PW_WAVES], s2);
      s3 = fma(m3, v[b + 3 * PW_WAVES], s3);
    }
    for (; b < rows; b += PW_WAVES) s0 = fma(M[(size_t)b * lda + j], v[b], s0);
    pa[wave * lp + j] = (s0 + s1) + (s2 + s3);
  }
}
__device__ __forceinline__ double sum4(const double* pa, int lp, int c) {
  return (pa[c] + pa[lp + c]) + (pa[2 * lp + c] + pa[3 * lp + c]);
}

__global__ __launch_bounds__(PW_BLOCK) void polish_wide_kernel(
    int no, int nc, const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ G,
    const double* __restrict__ h, double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Z,
    const int32_t* __restrict__ status, double delta, int refine_iters, int32_t* __restrict__ polish,
    double* __restrict__ res, int batch, double* work, long slice) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const PolishWideLds L = polish_wide_lds(no, nc);
  double* xs = sm + L.x;
  double* ya = sm + L.ya;
  double* r1 = sm + L.r1;
  double* r2 = sm + L.r2;
  double* us = sm + L.u;
  double* ws = sm + L.w;
  double* ss = sm + L.s;
  double* qs = sm + L.q;
  double* ds = sm + L.d;
  double* rv = sm + L.rv;
  double* hs = sm + L.h;
  double* ys = sm + L.y;
  double* zs = sm + L.z;
  double* gx = sm + L.gx;
  double* pa = sm + L.pa;
  double* red = sm + L.red;
  int* idx = reinterpret_cast<int*>(sm + L.idx);
  double* M1 = work + (size_t)blockIdx.x * slice;
  double* Ym = M1 + (size_t)no * no;
  double* M3 = Ym + (size_t)no * no;

  // one instance; the verdict, the same in every thread
  auto one = [&](long inst) -> int {
    // (an instance that is not solved is not read at all: a NON_CVX one holds NaN)
    if (status != nullptr && status[inst] != MPCASM_QP_SOLVED) return MPCASM_POLISH_SKIPPED;
    const double* Pb = P + (size_t)inst * no * no;
    const double* Gb = G + (size_t)inst * nc * no;
    double* Xb = X + (size_t)inst * no;
    double* Yb = Y + (size_t)inst * nc;
    double* Zb = Z + (size_t)inst * nc;
    for (int e = tid; e < no; e += PW_BLOCK) {
      qs[e] = q[(size_t)inst * no + e];
      xs[e] = Xb[e];
    }
    for (int e = tid; e < nc; e += PW_BLOCK) {
      hs[e] = h[(size_t)inst * nc + e];
      ys[e] = Yb[e];
      zs[e] = Zb[e];
    }
    __syncthreads();

    // ---- the active set: OSQP's test, the rows kept in ascending order (one wavefront, 64 rows a pass) ------
    if (wave == 0) {
      int count = 0;
      for (int base = 0; base < nc; base += 64) {
        const int r = base + lane;
        const bool act = r < nc && hs[r] - zs[r] < ys[r];
        const unsigned long long mask = __ballot(act);
        const int pos = count + __popcll(mask & ((1ull << lane) - 1ull));
        if (act && pos < no) idx[pos] = r;
        count += __popcll(mask);
      }
      if (lane == 0) red[15] = (double)count;
    }
    __syncthreads();
    const int na = (int)red[15];
    if (na > no) return MPCASM_POLISH_SKIPPED;   // (more active rows than unknowns: no KKT system of full rank)

    // |G x - z|_inf (zv == nullptr: |G x - min(G x, h)|_inf) and |P x + q + G'y|_inf of xs and the y in ys, both
    // kept in gx and ds; G'y cut over the wavefronts by rows, a lane a column, the rows whose y is 0 not read
    auto residuals = [&](const double* zv, double* rp_out, double* rd_out) {
      rows_mv(Gb, no, nc, no, xs, gx, lane, wave);
      rows_mv(Pb, no, no, no, xs, ds, lane, wave);
      for (int c = lane; c < no; c += 64) {
        double s0 = 0.0, s1 = 0.0;
        int r = wave;
        for (; r + PW_WAVES < nc; r += 2 * PW_WAVES) {
          const double y0 = ys[r], y1 = ys[r + PW_WAVES];
          if (y0 != 0.0) s0 = fma(Gb[(size_t)r * no + c], y0, s0);
          if (y1 != 0.0) s1 = fma(Gb[(size_t)(r + PW_WAVES) * no + c], y1, s1);
        }
        if (r < nc && ys[r] != 0.0) s0 = fma(Gb[(size_t)r * no + c], ys[r], s0);
        pa[wave * no + c] = s0 + s1;
      }
      __syncthreads();
      double rp = 0.0, rd = 0.0;
      for (int c = tid; c < no; c += PW_BLOCK) {
        const double dv = (ds[c] + qs[c]) + sum4(pa, no, c);
        ds[c] = dv;
        rd = nmax(rd, fabs(dv));
      }
      for (int r = tid; r < nc; r += PW_BLOCK)
        rp = nmax(rp, fabs(gx[r] - (zv != nullptr ? zv[r] : fmin(gx[r], hs[r]))));
      for (int off = 32; off > 0; off >>= 1) {
        rp = nmax(rp, __shfl_xor(rp, off, 64));
        rd = nmax(rd, __shfl_xor(rd, off, 64));
      }
      if (lane == 0) {
        red[wave] = rp;
        red[PW_WAVES + wave] = rd;
      }
      __syncthreads();
      *rp_out = nmax(nmax(red[0], red[1]), nmax(red[2], red[3]));
      *rd_out = nmax(nmax(red[4], red[5]), nmax(red[6], red[7]));
      __syncthreads();   // (red and pa are free again)
    };

    // ---- r_p, r_d of the iterate passed in ---------------------------------------------------------------
    double rp_in, rd_in;
    residuals(zs, &rp_in, &rd_in);

    // ---- M1 = (P + delta I)^-1 ---------------------------------------------------------------------------------
    for (int e = tid; e < no * no; e += PW_BLOCK) {
      const int a = e / no, b = e - a * no;
      M1[e] = Pb[e] + (a == b ? delta : 0.0);
    }
    if (!spd_inverse(M1, no, no, rv, tid, lane, wave)) return MPCASM_POLISH_REJECTED;

    // ---- Y = G_A M1: wavefront w forms the rows a = w + 4 t, four at a time over one sweep of M1's rows; the
    // entries of G's rows are the same in every lane ------------------------------------------------------------
    for (int a0 = wave; a0 < na; a0 += PW_WAVES * 4) {
      const double* g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int a = a0 + PW_WAVES * u;
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
          const int a = a0 + PW_WAVES * u;
          if (a < na && j < no) Ym[(size_t)a * no + j] = acc[u];
        }
      }
    }
    __syncthreads();
    // ---- the lower triangle of S = Y G_A' + delta I: a wavefront a row a, its row of Y in LDS, four rows of G_A
    // in flight ------------------------------------------------------------------------------------------------
    for (int a = wave; a < na; a += PW_WAVES) {
      double* yr = pa + wave * no;
      for (int c = lane; c < no; c += 64) yr[c] = Ym[(size_t)a * no + c];
      for (int b0 = 0; b0 <= a; b0 += PW_ROWS) {
        double acc[PW_ROWS];
#pragma unroll
        for (int u = 0; u < PW_ROWS; ++u) {
          acc[u] = 0.0;
          if (b0 + u <= a) {
            const double* gr = Gb + (size_t)idx[b0 + u] * no;
            for (int c = lane; c < no; c += 64) acc[u] = fma(gr[c], yr[c], acc[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < PW_ROWS; ++u) acc[u] = wave_sum(acc[u]);
#pragma unroll
        for (int u = 0; u < PW_ROWS; ++u)
          if (lane == 0 && b0 + u <= a) M3[(size_t)a * no + b0 + u] = acc[u] + (b0 + u == a ? delta : 0.0);
      }
    }
    if (!spd_inverse(M3, na, no, rv, tid, lane, wave)) return MPCASM_POLISH_REJECTED;

    // (K + dK) [dx; dy] = [r1; r2]: dx in us, dy in ss
    auto kkt_solve = [&]() {
      cols_mv(M1, no, no, no, r1, pa, no, lane, wave);
      rows_mv(Ym, no, na, no, r1, ws, lane, wave);
      __syncthreads();
      for (int c = tid; c < no; c += PW_BLOCK) us[c] = sum4(pa, no, c);            // a = M1 r1
      for (int a = tid; a < na; a += PW_BLOCK) ws[a] -= r2[a];                     // w = Y r1 - r2
      __syncthreads();
      cols_mv(M3, no, na, na, ws, pa, no, lane, wave);
      __syncthreads();
      for (int a = tid; a < na; a += PW_BLOCK) ss[a] = sum4(pa, no, a);            // dy = M3 w
      __syncthreads();
      cols_mv(Ym, no, na, no, ss, pa, no, lane, wave);
      __syncthreads();
      for (int c = tid; c < no; c += PW_BLOCK) us[c] -= sum4(pa, no, c);           // dx = a - Y' dy
      __syncthreads();
    };

    // ---- t0 = (K + dK)^-1 g, then the refinement against the K that is not regularised -------------------------
    for (int c = tid; c < no; c += PW_BLOCK) r1[c] = -qs[c];
    for (int a = tid; a < na; a += PW_BLOCK) r2[a] = hs[idx[a]];
    __syncthreads();
    kkt_solve();
    for (int c = tid; c < no; c += PW_BLOCK) xs[c] = us[c];
    for (int r = tid; r < nc; r += PW_BLOCK) ys[r] = 0.0;
    __syncthreads();
    for (int a = tid; a < na; a += PW_BLOCK) {
      ya[a] = ss[a];
      ys[idx[a]] = ss[a];
    }
    __syncthreads();
    double rp_hat, rd_hat;
    for (int it = 0; it < refine_iters; ++it) {
      residuals(nullptr, &rp_hat, &rd_hat);   // (gx = G x^ and ds = P x^ + q + G'y^ are what the step needs)
      for (int c = tid; c < no; c += PW_BLOCK) r1[c] = -ds[c];
      for (int a = tid; a < na; a += PW_BLOCK) r2[a] = hs[idx[a]] - gx[idx[a]];
      __syncthreads();
      kkt_solve();
      for (int c = tid; c < no; c += PW_BLOCK) xs[c] += us[c];
      for (int a = tid; a < na; a += PW_BLOCK) {
        const double yn = ya[a] + ss[a];
        ya[a] = yn;
        ys[idx[a]] = yn;
      }
      __syncthreads();
    }

    // ---- the polished point and the verdict --------------------------------------------------------------
    residuals(nullptr, &rp_hat, &rd_hat);
    double neg = 0.0;
    for (int a = tid; a < na; a += PW_BLOCK) neg = ya[a] >= 0.0 ? neg : 1.0;   // (a NaN counts as negative)
    for (int off = 32; off > 0; off >>= 1) neg = fmax(neg, __shfl_xor(neg, off, 64));
    if (lane == 0) red[8 + wave] = neg;
    __syncthreads();
    const bool signs = red[8] == 0.0 && red[9] == 0.0 && red[10] == 0.0 && red[11] == 0.0;
    const bool better = (rp_hat < rp_in && rd_hat < rd_in) || (rp_hat < rp_in && rd_in < 1e-10) ||
                        (rd_hat < rd_in && rp_in < 1e-10);
    if (!(better && signs)) return MPCASM_POLISH_REJECTED;
    for (int c = tid; c < no; c += PW_BLOCK) Xb[c] = xs[c];
    for (int r = tid; r < nc; r += PW_BLOCK) {
      Yb[r] = ys[r];
      Zb[r] = fmin(gx[r], hs[r]);
    }
    if (tid == 0 && res != nullptr) {
      res[inst * 2 + 0] = rp_hat;
      res[inst * 2 + 1] = rd_hat;
    }
    return MPCASM_POLISH_DONE;
  };

  for (long inst = blockIdx.x; inst < batch; inst += gridDim.x) {
    const int verdict = one(inst);
    if (tid == 0) polish[inst] = verdict;
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

int launch_qp_polish_wide(int no, int nc, const double* P, const double* q, const double* G, const double* h,
                          double* x, double* y, double* z, const int32_t* status, double delta, int refine_iters,
                          int32_t* polish, double* res, int batch, double* work, hipStream_t stream,
                          hipError_t* err) {
  int64_t lds = 0;
  int32_t grid = 0;
  const int rc = qp_polish_wide_info(no, nc, batch, &lds, nullptr, &grid);
  if (rc != MPCASM_OK) return rc;
  if (lds > 64 * 1024) {
    *err = allow_whole_lds(reinterpret_cast<const void*>(polish_wide_kernel));
    if (*err != hipSuccess) return MPCASM_ERR_HIP;
  }
  hipLaunchKernelGGL(polish_wide_kernel, dim3((unsigned)grid), dim3(PW_BLOCK), (size_t)lds, stream, no, nc, P, q, G,
                     h, x, y, z, status, delta, refine_iters, polish, res, batch, work, polish_wide_slice(no));
  *err = hipGetLastError();
  return *err == hipSuccess ? MPCASM_OK : MPCASM_ERR_HIP;
}

}  // namespace mpcasm
