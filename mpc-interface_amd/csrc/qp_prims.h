// qp_prims.h -- what the four QP solver kernels (admm.hip, admm_wide.hip, polish.hip, polish_wide.hip) share on the
// device, each piece written once: the reductions, the two strided inner products, rows of a matrix in memory times
// a vector, OSQP's verdict and step (the two solves), and the two factorisations of the two polishes (in LDS with an
// explicit L^-1; in place, LAPACK's order).  Every sum here has a fixed order -- the tests hold the kernels to
// restatements in the same order -- so a caller that needs another order keeps its own loop.  The two solves keep
// the same factorisations written into their kernels (admm.hip's `factor`, admm_wide.hip's `factor`): called from
// here they compiled to other code, and the solves measured 0.4 to 1.2 % slower.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_prims.h"
#include "kernels.h"

namespace mpcasm {

// one workgroup of four wavefronts per instance, in all four kernels
constexpr int QP_BLOCK = 256;
constexpr int QP_WAVES = QP_BLOCK / 64;

// ---- reductions over the 64 lanes of a wavefront, the result in every lane (wave_sum: device_prims.h) -----------
__device__ __forceinline__ double wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
// the larger of two, a NaN on either side kept (fmax drops it: a NaN must fail every comparison of the polish's rule)
__device__ __forceinline__ double nmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double wave_nmax(double v) {
  for (int off = 32; off > 0; off >>= 1) v = nmax(v, __shfl_xor(v, off, 64));
  return v;
}
// the four wavefronts' partial sums pa[w][c], rows lp apart
__device__ __forceinline__ double sum4(const double* pa, int lp, int c) {
  return (pa[c] + pa[lp + c]) + (pa[2 * lp + c] + pa[3 * lp + c]);
}

// ---- sum_i a[i sa] b[i sb], i < n ------------------------------------------------------------------------------------
// dot4: four sums side by side, eight pairs of reads in flight -- the loop must not be one dependent chain of
// read -> fma
__device__ __forceinline__ double dot4(const double* a, int sa, const double* b, int sb, int n, double init) {
  double s0 = init, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    double av[8], bv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) av[u] = a[(i + u) * sa], bv[u] = b[(i + u) * sb];
    s0 = fma(av[0], bv[0], s0);
    s1 = fma(av[1], bv[1], s1);
    s2 = fma(av[2], bv[2], s2);
    s3 = fma(av[3], bv[3], s3);
    s0 = fma(av[4], bv[4], s0);
    s1 = fma(av[5], bv[5], s1);
    s2 = fma(av[6], bv[6], s2);
    s3 = fma(av[7], bv[7], s3);
  }
  for (; i + 4 <= n; i += 4) {
    const double a0 = a[i * sa], a1 = a[(i + 1) * sa], a2 = a[(i + 2) * sa], a3 = a[(i + 3) * sa];
    const double b0 = b[i * sb], b1 = b[(i + 1) * sb], b2 = b[(i + 2) * sb], b3 = b[(i + 3) * sb];
    s0 = fma(a0, b0, s0);
    s1 = fma(a1, b1, s1);
    s2 = fma(a2, b2, s2);
    s3 = fma(a3, b3, s3);
  }
  for (; i < n; ++i) s0 = fma(a[i * sa], b[i * sb], s0);
  return (s0 + s1) + (s2 + s3);
}
// pdot: the same four sums, half as deep (the polish's sums are short).  The two differ in the order of their terms
// once n reaches 8: a caller keeps the one it has.
__device__ __forceinline__ double pdot(const double* a, int sa, const double* b, int sb, int n) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    const double a0 = a[i * sa], a1 = a[(i + 1) * sa], a2 = a[(i + 2) * sa], a3 = a[(i + 3) * sa];
    const double b0 = b[i * sb], b1 = b[(i + 1) * sb], b2 = b[(i + 2) * sb], b3 = b[(i + 3) * sb];
    s0 = fma(a0, b0, s0);
    s1 = fma(a1, b1, s1);
    s2 = fma(a2, b2, s2);
    s3 = fma(a3, b3, s3);
  }
  for (; i < n; ++i) s0 = fma(a[i * sa], b[i * sb], s0);
  return (s0 + s1) + (s2 + s3);
}

// out[r] = M[r] . x, r < rows, M [rows][lda] in memory, x [cols] in LDS: a wavefront takes four rows at a time, the
// lanes along them, so that four rows' loads are in flight before the first sum is reduced (one row at a time was
// one memory latency a row)
constexpr int QP_ROWS = 4;
__device__ __forceinline__ void rows_mv(const double* M, int lda, int rows, int cols, const double* x, double* out,
                                        int lane, int wave) {
  for (int r0 = wave * QP_ROWS; r0 < rows; r0 += QP_WAVES * QP_ROWS) {
    double acc[QP_ROWS];
#pragma unroll
    for (int u = 0; u < QP_ROWS; ++u) {
      acc[u] = 0.0;
      if (r0 + u < rows)
        for (int c = lane; c < cols; c += 64) acc[u] = fma(M[(size_t)(r0 + u) * lda + c], x[c], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < QP_ROWS; ++u) acc[u] = wave_sum(acc[u]);
#pragma unroll
    for (int u = 0; u < QP_ROWS; ++u)
      if (lane == 0 && r0 + u < rows) out[r0 + u] = acc[u];
  }
}

// ---- matrices in LDS: Cholesky in place, the factor inverted beside it -------------------------------------------
// Cholesky in place of the lower triangle of M [n][ld]; false when a pivot is not positive (a NaN among them)
__device__ inline bool cholesky_lds(double* M, int n, int ld, int tid, int lane, int wave) {
  bool good = true;
  for (int k = 0; k < n; ++k) {
    const double dkk = M[k * ld + k];
    good = good && dkk > 0.0;
    const double d = sqrt(dkk > 0.0 ? dkk : 1.0);
    __syncthreads();
    for (int i = k + tid; i < n; i += QP_BLOCK) M[i * ld + k] = i == k ? d : M[i * ld + k] / d;
    __syncthreads();
    // the trailing block: wavefront w takes the rows k + 1 + w, + 4, ..., a lane the column k + 1 + lane
    // (+ 64, ... for more unknowns than lanes) up to the diagonal
    for (int j = k + 1 + lane; j < n; j += 64) {
      const double ljk = M[j * ld + k];
      for (int i = k + 1 + wave + (j > k + 1 + wave ? ((j - k - 1 - wave + QP_WAVES - 1) / QP_WAVES) * QP_WAVES : 0);
           i < n; i += QP_WAVES)
        M[i * ld + j] = fma(-M[i * ld + k], ljk, M[i * ld + j]);
    }
    __syncthreads();
  }
  return good;
}

// T [n][ld] = L^-1: thread c solves L t = e_c (rows above c are zero), its sums pdot's
__device__ inline void invert_lower_lds(const double* Lm, double* T, int n, int ld, int tid) {
  for (int c = tid; c < n; c += QP_BLOCK)
    for (int i = 0; i < n; ++i) {
      const double sv = (i == c ? 1.0 : 0.0) - (i > c ? pdot(Lm + i * ld + c, 1, T + c * ld + c, ld, i - c) : 0.0);
      T[i * ld + c] = i < c ? 0.0 : sv / Lm[i * ld + i];
    }
  __syncthreads();
}

// ---- a matrix in LDS or in memory: the inverse in place ---------------------------------------------------------------
// A [n][lda], symmetric positive definite, its lower triangle read: A^-1 in place, both triangles (potrf: A = L L';
// trtri: L^-1 in place; lauum: A^-1 = L^-T L^-1 in place; the upper triangle mirrored) -- LAPACK's order, unblocked,
// a barrier per step.  rv: n doubles of LDS.  false as soon as the factorisation has met a pivot that is not positive
// (a NaN among them): A is then not an inverse, and what it holds is the caller's to overwrite.  A may be memory
// this workgroup wrote: every read of it is behind a barrier, with vector loads.
__device__ inline bool spd_inverse(double* A, int n, int lda, double* rv, int tid, int lane, int wave) {
  __syncthreads();
  bool good = true;
  for (int k = 0; k < n; ++k) {
    const double dkk = A[(size_t)k * lda + k];
    good = good && dkk > 0.0;
    const double d = sqrt(dkk > 0.0 ? dkk : 1.0);
    __syncthreads();
    for (int i = k + tid; i < n; i += QP_BLOCK) {
      const double v = i == k ? d : A[(size_t)i * lda + k] / d;
      A[(size_t)i * lda + k] = v;
      rv[i] = v;
    }
    __syncthreads();
    for (int i = k + 1 + wave; i < n; i += QP_WAVES) {
      const double li = rv[i];
      for (int j = k + 1 + lane; j <= i; j += 64) A[(size_t)i * lda + j] = fma(-li, rv[j], A[(size_t)i * lda + j]);
    }
    __syncthreads();
  }
  if (!good) return false;   // (every thread read the same pivots)
  for (int j = n - 1; j >= 0; --j) {
    const double ljj = A[(size_t)j * lda + j];
    for (int i = j + 1 + tid; i < n; i += QP_BLOCK) rv[i] = A[(size_t)i * lda + j];
    __syncthreads();
    const double ajj = 1.0 / ljj;
    for (int i = j + 1 + wave; i < n; i += QP_WAVES) {
      double sacc = 0.0;
      for (int k = j + 1 + lane; k <= i; k += 64) sacc = fma(A[(size_t)i * lda + k], rv[k], sacc);
      sacc = wave_sum(sacc);
      if (lane == 0) A[(size_t)i * lda + j] = -ajj * sacc;
    }
    if (tid == 0) A[(size_t)j * lda + j] = ajj;
    __syncthreads();
  }
  for (int i = 0; i < n; ++i) {
    for (int k = i + tid; k < n; k += QP_BLOCK) rv[k] = A[(size_t)k * lda + i];
    __syncthreads();
    for (int b = tid; b <= i; b += QP_BLOCK) {
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
  for (int e = tid; e < n * n; e += QP_BLOCK) {
    const int a = e / n, b = e - a * n;
    if (b > a) A[(size_t)a * lda + b] = A[(size_t)b * lda + a];
  }
  __syncthreads();
  return true;
}

// ---- OSQP's stopping rules (l = -inf, u = h; infinity norms; no scaling) -------------------------------------------
// the certificates, from the step of an iteration: |dy|, h'dy, |G'dy| and |dx|, q'dx, |P dx|, max(G dx)
__device__ __forceinline__ bool qp_primal_infeasible(const SolveArgs& s, double ndy, double hdy, double ngdy) {
  return ndy > 1e-30 && hdy < -s.eps_prim_inf * ndy && ngdy < s.eps_prim_inf * ndy;
}
__device__ __forceinline__ bool qp_dual_infeasible(const SolveArgs& s, double ndx, double qdx, double npdx,
                                                   double mgdx) {
  return ndx > 1e-30 && qdx < -s.eps_dual_inf * ndx && npdx < s.eps_dual_inf * ndx && mgdx < s.eps_dual_inf * ndx;
}
// ---- soft rows (the SOFT instantiations of the two solves): row i costs lin t + 1/2 quad t^2 for t = (Gx - h)_i > 0
// a pair the solve takes: lin in [0, +inf] (+inf: a hard row), quad in [0, +inf); a NaN fails both
__device__ __forceinline__ bool qp_soft_valid(double lin, double quad) {
  return lin >= 0.0 && quad >= 0.0 && quad < INFINITY;
}
__device__ __forceinline__ bool qp_soft_row(double lin) { return lin < INFINITY; }
// the z update, v = alpha zt + (1 - alpha) z + y / rho: the minimiser of phi(z - h) + rho / 2 (z - v)^2.  A hard row
// takes the hard solve's expression itself; a soft row past h stays at h while rho (v - h) <= lin (y, the slope
// there, is below lin) and moves out at slope lin + quad (z - h) beyond
// (quad: where the row's quad lies -- read only by a soft row past h)
__device__ __forceinline__ double qp_soft_z(double v, double h, double rho, double lin, const double* quad) {
  if (!qp_soft_row(lin) || !(v > h)) return fmin(v, h);
  return h + fmax(0.0, (rho * (v - h) - lin) / (rho + *quad));
}

// the verdict of a check -- "solved", "primal infeasible", "dual infeasible", in that order; 0: go on -- from the
// residuals r_p, r_d and their scales
__device__ __forceinline__ int qp_verdict(const SolveArgs& s, double rp, double sp, double rd, double sd, bool pinf,
                                          bool dinf) {
  return rp <= s.eps_abs + s.eps_rel * sp && rd <= s.eps_abs + s.eps_rel * sd ? MPCASM_QP_SOLVED
         : pinf ? MPCASM_QP_PRIMAL_INFEASIBLE
         : dinf ? MPCASM_QP_DUAL_INFEASIBLE : 0;
}
// OSQP's step after check k of an instance that goes on: the two residuals equally far from their tolerances,
// clamped; rho itself where the step is not due (a NaN: no move, it fails the caller's 5x test)
__device__ __forceinline__ double qp_next_rho(const SolveArgs& s, double rho, int verdict, int k, int iters, double rp,
                                              double sp, double rd, double sd) {
  double rn = rho;
  if (verdict == 0 && s.adaptive_rho_interval > 0 && k % s.adaptive_rho_interval == 0 && k < iters) {
    rn = rho * sqrt((rp / (sp + 1e-30)) / (rd / (sd + 1e-30)));
    rn = rn < 1e-6 ? 1e-6 : rn > 1e6 ? 1e6 : rn;
  }
  return rn;
}

}  // namespace mpcasm
