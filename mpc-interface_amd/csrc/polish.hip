// polish.hip -- K6: OSQP's solution polishing for a batch of solved QPs, on the device.  What
// qpsolvers.osqp_solve_qp (use_examples/simple_functional_example/biped_mpc_loop.py:60) does after its ADMM
// loop has stopped, when polishing is asked for: guess the active set from the iterate, solve the KKT system
// of the equality-constrained QP on it, refine, and keep the result only when it is the better point
// (Stellato, Banjac, Goulart, Bemporad, Boyd, Math. Prog. Comp. 12 (2020), section 4 "Solution polishing").
// For  min 1/2 x'Px + q'x  s.t.  Gx <= h  (l = -inf, u = h) and an iterate x, y, z:
//     active            row i iff h_i - z_i < y_i;  G_A, h_A the na active rows (na > no: skipped)
//     K = [[P, G_A'], [G_A, 0]],  g = [-q; h_A],  dK = diag(delta I_no, -delta I_na)
//     t = (K + dK)^-1 g;  refine_iters times  t += (K + dK)^-1 (g - K t)      (K, P, G as given: not regularised)
//     x^ = t[:no],  y^ = t[no:] on the active rows and 0 elsewhere,  z^ = min(G x^, h)
//     accepted iff OSQP's rule on the residuals holds AND every y^_i >= 0 (the second half is this
//     project's, the biped's loop produces points that OSQP's rule lets through with a negative multiplier)
// restated on the CPU by tests/polish_restatement.py, which the tests hold this kernel to.
//
// One workgroup of four wavefronts per instance, as admm.hip.  K + dK is quasi-definite; block elimination on
// it is two Cholesky factorisations:  Pd = P + delta I = L L'  and  S = G_A Pd^-1 G_A' + delta I = Ls Ls'  (na <= no),
// both with admm.hip's in-LDS code, both factors inverted column by column (T = L^-1, Ts = Ls^-1).  With
// W = G_A T' (so that S = W W' + delta I) a solve of (K + dK) [dx; dy] = [r1; r2] is six matrix-vector products
//     u = T r1;  w = W u - r2;  v = Ts w;  dy = Ts' v;  s = u - W' dy;  dx = T' s
// every sum cut over the four wavefronts, none a dependent chain longer than a row.  LDS per instance: four
// matrices of no (no | 1) doubles -- Pd -> L -> W;  T;  G_A -> Ts;  S -> Ls -- and the vectors: see polish_lds.
// The residuals (of the iterate passed in, of every refinement step and of the polished point) read P and G
// from memory, a wavefront per row, the lanes along it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace mpcasm {

namespace {

constexpr int POLISH_BLOCK = 256;
constexpr int POLISH_WAVES = POLISH_BLOCK / 64;

struct PolishLds {
  int m1, m2, m3, m4, x, ya, r1, r2, u, w, s, q, d, h, y, z, gx, pa, red, idx, total, ld;
};
__host__ __device__ inline PolishLds polish_lds(int no, int nc) {
  PolishLds L;
  L.ld = no | 1;   // (an odd leading dimension: a column of a row-major matrix is conflict-free)
  const int mat = no * L.ld;
  L.m1 = 0;                 // Pd, its factor L, then W = G_A T'      [no][ld], [na][ld]
  L.m2 = L.m1 + mat;        // T = L^-1                               [no][ld]
  L.m3 = L.m2 + mat;        // G_A, then Ts = Ls^-1                   [na][ld]
  L.m4 = L.m3 + mat;        // S, then its factor Ls                  [na][ld]
  L.x = L.m4 + mat;         // x^ (first: the iterate's x)
  L.ya = L.x + no;          // y^ on the active rows, compact
  L.r1 = L.ya + no;
  L.r2 = L.r1 + no;
  L.u = L.r2 + no;
  L.w = L.u + no;           // w, then v
  L.s = L.w + no;           // dy, then s
  L.q = L.s + no;
  L.d = L.q + no;           // P x + q + G'y
  L.h = L.d + no;
  L.y = L.h + nc;           // the iterate's y, then y^ on all rows
  L.z = L.y + nc;           // the iterate's z
  L.gx = L.z + nc;          // G x
  L.pa = L.gx + nc;         // [POLISH_WAVES][no] partial sums
  L.red = L.pa + POLISH_WAVES * no;   // 16 doubles: reductions and verdicts
  L.idx = L.red + 16;       // no int32: the active rows, ascending
  L.total = L.idx + (no + 1) / 2;
  L.total += L.total & 1;
  return L;
}

// sum_i a[i sa] b[i sb], i < n: four sums side by side (admm.hip's dot4, half as deep: the sums here are short)
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

// the larger of two, a NaN on either side kept (fmax drops it: a NaN must fail every comparison of the rule)
__device__ __forceinline__ double nmax(double a, double b) { return (a > b || a != a) ? a : b; }

// Cholesky in place of the lower triangle of M [n][ld] (admm.hip's); false when a pivot is not positive
__device__ inline bool cholesky_lds(double* M, int n, int ld, int tid, int lane, int wave) {
  bool good = true;
  for (int k = 0; k < n; ++k) {
    const double dkk = M[k * ld + k];
    good = good && dkk > 0.0;
    const double d = sqrt(dkk > 0.0 ? dkk : 1.0);
    __syncthreads();
    for (int i = k + tid; i < n; i += POLISH_BLOCK) M[i * ld + k] = i == k ? d : M[i * ld + k] / d;
    __syncthreads();
    // the trailing block: wavefront w takes the rows k + 1 + w, + 4, ..., a lane the column k + 1 + lane
    // (+ 64, ... for more unknowns than lanes) up to the diagonal
    for (int j = k + 1 + lane; j < n; j += 64) {
      const double ljk = M[j * ld + k];
      for (int i = k + 1 + wave + (j > k + 1 + wave ? ((j - k - 1 - wave + POLISH_WAVES - 1) / POLISH_WAVES) * POLISH_WAVES : 0);
           i < n; i += POLISH_WAVES)
        M[i * ld + j] = fma(-M[i * ld + k], ljk, M[i * ld + j]);
    }
    __syncthreads();
  }
  return good;
}

// T [n][ld] = L^-1: thread c solves L t = e_c (rows above c are zero)
__device__ inline void invert_lower_lds(const double* Lm, double* T, int n, int ld, int tid) {
  for (int c = tid; c < n; c += POLISH_BLOCK)
    for (int i = 0; i < n; ++i) {
      const double sv = (i == c ? 1.0 : 0.0) - (i > c ? pdot(Lm + i * ld + c, 1, T + c * ld + c, ld, i - c) : 0.0);
      T[i * ld + c] = i < c ? 0.0 : sv / Lm[i * ld + i];
    }
  __syncthreads();
}

// wavefront `wave`'s quarter of out = M v (TRANS: M'v), M [.][ld]: pa[wave][c], c < n_out, over the terms
// wave, wave + 4, ... < n_sum
template <bool TRANS>
__device__ __forceinline__ void mv_part(const double* M, int ld, int n_out, int n_sum, const double* v,
                                        double* pa, int lp, int lane, int wave) {
  const int terms = n_sum > wave ? (n_sum - wave + POLISH_WAVES - 1) / POLISH_WAVES : 0;
  for (int c = lane; c < n_out; c += 64)
    pa[wave * lp + c] = TRANS ? pdot(M + wave * ld + c, POLISH_WAVES * ld, v + wave, POLISH_WAVES, terms)
                              : pdot(M + c * ld + wave, POLISH_WAVES, v + wave, POLISH_WAVES, terms);
}
__device__ __forceinline__ double sum4(const double* pa, int lp, int c) {
  return (pa[c] + pa[lp + c]) + (pa[2 * lp + c] + pa[3 * lp + c]);
}

__global__ __launch_bounds__(POLISH_BLOCK) void polish_kernel(
    int no, int nc, const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ G,
    const double* __restrict__ h, double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Z,
    const int32_t* __restrict__ status, double delta, int refine_iters, int32_t* __restrict__ polish,
    double* __restrict__ res, int batch) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long inst = blockIdx.x;
  if (inst >= batch) return;
  // (an instance that is not solved is not read at all: a NON_CVX one holds NaN)
  if (status != nullptr && status[inst] != MPCASM_QP_SOLVED) {
    if (tid == 0) polish[inst] = MPCASM_POLISH_SKIPPED;
    return;
  }
  const PolishLds L = polish_lds(no, nc);
  const int ld = L.ld;
  double* M1 = sm + L.m1;
  double* T = sm + L.m2;
  double* M3 = sm + L.m3;
  double* M4 = sm + L.m4;
  double* xs = sm + L.x;
  double* ya = sm + L.ya;
  double* r1 = sm + L.r1;
  double* r2 = sm + L.r2;
  double* us = sm + L.u;
  double* ws = sm + L.w;
  double* ss = sm + L.s;
  double* qs = sm + L.q;
  double* ds = sm + L.d;
  double* hs = sm + L.h;
  double* ys = sm + L.y;
  double* zs = sm + L.z;
  double* gx = sm + L.gx;
  double* pa = sm + L.pa;
  double* red = sm + L.red;
  int* idx = reinterpret_cast<int*>(sm + L.idx);
  const double* Pb = P + (size_t)inst * no * no;
  const double* Gb = G + (size_t)inst * nc * no;
  double* Xb = X + (size_t)inst * no;
  double* Yb = Y + (size_t)inst * nc;
  double* Zb = Z + (size_t)inst * nc;

  for (int e = tid; e < no; e += POLISH_BLOCK) {
    qs[e] = q[(size_t)inst * no + e];
    xs[e] = Xb[e];
  }
  for (int e = tid; e < nc; e += POLISH_BLOCK) {
    hs[e] = h[(size_t)inst * nc + e];
    ys[e] = Yb[e];
    zs[e] = Zb[e];
  }
  __syncthreads();

  // ---- the active set: OSQP's test, the rows kept in ascending order (one wavefront, 64 rows a pass) -------
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
  if (na > no) {   // (more active rows than unknowns: no KKT system of full rank to solve)
    if (tid == 0) polish[inst] = MPCASM_POLISH_SKIPPED;
    return;
  }

  // out[r] = M[r] . xs for the rows of a matrix in memory: a wavefront takes four rows at a time, so that four
  // rows' loads are in flight before the first sum is reduced (one row at a time was one memory latency a row)
  auto rows_times_x = [&](const double* M, int rows, double* out) {
    constexpr int RB = 4;
    for (int r0 = wave * RB; r0 < rows; r0 += POLISH_WAVES * RB) {
      double acc[RB];
#pragma unroll
      for (int u = 0; u < RB; ++u) {
        acc[u] = 0.0;
        if (r0 + u < rows)
          for (int c = lane; c < no; c += 64) acc[u] = fma(M[(size_t)(r0 + u) * no + c], xs[c], acc[u]);
      }
#pragma unroll
      for (int u = 0; u < RB; ++u)
        for (int off = 32; off > 0; off >>= 1) acc[u] += __shfl_xor(acc[u], off, 64);
#pragma unroll
      for (int u = 0; u < RB; ++u)
        if (lane == 0 && r0 + u < rows) out[r0 + u] = acc[u];
    }
  };

  // |G x - z|_inf (zv == nullptr: |G x - min(G x, h)|_inf) and |P x + q + G'y|_inf of xs and the y in ys, both
  // kept in gx and ds: a wavefront per row of G and of P, the lanes along the row; G'y cut over the wavefronts
  // by rows, a lane a column (rows whose y is 0 are not read: most of them, for a polished point)
  auto residuals = [&](const double* zv, double* rp_out, double* rd_out) {
    rows_times_x(Gb, nc, gx);
    rows_times_x(Pb, no, ds);
    for (int c = lane; c < no; c += 64) {
      double s0 = 0.0, s1 = 0.0;
      int r = wave;
      for (; r + POLISH_WAVES < nc; r += 2 * POLISH_WAVES) {
        const double y0 = ys[r], y1 = ys[r + POLISH_WAVES];
        if (y0 != 0.0) s0 = fma(Gb[(size_t)r * no + c], y0, s0);
        if (y1 != 0.0) s1 = fma(Gb[(size_t)(r + POLISH_WAVES) * no + c], y1, s1);
      }
      if (r < nc && ys[r] != 0.0) s0 = fma(Gb[(size_t)r * no + c], ys[r], s0);
      pa[wave * no + c] = s0 + s1;
    }
    __syncthreads();
    double rp = 0.0, rd = 0.0;
    for (int c = tid; c < no; c += POLISH_BLOCK) {
      const double dv = (ds[c] + qs[c]) + sum4(pa, no, c);
      ds[c] = dv;
      rd = nmax(rd, fabs(dv));
    }
    for (int r = tid; r < nc; r += POLISH_BLOCK)
      rp = nmax(rp, fabs(gx[r] - (zv != nullptr ? zv[r] : fmin(gx[r], hs[r]))));
    for (int off = 32; off > 0; off >>= 1) {
      rp = nmax(rp, __shfl_xor(rp, off, 64));
      rd = nmax(rd, __shfl_xor(rd, off, 64));
    }
    if (lane == 0) {
      red[wave] = rp;
      red[POLISH_WAVES + wave] = rd;
    }
    __syncthreads();
    *rp_out = nmax(nmax(red[0], red[1]), nmax(red[2], red[3]));
    *rd_out = nmax(nmax(red[4], red[5]), nmax(red[6], red[7]));
    __syncthreads();   // (red and pa are free again)
  };

  // ---- r_p, r_d of the iterate passed in -----------------------------------------------------------------
  double rp_in, rd_in;
  residuals(zs, &rp_in, &rd_in);

  // ---- Pd = P + delta I and the active rows of G, on chip ---------------------------------------------------
  for (int e = tid; e < no * no; e += POLISH_BLOCK) {
    const int a = e / no, b = e - a * no;
    M1[a * ld + b] = Pb[e] + (a == b ? delta : 0.0);
  }
  for (int e = tid; e < na * no; e += POLISH_BLOCK) {
    const int a = e / no, c = e - a * no;
    M3[a * ld + c] = Gb[(size_t)idx[a] * no + c];
  }
  __syncthreads();
  bool good = cholesky_lds(M1, no, ld, tid, lane, wave);
  invert_lower_lds(M1, T, no, ld, tid);
  // ---- W = G_A T' over L (T is lower triangular: the sum ends at the diagonal) ------------------------------
  for (int e = tid; e < na * no; e += POLISH_BLOCK) {
    const int a = e / no, k = e - a * no;
    M1[a * ld + k] = pdot(M3 + a * ld, 1, T + k * ld, 1, k + 1);
  }
  __syncthreads();
  // ---- S = W W' + delta I, factored, the factor inverted over G_A ----------------------------------------------
  for (int e = tid; e < na * na; e += POLISH_BLOCK) {
    const int a = e / na, b = e - a * na;
    M4[a * ld + b] = pdot(M1 + a * ld, 1, M1 + b * ld, 1, no) + (a == b ? delta : 0.0);
  }
  __syncthreads();
  good = cholesky_lds(M4, na, ld, tid, lane, wave) && good;
  if (!good) {   // (a pivot that is not positive, a NaN among them)
    if (tid == 0) polish[inst] = MPCASM_POLISH_REJECTED;
    return;
  }
  invert_lower_lds(M4, M3, na, ld, tid);
  const double* W = M1;
  const double* Ts = M3;

  // (K + dK) [dx; dy] = [r1; r2]: dx in us, dy in ss
  auto kkt_solve = [&]() {
    mv_part<false>(T, ld, no, no, r1, pa, no, lane, wave);
    __syncthreads();
    for (int c = tid; c < no; c += POLISH_BLOCK) us[c] = sum4(pa, no, c);            // u = T r1
    __syncthreads();
    mv_part<false>(W, ld, na, no, us, pa, no, lane, wave);
    __syncthreads();
    for (int a = tid; a < na; a += POLISH_BLOCK) ws[a] = sum4(pa, no, a) - r2[a];    // w = W u - r2
    __syncthreads();
    mv_part<false>(Ts, ld, na, na, ws, pa, no, lane, wave);
    __syncthreads();
    for (int a = tid; a < na; a += POLISH_BLOCK) ws[a] = sum4(pa, no, a);            // v = Ts w
    __syncthreads();
    mv_part<true>(Ts, ld, na, na, ws, pa, no, lane, wave);
    __syncthreads();
    for (int a = tid; a < na; a += POLISH_BLOCK) ss[a] = sum4(pa, no, a);            // dy = Ts' v
    __syncthreads();
    mv_part<true>(W, ld, no, na, ss, pa, no, lane, wave);
    __syncthreads();
    for (int c = tid; c < no; c += POLISH_BLOCK) us[c] -= sum4(pa, no, c);           // s = u - W' dy
    __syncthreads();
    mv_part<true>(T, ld, no, no, us, pa, no, lane, wave);
    __syncthreads();
    for (int c = tid; c < no; c += POLISH_BLOCK) us[c] = sum4(pa, no, c);            // dx = T' s
    __syncthreads();
  };

  // ---- t0 = (K + dK)^-1 g, then the refinement against the K that is not regularised ---------------------------
  for (int c = tid; c < no; c += POLISH_BLOCK) r1[c] = -qs[c];
  for (int a = tid; a < na; a += POLISH_BLOCK) r2[a] = hs[idx[a]];
  __syncthreads();
  kkt_solve();
  for (int c = tid; c < no; c += POLISH_BLOCK) xs[c] = us[c];
  for (int r = tid; r < nc; r += POLISH_BLOCK) ys[r] = 0.0;
  __syncthreads();
  for (int a = tid; a < na; a += POLISH_BLOCK) {
    ya[a] = ss[a];
    ys[idx[a]] = ss[a];
  }
  __syncthreads();
  double rp_hat, rd_hat;
  for (int it = 0; it < refine_iters; ++it) {
    residuals(nullptr, &rp_hat, &rd_hat);   // (gx = G x^ and ds = P x^ + q + G'y^ are what the step needs)
    for (int c = tid; c < no; c += POLISH_BLOCK) r1[c] = -ds[c];
    for (int a = tid; a < na; a += POLISH_BLOCK) r2[a] = hs[idx[a]] - gx[idx[a]];
    __syncthreads();
    kkt_solve();
    for (int c = tid; c < no; c += POLISH_BLOCK) xs[c] += us[c];
    for (int a = tid; a < na; a += POLISH_BLOCK) {
      const double yn = ya[a] + ss[a];
      ya[a] = yn;
      ys[idx[a]] = yn;
    }
    __syncthreads();
  }

  // ---- the polished point and the verdict ----------------------------------------------------------------
  residuals(nullptr, &rp_hat, &rd_hat);
  double neg = 0.0;
  for (int a = tid; a < na; a += POLISH_BLOCK) neg = ya[a] >= 0.0 ? neg : 1.0;   // (a NaN counts as negative)
  for (int off = 32; off > 0; off >>= 1) neg = fmax(neg, __shfl_xor(neg, off, 64));
  if (lane == 0) red[8 + wave] = neg;
  __syncthreads();
  const bool signs = red[8] == 0.0 && red[9] == 0.0 && red[10] == 0.0 && red[11] == 0.0;
  const bool better = (rp_hat < rp_in && rd_hat < rd_in) || (rp_hat < rp_in && rd_in < 1e-10) ||
                      (rd_hat < rd_in && rp_in < 1e-10);
  if (!(better && signs)) {
    if (tid == 0) polish[inst] = MPCASM_POLISH_REJECTED;
    return;
  }
  for (int c = tid; c < no; c += POLISH_BLOCK) Xb[c] = xs[c];
  for (int r = tid; r < nc; r += POLISH_BLOCK) {
    Yb[r] = ys[r];
    Zb[r] = fmin(gx[r], hs[r]);
  }
  if (tid == 0) {
    polish[inst] = MPCASM_POLISH_DONE;
    if (res != nullptr) {
      res[inst * 2 + 0] = rp_hat;
      res[inst * 2 + 1] = rd_hat;
    }
  }
}

}  // namespace

size_t polish_lds_bytes(int no, int nc) { return (size_t)polish_lds(no, nc).total * sizeof(double); }

int launch_qp_polish(int no, int nc, const double* P, const double* q, const double* G, const double* h,
                     double* x, double* y, double* z, const int32_t* status, double delta, int refine_iters,
                     int32_t* polish, double* res, int batch, hipStream_t stream, hipError_t* err) {
  const size_t lds = polish_lds_bytes(no, nc);
  if (lds > (size_t)RESIDENT_LDS_LIMIT) return MPCASM_ERR_LIMIT;
  if (lds > 64 * 1024) {
    *err = allow_whole_lds(reinterpret_cast<const void*>(polish_kernel));
    if (*err != hipSuccess) return MPCASM_ERR_HIP;
  }
  hipLaunchKernelGGL(polish_kernel, dim3((unsigned)batch), dim3(POLISH_BLOCK), lds, stream, no, nc, P, q, G, h,
                     x, y, z, status, delta, refine_iters, polish, res, batch);
  *err = hipGetLastError();
  return *err == hipSuccess ? MPCASM_OK : MPCASM_ERR_HIP;
}

}  // namespace mpcasm
