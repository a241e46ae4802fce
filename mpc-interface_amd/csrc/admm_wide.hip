// admm_wide.hip -- K5's solve to tolerance for QPs whose matrices do not fit in one workgroup's LDS
// (mpcasm_qp_solve_wide): the iteration, the stopping rules and adaptive rho of admm.hip's solve mode,
// restated for G read in place from the caller's buffer and K^-1 in LDS only where it fits beside the
// vectors, else in the caller's d_kinv.
//
// One workgroup of four wavefronts per instance, no state shared between workgroups.  Every vector of
// length no lives in registers, lane l holding the columns j = l, l + 64, ... (NCH of them) -- replicated in
// the four wavefronts, which compute them alike -- and in LDS where a wavefront must read another lane's
// entry; the vectors of length nc (z, y, h) and the per-wavefront partial sums live in LDS.  An iteration:
//   A  r = sigma x - q + G'v from the partial sums the last pass left            (a barrier)
//   B  xt = K^-1 r: K^-1 is symmetric, so lane j sums K^-1[b][j] r[b] over the rows b of its wavefront,
//      coalesced, no reduction across lanes; the four partials meet in LDS       (a barrier)
//   C  xt and x+ = alpha xt + (1 - alpha) x, in registers
//   D  one pass over G: wavefront w takes the rows i = w, w + 4, ..., four in flight; G_i xt is one
//      reduction across the wavefront, z_i, y_i and v_i = rho z_i - y_i follow, and v_i G_i goes into the
//      lanes' column accumulators -- next iteration's G'v -- while the row is still in registers (a barrier)
// At a check the same pass also forms G_i x, G_i dx, G'y and G'dy; P x and P dx come from d_P.  The verdicts
// are admm.hip's, in its order, one per workgroup (every wavefront reaches the same one from the same sums).
//
// K = P + sigma I + rho G'G is formed, factored (Cholesky, in place: potrf), its factor inverted in place
// (trtri) and K^-1 = L^-T L^-1 formed in place (lauum) -- LAPACK's order, unblocked, a barrier per step --
// in LDS or in d_kinv[b], by the same code; adaptive rho calls it again.  Values this kernel wrote to d_kinv
// are read back only behind a workgroup barrier, with vector loads: the pointer is neither const nor restrict.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "kernels.h"
#include "qp_prims.h"

namespace mpcasm {

namespace {

constexpr int WIDE_ROWS = 4;   // rows of G a wavefront keeps in flight in the pass
constexpr int WIDE_MAX_NO = 512;

struct WideLds {
  int z, y, h, xs, dx, rv, pa, pb, pc, pk, pe, red, sl, sq, mi, ld, total;
};
// soft: the soft instantiations' layout -- the two penalty vectors between the verdict terms and K^-1
__host__ __device__ inline WideLds wide_lds(int no, int nc, bool onchip, bool soft = false) {
  WideLds L;
  L.ld = no | 1;   // (K^-1 in LDS: an odd leading dimension, the factorisation walks its columns)
  L.z = 0;
  L.y = L.z + nc;
  L.h = L.y + nc;
  L.xs = L.h + nc;             // x, for the rows of P x (checks)
  L.dx = L.xs + no;            // dx, for P dx (checks)
  L.rv = L.dx + no;            // r; the factorisation's column
  L.pa = L.rv + no;            // [QP_WAVES][no] partial sums of G'v
  L.pb = L.pa + QP_WAVES * no;   // of G'y (checks)
  L.pc = L.pb + QP_WAVES * no;   // of G'dy (checks)
  L.pk = L.pc + QP_WAVES * no;   // of K^-1 r; of P x (checks)
  L.pe = L.pk + QP_WAVES * no;   // of P dx (checks)
  L.red = L.pe + QP_WAVES * no;  // [QP_WAVES][16] a wavefront's row verdict terms
  L.sl = L.red + QP_WAVES * 16;  // lin, quad [nc] (soft only)
  L.sq = L.sl + (soft ? nc : 0);
  L.mi = L.sq + (soft ? nc : 0);
  L.total = L.mi + (onchip ? no * L.ld : 0);
  L.total += L.total & 1;
  return L;
}

// NCH: columns per lane (no <= 64 NCH); ONCHIP: K^-1 in LDS; S = SoftSolveArgs: the soft instantiation
// (mpcasm_qp_solve_wide_soft), which differs as admm.hip's does -- the load, the z update, the dy a check keeps
template <int NCH, bool ONCHIP, typename S = SolveArgs>
__global__ __launch_bounds__(QP_BLOCK) void admm_wide_kernel(
    int no, int nc, const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ G,
    const double* __restrict__ h, double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Z,
    double* __restrict__ res, double sigma, double alpha, int iters, int warm, int batch, double* Kinv,
    int kinv_valid, S s) {
  constexpr bool SOFT = std::is_same<S, SoftSolveArgs>::value;
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long inst = blockIdx.x;
  if (inst >= batch) return;
  const WideLds L = wide_lds(no, nc, ONCHIP, SOFT);
  double* sl = sm + L.sl;   // (SOFT only)
  double* sq = sm + L.sq;
  double* zs = sm + L.z;
  double* ys = sm + L.y;
  double* hs = sm + L.h;
  double* xs = sm + L.xs;
  double* dxs = sm + L.dx;
  double* rv = sm + L.rv;
  double* pa = sm + L.pa;
  double* pb = sm + L.pb;
  double* pc = sm + L.pc;
  double* pk = sm + L.pk;
  double* pe = sm + L.pe;
  double* red = sm + L.red;
  const double* Pb = P + (size_t)inst * no * no;
  const double* Gb = G + (size_t)inst * nc * no;
  double* Kg = Kinv != nullptr ? Kinv + (size_t)inst * no * no : nullptr;
  double* Km = ONCHIP ? sm + L.mi : Kg;   // where the iteration reads K^-1
  const int kld = ONCHIP ? L.ld : no;
  const double bad = __builtin_nan("");

  double rho = s.rho[inst];
  bool pen_bad = false;
  double xr[NCH], qr[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = lane + 64 * c;
    qr[c] = j < no ? q[(size_t)inst * no + j] : 0.0;
    xr[c] = j < no && warm ? X[(size_t)inst * no + j] : 0.0;
  }
  for (int e = tid; e < nc; e += QP_BLOCK) {
    const double hv = h[(size_t)inst * nc + e];
    hs[e] = hv;
    ys[e] = warm ? Y[(size_t)inst * nc + e] : 0.0;
    zs[e] = warm ? Z[(size_t)inst * nc + e] : fmin(0.0, hv);
    if constexpr (SOFT) {
      const double lv = s.soft.lin[inst * s.soft.stride + e], qv = s.soft.quad[inst * s.soft.stride + e];
      sl[e] = lv;
      sq[e] = qv;
      pen_bad = pen_bad || !qp_soft_valid(lv, qv);
    }
  }
  if constexpr (SOFT) {   // (one bad pair: the instance is not solved; red is free until the first pass)
    const bool any = __ballot(pen_bad) != 0;
    if (lane == 0) red[wave * 16] = any ? 1.0 : 0.0;
    __syncthreads();
    pen_bad = (red[0] + red[16]) + (red[32] + red[48]) != 0.0;
  }

  // ---- K = P + sigma I + rho G'G, then K^-1 in place (false: K is not positive definite) ---------------
  auto factor = [&]() -> bool {
    double* A = Km;
    const int lda = kld;
    __syncthreads();
    // wavefront w forms the rows a = w + 4 t, four at a time: one sweep over G's rows serves the four
    for (int a0 = wave; a0 < no; a0 += QP_WAVES * 4) {
      double acc[4][NCH];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[u][c] = 0.0;
      for (int r = 0; r < nc; ++r) {
        const double* gr = Gb + (size_t)r * no;
        double ga[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int a = a0 + QP_WAVES * u;
          ga[u] = a < no ? gr[a] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int j = lane + 64 * c;
          const double gb = j < no ? gr[j] : 0.0;
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[u][c] = fma(ga[u], gb, acc[u][c]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int a = a0 + QP_WAVES * u;
        if (a >= no) break;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int j = lane + 64 * c;
          if (j < no) A[(size_t)a * lda + j] = fma(rho, acc[u][c], Pb[(size_t)a * no + j]) + (a == j ? sigma : 0.0);
        }
      }
    }
    __syncthreads();
    bool good = true;
    // ---- potrf: K = L L', the lower triangle in place ------------------------------------------------
    for (int k = 0; k < no; ++k) {
      const double dkk = A[(size_t)k * lda + k];
      good = good && dkk > 0.0;
      const double d = sqrt(dkk > 0.0 ? dkk : 1.0);
      __syncthreads();
      for (int i = k + tid; i < no; i += QP_BLOCK) {
        const double v = i == k ? d : A[(size_t)i * lda + k] / d;
        A[(size_t)i * lda + k] = v;
        rv[i] = v;
      }
      __syncthreads();
      for (int i = k + 1 + wave; i < no; i += QP_WAVES) {
        const double li = rv[i];
        for (int j = k + 1 + lane; j <= i; j += 64) A[(size_t)i * lda + j] = fma(-li, rv[j], A[(size_t)i * lda + j]);
      }
      __syncthreads();
    }
    // ---- trtri: L^-1 in place, column j from the inverted trailing block --------------------------------
    for (int j = no - 1; j >= 0; --j) {
      const double ljj = A[(size_t)j * lda + j];
      for (int i = j + 1 + tid; i < no; i += QP_BLOCK) rv[i] = A[(size_t)i * lda + j];
      __syncthreads();
      const double ajj = 1.0 / ljj;
      for (int i = j + 1 + wave; i < no; i += QP_WAVES) {
        double sacc = 0.0;
        for (int k = j + 1 + lane; k <= i; k += 64) sacc = fma(A[(size_t)i * lda + k], rv[k], sacc);
        sacc = wave_sum(sacc);
        if (lane == 0) A[(size_t)i * lda + j] = -ajj * sacc;
      }
      if (tid == 0) A[(size_t)j * lda + j] = ajj;
      __syncthreads();
    }
    // ---- lauum: K^-1 = L^-T L^-1, row i from the rows >= i (not yet overwritten) ----------------------------
    for (int i = 0; i < no; ++i) {
      for (int k = i + tid; k < no; k += QP_BLOCK) rv[k] = A[(size_t)k * lda + i];
      __syncthreads();
      for (int b = tid; b <= i; b += QP_BLOCK) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int k = i;
        for (; k + 4 <= no; k += 4) {
          s0 = fma(rv[k], A[(size_t)k * lda + b], s0);
          s1 = fma(rv[k + 1], A[(size_t)(k + 1) * lda + b], s1);
          s2 = fma(rv[k + 2], A[(size_t)(k + 2) * lda + b], s2);
          s3 = fma(rv[k + 3], A[(size_t)(k + 3) * lda + b], s3);
        }
        for (; k < no; ++k) s0 = fma(rv[k], A[(size_t)k * lda + b], s0);
        A[(size_t)i * lda + b] = (s0 + s1) + (s2 + s3);   // (only this thread reads (i, b))
      }
      __syncthreads();
    }
    // the upper triangle from the lower: the iteration reads whole rows
    for (int e = tid; e < no * no; e += QP_BLOCK) {
      const int a = e / no, b = e - a * no;
      if (b > a) A[(size_t)a * lda + b] = A[(size_t)b * lda + a];
    }
    __syncthreads();
    if (ONCHIP && Kg != nullptr) {
      for (int e = tid; e < no * no; e += QP_BLOCK) {
        const int a = e / no, b = e - a * no;
        Kg[e] = good ? A[(size_t)a * lda + b] : bad;
      }
    } else if (!good) {
      for (int e = tid; e < no * no; e += QP_BLOCK) {
        const int a = e / no, b = e - a * no;
        A[(size_t)a * lda + b] = bad;
      }
    }
    __syncthreads();
    return good;
  };

  // ---- one pass over G's rows of this wavefront (UPDATE: the iteration's z, y and G'v; CHECK: the terms of
  // the verdicts; neither: G'v from the current z, y) ---------------------------------------------------------
  // xt: G_i xt is the iteration's zt_i; xn: the x of G x; dxr: dx.  Column sums of the wavefront's rows go to
  // pa (v), pb (y), pc (dy); row terms to red[wave][0..4]: |Gx - z|, max(|Gx|, |z|), |dy|, h'dy, max G dx.
  auto pass = [&](auto update, auto check, const double* xt, const double* xn, const double* dxr, double inv_rho) {
    constexpr bool UPD = decltype(update)::value, CHK = decltype(check)::value;
    double cv[NCH], cy[NCH], cd[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) cv[c] = cy[c] = cd[c] = 0.0;
    double rp = 0.0, sp = 0.0, ndy = 0.0, hdy = 0.0, mgdx = -INFINITY;
    for (int i0 = wave; i0 < nc; i0 += QP_WAVES * WIDE_ROWS) {
      double g[WIDE_ROWS][NCH];
#pragma unroll
      for (int u = 0; u < WIDE_ROWS; ++u) {
        const int i = i0 + QP_WAVES * u;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int j = lane + 64 * c;
          g[u][c] = i < nc && j < no ? Gb[(size_t)i * no + j] : 0.0;
        }
      }
      double zt[WIDE_ROWS], gx[WIDE_ROWS], gd[WIDE_ROWS];
#pragma unroll
      for (int u = 0; u < WIDE_ROWS; ++u) {
        zt[u] = gx[u] = gd[u] = 0.0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          if (UPD) zt[u] = fma(g[u][c], xt[c], zt[u]);
          if (CHK) gx[u] = fma(g[u][c], xn[c], gx[u]), gd[u] = fma(g[u][c], dxr[c], gd[u]);
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int u = 0; u < WIDE_ROWS; ++u) {
          if (UPD) zt[u] += __shfl_xor(zt[u], off, 64);
          if (CHK) gx[u] += __shfl_xor(gx[u], off, 64), gd[u] += __shfl_xor(gd[u], off, 64);
        }
      }
#pragma unroll
      for (int u = 0; u < WIDE_ROWS; ++u) {
        const int i = i0 + QP_WAVES * u;
        if (i >= nc) break;
        double zn = zs[i], yn = ys[i], dy = 0.0;
        if (UPD) {
          const double zr = fma(alpha, zt[u], (1.0 - alpha) * zn);
          const double yo = yn;
          if constexpr (SOFT) zn = qp_soft_z(fma(yo, inv_rho, zr), hs[i], rho, sl[i], sq + i);
          else zn = fmin(fma(yo, inv_rho, zr), hs[i]);
          yn = fma(rho, zr - zn, yo);
          dy = SOFT && qp_soft_row(sl[i]) ? 0.0 : fmax(yn - yo, 0.0);   // (a soft row certifies nothing)
          if (lane == 0) zs[i] = zn, ys[i] = yn;
        }
        const double v = fma(rho, zn, -yn);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          if (UPD || !CHK) cv[c] = fma(v, g[u][c], cv[c]);
          if (CHK) cy[c] = fma(yn, g[u][c], cy[c]), cd[c] = fma(dy, g[u][c], cd[c]);
        }
        if (CHK) {
          rp = fmax(rp, fabs(gx[u] - zn));
          sp = fmax(sp, fmax(fabs(gx[u]), fabs(zn)));
          ndy = fmax(ndy, dy);
          hdy = fma(hs[i], dy, hdy);
          mgdx = fmax(mgdx, gd[u]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = lane + 64 * c;
      if (j >= no) continue;
      if (UPD || !CHK) pa[wave * no + j] = cv[c];
      if (CHK) pb[wave * no + j] = cy[c], pc[wave * no + j] = cd[c];
    }
    if (CHK && lane == 0) {
      red[wave * 16 + 0] = rp, red[wave * 16 + 1] = sp, red[wave * 16 + 2] = ndy;
      red[wave * 16 + 3] = hdy, red[wave * 16 + 4] = mgdx;
    }
  };
  // the four partials of buffer p at this lane's columns
  auto gather = [&](const double* p, double* out) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = lane + 64 * c;
      out[c] = j < no ? (p[j] + p[no + j]) + (p[2 * no + j] + p[3 * no + j]) : 0.0;
    }
  };
  // P a and P b (P symmetric: lane j sums P[b][j] a[b] over its wavefront's rows b) into pk and pe
  auto p_products = [&](const double* av, const double* bv) {
    double ca[NCH], cb[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) ca[c] = cb[c] = 0.0;
    for (int b = wave; b < no; b += QP_WAVES) {
      const double ab = av[b], bb = bv[b];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int j = lane + 64 * c;
        const double pv = j < no ? Pb[(size_t)b * no + j] : 0.0;
        ca[c] = fma(pv, ab, ca[c]);
        cb[c] = fma(pv, bb, cb[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = lane + 64 * c;
      if (j < no) pk[wave * no + j] = ca[c], pe[wave * no + j] = cb[c];
    }
  };
  using T = std::true_type;
  using F = std::false_type;

  bool ok = true;
  if (!(rho > 0.0) || pen_bad) {   // (no step to take: the instance is not convex)
    ok = false;
    if (Kg != nullptr)
      for (int e = tid; e < no * no; e += QP_BLOCK) Kg[e] = bad;
  } else if (Kinv != nullptr && kinv_valid != 0) {
    if (ONCHIP)
      for (int e = tid; e < no * no; e += QP_BLOCK) Km[(e / no) * kld + e % no] = Kg[e];
  } else {
    ok = factor();
  }
  __syncthreads();

  double inv_rho = 1.0 / rho;
  int status = ok ? MPCASM_QP_MAX_ITER : MPCASM_QP_NON_CVX, ran = ok ? iters : 0;
  double none[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) none[c] = 0.0;
  if (ok) pass(F{}, F{}, none, none, none, inv_rho);   // G'v of the start
  __syncthreads();
  for (int it = 0; it < (ok ? iters : 0); ++it) {
    const int k = it + 1;
    const bool due = k % s.check_every == 0 || k == iters;
    // A: r
    double pv[NCH];
    gather(pa, pv);
    if (wave == 0) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int j = lane + 64 * c;
        if (j < no) rv[j] = fma(sigma, xr[c], -qr[c]) + pv[c];
      }
    }
    __syncthreads();
    // B: the wavefront's share of K^-1 r, four rows of K^-1 in flight
    {
      double acc[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) acc[c] = 0.0;
      int b = wave;
      for (; b + 3 * QP_WAVES < no; b += 4 * QP_WAVES) {
        double kv[4][NCH], rb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          rb[u] = rv[b + u * QP_WAVES];
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const int j = lane + 64 * c;
            kv[u][c] = j < no ? Km[(size_t)(b + u * QP_WAVES) * kld + j] : 0.0;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int c = 0; c < NCH; ++c) acc[c] = fma(kv[u][c], rb[u], acc[c]);
      }
      for (; b < no; b += QP_WAVES) {
        const double rb = rv[b];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int j = lane + 64 * c;
          if (j < no) acc[c] = fma(Km[(size_t)b * kld + j], rb, acc[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int j = lane + 64 * c;
        if (j < no) pk[wave * no + j] = acc[c];
      }
    }
    __syncthreads();
    // C: xt, x
    double xt[NCH], dx[NCH];
    gather(pk, xt);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const double xo = xr[c];
      xr[c] = fma(alpha, xt[c], (1.0 - alpha) * xo);
      dx[c] = xr[c] - xo;
    }
    if (due && wave == 0) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int j = lane + 64 * c;
        if (j < no) xs[j] = xr[c], dxs[j] = dx[c];
      }
    }
    // D: the pass over G
    if (due) pass(T{}, T{}, xt, xr, dx, inv_rho);
    else pass(T{}, F{}, xt, xr, dx, inv_rho);
    __syncthreads();
    if (!due) continue;
    // ---- the check -------------------------------------------------------------------------------------
    p_products(xs, dxs);
    __syncthreads();
    double gty[NCH], gtdy[NCH], px[NCH], pdx[NCH];
    gather(pb, gty);
    gather(pc, gtdy);
    gather(pk, px);
    gather(pe, pdx);
    double rd = 0.0, sd = 0.0, ndx = 0.0, qdx = 0.0, npdx = 0.0, ngdy = 0.0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (lane + 64 * c >= no) continue;
      rd = fmax(rd, fabs(px[c] + qr[c] + gty[c]));
      sd = fmax(sd, fmax(fabs(px[c]), fmax(fabs(gty[c]), fabs(qr[c]))));
      ndx = fmax(ndx, fabs(dx[c]));
      qdx = fma(qr[c], dx[c], qdx);
      npdx = fmax(npdx, fabs(pdx[c]));
      ngdy = fmax(ngdy, fabs(gtdy[c]));
    }
    rd = wave_max(rd), sd = wave_max(sd), ndx = wave_max(ndx), qdx = wave_sum(qdx);
    npdx = wave_max(npdx), ngdy = wave_max(ngdy);
    double rp = 0.0, sp = 0.0, ndy = 0.0, hdy = 0.0, mgdx = -INFINITY;
    for (int w = 0; w < QP_WAVES; ++w) {
      rp = fmax(rp, red[w * 16 + 0]);
      sp = fmax(sp, red[w * 16 + 1]);
      ndy = fmax(ndy, red[w * 16 + 2]);
      hdy += red[w * 16 + 3];
      mgdx = fmax(mgdx, red[w * 16 + 4]);
    }
    const int verdict = qp_verdict(s, rp, sp, rd, sd, qp_primal_infeasible(s, ndy, hdy, ngdy),
                                   qp_dual_infeasible(s, ndx, qdx, npdx, mgdx));
    const double rn = qp_next_rho(s, rho, verdict, k, iters, rp, sp, rd, sd);
    if (verdict != 0) {
      status = verdict;
      ran = k;
      break;
    }
    if (rn > 5.0 * rho || rn < rho / 5.0) {
      rho = rn;
      inv_rho = 1.0 / rho;
      if (!factor()) {
        ok = false;
        status = MPCASM_QP_NON_CVX;
        ran = k;
        break;
      }
      pass(F{}, F{}, none, none, none, inv_rho);   // G'v for the new rho
      __syncthreads();
    }
  }
  if (tid == 0) {
    s.rho[inst] = rho;
    s.status[inst] = status;
    s.iters[inst] = ran;
  }

  // ---- results; OSQP's residuals |Gx - z|_inf, |Px + q + G'y|_inf of the returned iterate ------------------
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = lane + 64 * c;
    if (wave == 0 && j < no) X[(size_t)inst * no + j] = ok ? xr[c] : bad;
  }
  for (int r = tid; r < nc; r += QP_BLOCK) {
    Y[(size_t)inst * nc + r] = ok ? ys[r] : bad;
    Z[(size_t)inst * nc + r] = ok ? zs[r] : bad;
  }
  if (res != nullptr) {
    __syncthreads();   // (the last check's readers of pb, pc, pk, pe, red are done)
    if (wave == 0) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int j = lane + 64 * c;
        if (j < no) xs[j] = xr[c], dxs[j] = 0.0;
      }
    }
    __syncthreads();
    pass(F{}, T{}, none, xr, none, inv_rho);
    p_products(xs, dxs);
    __syncthreads();
    if (wave == 0) {
      double gty[NCH], px[NCH];
      gather(pb, gty);
      gather(pk, px);
      double rd = 0.0;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (lane + 64 * c < no) rd = fmax(rd, fabs(px[c] + qr[c] + gty[c]));
      rd = wave_max(rd);
      double rp = 0.0;
      for (int w = 0; w < QP_WAVES; ++w) rp = fmax(rp, red[w * 16 + 0]);
      if (lane == 0) {
        res[inst * 2 + 0] = ok ? rp : bad;
        res[inst * 2 + 1] = ok ? rd : bad;
      }
    }
  }
}

// where K^-1 lives for (no, nc): in LDS when it fits beside the vectors, unless MPCASM_QP_WIDE_KINV says
// otherwise ("lds": there whenever it fits; "global": always in d_kinv)
bool wide_kinv_on_chip(int no, int nc, bool soft) {
  const bool fits = (size_t)wide_lds(no, nc, true, soft).total * sizeof(double) <= (size_t)RESIDENT_LDS_LIMIT;
  const char* env = getenv("MPCASM_QP_WIDE_KINV");
  if (env != nullptr && strcmp(env, "global") == 0) return false;
  if (env != nullptr && strcmp(env, "lds") == 0) return fits;
  return fits;
}

template <int NCH, bool ONCHIP>
int launch_wide(const QpBatch& b, const QpSolve& s, size_t lds, hipStream_t stream, hipError_t* err) {
  return launch_with_lds(admm_wide_kernel<NCH, ONCHIP>, (unsigned)b.batch, QP_BLOCK, lds, stream, err, b.no, b.nc,
                         b.P, b.q, b.G, b.h, b.x, b.y, b.z, s.res, s.sigma, s.alpha, s.max_iter, s.warm, b.batch,
                         s.kinv, s.kinv_valid, static_cast<const SolveArgs&>(s));
}

template <int NCH, bool ONCHIP>
int launch_wide_soft(const QpBatch& b, const QpSolve& s, const QpSoft& soft, size_t lds, hipStream_t stream,
                     hipError_t* err) {
  SoftSolveArgs sa;
  static_cast<SolveArgs&>(sa) = s;
  sa.soft = soft;
  return launch_with_lds(admm_wide_kernel<NCH, ONCHIP, SoftSolveArgs>, (unsigned)b.batch, QP_BLOCK, lds, stream, err,
                         b.no, b.nc, b.P, b.q, b.G, b.h, b.x, b.y, b.z, s.res, s.sigma, s.alpha, s.max_iter, s.warm,
                         b.batch, s.kinv, s.kinv_valid, sa);
}

int wide_info(int no, int nc, bool soft, int64_t* lds_bytes, int32_t* kinv_on_chip) {
  const bool on = no <= WIDE_MAX_NO && wide_kinv_on_chip(no, nc, soft);
  const size_t lds = (size_t)wide_lds(no, nc, on, soft).total * sizeof(double);
  if (lds_bytes) *lds_bytes = (int64_t)lds;
  if (kinv_on_chip) *kinv_on_chip = on ? 1 : 0;
  return no > WIDE_MAX_NO || lds > (size_t)RESIDENT_LDS_LIMIT ? MPCASM_ERR_LIMIT : MPCASM_OK;
}

}  // namespace

int qp_solve_wide_info(int no, int nc, int64_t* lds_bytes, int32_t* kinv_on_chip) {
  return wide_info(no, nc, false, lds_bytes, kinv_on_chip);
}
int qp_solve_wide_soft_info(int no, int nc, int64_t* lds_bytes, int32_t* kinv_on_chip) {
  return wide_info(no, nc, true, lds_bytes, kinv_on_chip);
}

int launch_qp_solve_wide(const QpBatch& b, const QpSolve& s, hipStream_t stream, hipError_t* err) {
  int64_t lds = 0;
  int32_t on = 0;
  const int rc = qp_solve_wide_info(b.no, b.nc, &lds, &on);
  if (rc != MPCASM_OK) return rc;
  if (!on && s.kinv == nullptr) return MPCASM_ERR_ARG;   // (d_kinv is the factorisation's workspace)
  // the instantiation: K^-1's home, and the columns a lane holds
  using Launch = int (*)(const QpBatch&, const QpSolve&, size_t, hipStream_t, hipError_t*);
  static const Launch table[2][4] = {
      {launch_wide<1, true>, launch_wide<2, true>, launch_wide<4, true>, launch_wide<8, true>},
      {launch_wide<1, false>, launch_wide<2, false>, launch_wide<4, false>, launch_wide<8, false>}};
  return table[on ? 0 : 1][b.no <= 64 ? 0 : b.no <= 128 ? 1 : b.no <= 256 ? 2 : 3](b, s, (size_t)lds, stream, err);
}

int launch_qp_solve_wide_soft(const QpBatch& b, const QpSolve& s, const QpSoft& soft, hipStream_t stream,
                              hipError_t* err) {
  int64_t lds = 0;
  int32_t on = 0;
  const int rc = qp_solve_wide_soft_info(b.no, b.nc, &lds, &on);
  if (rc != MPCASM_OK) return rc;
  if (!on && s.kinv == nullptr) return MPCASM_ERR_ARG;   // (d_kinv is the factorisation's workspace)
  using Launch = int (*)(const QpBatch&, const QpSolve&, const QpSoft&, size_t, hipStream_t, hipError_t*);
  static const Launch table[2][4] = {
      {launch_wide_soft<1, true>, launch_wide_soft<2, true>, launch_wide_soft<4, true>, launch_wide_soft<8, true>},
      {launch_wide_soft<1, false>, launch_wide_soft<2, false>, launch_wide_soft<4, false>,
       launch_wide_soft<8, false>}};
  return table[on ? 0 : 1][b.no <= 64 ? 0 : b.no <= 128 ? 1 : b.no <= 256 ? 2 : 3](b, s, soft, (size_t)lds, stream,
                                                                                    err);
}

}  // namespace mpcasm
