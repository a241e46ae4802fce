// admm.hip -- K5: the step after the assembly, on the device (the "or"): a batch
// of dense QPs  min 1/2 x'Px + q'x  s.t.  Gx <= h  straight out of mpcasm_assemble's buffers, iterated
// with OSQP's ADMM -- the solve the reference's loop hands to qpsolvers.osqp_solve_qp
// (use_examples/simple_functional_example/biped_mpc_loop.py:57-60).  osqp is a third-party dependency
// of the example, absent from the reference tree; the iteration is the published one (Stellato,
// Banjac, Goulart, Bemporad, Boyd, Math. Prog. Comp. 12 (2020), Algorithm 1, reduced KKT form):
//     (P + sigma I + rho G'G) xt = sigma x - q + G'(rho z - y);   zt = G xt
//     x+ = alpha xt + (1 - alpha) x
//     z+ = min(alpha zt + (1 - alpha) z + y / rho, h);   y+ = y + rho (alpha zt + (1 - alpha) z - z+)
// restated on the CPU by oracle/admm_oracle.py, which the tests hold this kernel to.
//
// One workgroup of four wavefronts per instance, everything in LDS: the matrix K = P + sigma I + rho G'G is
// factored once (Cholesky, in place), inverted once (L^-1 column by column, every thread its own right-hand
// side; then K^-1 = L^-T L^-1), and an iteration is three matrix-vector products -- G'v, K^-1 r and G xt --
// with no dependent chain longer than a row: the two triangular solves per iteration that OSQP's LDL' does on
// the host would be 2 no dependent steps of a wavefront each.  K is symmetric positive definite by
// construction (sigma > 0), well conditioned for the steps OSQP uses; the explicit inverse changes the
// iterates by rounding only.  LDS per instance: no (no|1) doubles for K^-1, max(nc, no) (no|1) for G (and,
// before G is needed, L^-1), the vectors and the partial sums: 40 KB for the biped at N = 16 (no = 36,
// nc = 76): four instances per CU.
//
// The solve mode (mpcasm_qp_solve, admm_kernel<true>) is the same kernel with OSQP's stopping rules on top:
// every check_every iterations (and at the last) the instance tests "solved", "primal infeasible", "dual
// infeasible" in that order on the iterate and its step (l = -inf, u = h; infinity norms; no scaling), one
// decision per workgroup behind a barrier, and a finished workgroup retires.  Every adaptive_rho_interval
// iterations rho moves to OSQP's rho * sqrt((r_p / scale_p) / (r_d / scale_d)) when that is 5x off: K is formed,
// factored and inverted again in LDS with the same code.  The checks read P from global memory (it is not
// in LDS after K is formed) and use the partial-sum buffers as scratch: the layout is the same as the plain
// iteration's, so is the LDS an instance takes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "kernels.h"
#include "qp_prims.h"

namespace mpcasm {

namespace {

struct AdmmLds {
  int mi, gs, x, q, z, y, h, v, r, xt, pa, pb, sl, sq, total, ld, lp;
};
// soft: the soft instantiation's layout -- the same, with the two penalty vectors behind it
__host__ __device__ inline AdmmLds admm_lds(int no, int nc, bool soft = false) {
  AdmmLds L;
  L.ld = no | 1;   // (an odd leading dimension: a column of a row-major matrix is conflict-free)
  L.lp = no > nc ? no : nc;
  L.mi = 0;
  L.gs = L.mi + no * L.ld;
  L.x = L.gs + (nc > no ? nc : no) * L.ld;
  L.q = L.x + no;
  L.z = L.q + no;
  L.y = L.z + nc;
  L.h = L.y + nc;
  L.v = L.h + nc;                     // rho z - y
  L.r = L.v + nc;                     // the right-hand side
  L.xt = L.r + no;
  L.pa = L.xt + no;                   // [QP_WAVES][lp] partial sums of G'v, then of G xt
  L.pb = L.pa + QP_WAVES * L.lp;    // [QP_WAVES][no] partial sums of K^-1 r
  L.sl = L.pb + QP_WAVES * no;      // lin, quad [nc] (soft only)
  L.sq = L.sl + (soft ? nc : 0);
  L.total = L.sq + (soft ? nc : 0);
  L.total += L.total & 1;
  return L;
}

// One workgroup of four wavefronts per instance.  Everything that is a sum over rows or columns is cut in
// four -- wavefront w takes the terms i = w, w + 4, ... -- and the partial sums meet in LDS behind a barrier:
// one wavefront per instance (the first version) had nothing to hide an LDS round trip behind and spent
// 10 000 cycles per iteration on three matrix-vector products of 36 x 76.
// SOLVE: `iters` is max_iter, rho is the instance's s.rho[inst] and the loop ends at the first check that
// decides; the iterates of the plain iteration are the same as before.
// S = SoftSolveArgs: the soft instantiation (mpcasm_qp_solve_soft) -- the penalties loaded and tested beside h, the
// z update qp_soft_z, a soft row's dy left out of the primal certificate; nothing else differs.
template <bool SOLVE, typename S = SolveArgs>
__global__ __launch_bounds__(QP_BLOCK) void admm_kernel(
    int no, int nc, const double* __restrict__ P, const double* __restrict__ q,
    const double* __restrict__ G, const double* __restrict__ h, double* __restrict__ X,
    double* __restrict__ Y, double* __restrict__ Z, double* __restrict__ res, double rho, double sigma,
    double alpha, int iters, int warm, int batch, double* __restrict__ Kinv, int kinv_valid, S s) {
  constexpr bool SOFT = std::is_same<S, SoftSolveArgs>::value;
  static_assert(SOLVE || !SOFT, "soft rows are the solve mode's");
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long inst = blockIdx.x;
  if (inst >= batch) return;
  const AdmmLds L = admm_lds(no, nc, SOFT);
  const int ld = L.ld, lp = L.lp;
  double* Mi = sm + L.mi;   // K, then its Cholesky factor (lower), then K^-1
  double* Gs = sm + L.gs;   // G [nc][ld]; in between: T = L^-1 [no][ld]
  double* xs = sm + L.x;
  double* qs = sm + L.q;
  double* zs = sm + L.z;
  double* ys = sm + L.y;
  double* hs = sm + L.h;
  double* vs = sm + L.v;
  double* rv = sm + L.r;
  double* xt = sm + L.xt;
  double* pa = sm + L.pa;
  double* pbuf = sm + L.pb;
  double* sl = sm + L.sl;   // (SOFT only)
  double* sq = sm + L.sq;
  const double* Pb = P + (size_t)inst * no * no;
  const double* Gb = G + (size_t)inst * nc * no;
  auto load_g = [&]() {
    for (int e = tid; e < nc * no; e += QP_BLOCK) {
      const int r = e / no, c = e - r * no;
      Gs[r * ld + c] = Gb[e];
    }
  };

  // ---- K = P + sigma I + rho G'G ------------------------------------------------------------------
  // (a caller whose P and G did not change since the last call -- the same model and structure, a new
  // `given` -- hands K^-1 back in: no factorisation, the larger part of a call of 25 iterations)
  if constexpr (SOLVE) rho = s.rho[inst];
  const bool reuse = Kinv != nullptr && kinv_valid != 0;
  bool pen_bad = false;
  load_g();
  for (int e = tid; e < no; e += QP_BLOCK) {
    qs[e] = q[(size_t)inst * no + e];
    xs[e] = warm ? X[(size_t)inst * no + e] : 0.0;
  }
  for (int e = tid; e < nc; e += QP_BLOCK) {
    const double hv = h[(size_t)inst * nc + e];
    hs[e] = hv;
    ys[e] = warm ? Y[(size_t)inst * nc + e] : 0.0;
    zs[e] = warm ? Z[(size_t)inst * nc + e] : fmin(0.0, hv);   // (a cold start: z = min(G x, h) with x = 0)
    if constexpr (SOFT) {
      const double lv = s.soft.lin[inst * s.soft.stride + e], qv = s.soft.quad[inst * s.soft.stride + e];
      sl[e] = lv;
      sq[e] = qv;
      pen_bad = pen_bad || !qp_soft_valid(lv, qv);
    }
  }
  if constexpr (SOFT) {   // (one bad pair: the instance is not solved; pa is free until the iterations)
    const bool any = __ballot(pen_bad) != 0;
    if (lane == 0) pa[wave] = any ? 1.0 : 0.0;
  }
  __syncthreads();
  if constexpr (SOFT) pen_bad = (pa[0] + pa[1]) + (pa[2] + pa[3]) != 0.0;

  // K from G in LDS and P in memory, factored and inverted into Mi (false: K is not positive definite);
  // the solve mode calls it again when rho moves
  auto factor = [&]() -> bool {
    for (int e = tid; e < no * no; e += QP_BLOCK) {
      const int a = e / no, b = e - a * no;
      const double acc = dot4(Gs + a, ld, Gs + b, ld, nc, 0.0);
      Mi[a * ld + b] = fma(rho, acc, Pb[e]) + (a == b ? sigma : 0.0);
    }
    __syncthreads();
    bool good = true;
    // ---- Cholesky, in place (the lower triangle): K = L L' ----------------------------------------
    for (int k = 0; k < no; ++k) {
      const double dkk = Mi[k * ld + k];
      good = good && dkk > 0.0;
      const double d = sqrt(dkk > 0.0 ? dkk : 1.0);
      __syncthreads();
      for (int i = k + tid; i < no; i += QP_BLOCK) Mi[i * ld + k] = i == k ? d : Mi[i * ld + k] / d;
      __syncthreads();
      // the trailing block: wavefront w takes the rows k + 1 + w, + 4, ..., a lane the column k + 1 + lane
      // (+ 64, ... for more unknowns than lanes) up to the diagonal
      for (int j = k + 1 + lane; j < no; j += 64) {
        const double ljk = Mi[j * ld + k];
        for (int i = k + 1 + wave + (j > k + 1 + wave ? ((j - k - 1 - wave + QP_WAVES - 1) / QP_WAVES) * QP_WAVES : 0);
             i < no; i += QP_WAVES)
          Mi[i * ld + j] = fma(-Mi[i * ld + k], ljk, Mi[i * ld + j]);
      }
      __syncthreads();
    }
    // ---- T = L^-1: thread c solves L t = e_c (rows above c stay zero) --------------------------------
    double* T = Gs;
    for (int c = tid; c < no; c += QP_BLOCK)
      for (int i = 0; i < no; ++i) {
        const double sv = (i == c ? 1.0 : 0.0) - (i > c ? dot4(Mi + i * ld + c, 1, T + c * ld + c, ld, i - c, 0.0) : 0.0);
        T[i * ld + c] = i < c ? 0.0 : sv / Mi[i * ld + i];
      }
    __syncthreads();
    // ---- K^-1 = T' T ---------------------------------------------------------------------------------
    for (int e = tid; e < no * no; e += QP_BLOCK) {
      const int a = e / no, b = e - a * no;
      const int i0 = a > b ? a : b;
      Mi[a * ld + b] = dot4(T + i0 * ld + a, ld, T + i0 * ld + b, ld, no - i0, 0.0);
    }
    __syncthreads();
    if (Kinv != nullptr)
      for (int e = tid; e < no * no; e += QP_BLOCK)
        Kinv[(size_t)inst * no * no + e] = good ? Mi[(e / no) * ld + e % no] : __builtin_nan("");
    load_g();   // (the factorisation used G's place for L^-1)
    __syncthreads();
    return good;
  };

  bool ok = true;
  if (SOLVE && (!(rho > 0.0) || pen_bad)) {   // (no step to take: the solve calls the instance not convex)
    ok = false;
    if (Kinv != nullptr)
      for (int e = tid; e < no * no; e += QP_BLOCK) Kinv[(size_t)inst * no * no + e] = __builtin_nan("");
  } else if (reuse) {
    for (int e = tid; e < no * no; e += QP_BLOCK) Mi[(e / no) * ld + e % no] = Kinv[(size_t)inst * no * no + e];
    __syncthreads();
  } else {
    ok = factor();
  }

  // ---- the iterations: six short phases, a barrier behind each; every sum a strided inner product with
  // several reads in flight (dot4) -------------------------------------------------------------------------
  double inv_rho = 1.0 / rho;
  // wavefront w's share of a sum over `count` terms: i = w, w + 4, ...
  const int rows_w = nc > wave ? (nc - wave + QP_WAVES - 1) / QP_WAVES : 0;
  const int cols_w = no > wave ? (no - wave + QP_WAVES - 1) / QP_WAVES : 0;
  int status = ok ? MPCASM_QP_MAX_ITER : MPCASM_QP_NON_CVX, ran = ok ? iters : 0;
  for (int r = tid; r < nc; r += QP_BLOCK) vs[r] = fma(rho, zs[r], -ys[r]);
  __syncthreads();
  for (int it = 0; it < (SOLVE && !ok ? 0 : iters); ++it) {
    // (solve mode: a check after this iteration -- it keeps the step dx in pb, dy in pa)
    const int k = it + 1;
    const bool due = SOLVE && (k % s.check_every == 0 || k == iters);
    // pa[w][c] = sum over this wavefront's rows of G[r][c] v[r]
    for (int c = lane; c < no; c += 64)
      pa[wave * lp + c] = dot4(Gs + wave * ld + c, QP_WAVES * ld, vs + wave, QP_WAVES, rows_w, 0.0);
    __syncthreads();
    for (int b = tid; b < no; b += QP_BLOCK)
      rv[b] = fma(sigma, xs[b], -qs[b]) + ((pa[b] + pa[lp + b]) + (pa[2 * lp + b] + pa[3 * lp + b]));
    __syncthreads();
    // pb[w][c] = sum over this wavefront's b of K^-1[c][b] r[b]
    for (int c = lane; c < no; c += 64)
      pbuf[wave * no + c] = dot4(Mi + c * ld + wave, QP_WAVES, rv + wave, QP_WAVES, cols_w, 0.0);
    __syncthreads();
    for (int c = tid; c < no; c += QP_BLOCK) {
      const double xtc = (pbuf[c] + pbuf[no + c]) + (pbuf[2 * no + c] + pbuf[3 * no + c]);
      const double xo = xs[c], xn = fma(alpha, xtc, (1.0 - alpha) * xo);
      xt[c] = xtc;
      xs[c] = xn;
      if (due) pbuf[c] = xn - xo;   // (this thread's own column: no other thread reads it in this phase)
    }
    __syncthreads();
    // pa[w][r] = sum over this wavefront's c of G[r][c] xt[c]
    for (int r = lane; r < nc; r += 64)
      pa[wave * lp + r] = dot4(Gs + r * ld + wave, QP_WAVES, xt + wave, QP_WAVES, cols_w, 0.0);
    __syncthreads();
    for (int r = tid; r < nc; r += QP_BLOCK) {
      const double zt = (pa[r] + pa[lp + r]) + (pa[2 * lp + r] + pa[3 * lp + r]);
      const double zr = fma(alpha, zt, (1.0 - alpha) * zs[r]);
      double zn;
      if constexpr (SOFT) zn = qp_soft_z(fma(ys[r], inv_rho, zr), hs[r], rho, sl[r], sq + r);
      else zn = fmin(fma(ys[r], inv_rho, zr), hs[r]);
      const double yo = ys[r], yn = fma(rho, zr - zn, yo);
      ys[r] = yn;
      zs[r] = zn;
      vs[r] = fma(rho, zn, -yn);
      // (dy projected on the normal cone of (-inf, h]; a soft row has none: its y climbing to lin is no certificate)
      if (due) pa[r] = SOFT && qp_soft_row(sl[r]) ? 0.0 : fmax(yn - yo, 0.0);
    }
    __syncthreads();
    if constexpr (SOLVE) {
      if (due) {
        // one wavefront per test, each over all rows or columns: the verdicts need no partial sums
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = -INFINITY;
        if (wave == 0) {          // r_p = |Gx - z|, its scale max(|Gx|, |z|)
          for (int r = lane; r < nc; r += 64) {
            const double gx = dot4(Gs + r * ld, 1, xs, 1, no, 0.0);
            a0 = fmax(a0, fabs(gx - zs[r]));
            a1 = fmax(a1, fmax(fabs(gx), fabs(zs[r])));
          }
        } else if (wave == 1) {   // r_d = |Px + q + G'y|, its scale max(|Px|, |G'y|, |q|)
          for (int c = lane; c < no; c += 64) {
            const double px = dot4(Pb + (size_t)c * no, 1, xs, 1, no, 0.0);
            const double gty = dot4(Gs + c, ld, ys, 1, nc, 0.0);
            a0 = fmax(a0, fabs(px + qs[c] + gty));
            a1 = fmax(a1, fmax(fabs(px), fmax(fabs(gty), fabs(qs[c]))));
          }
        } else if (wave == 2) {   // |dy|, h'dy, |G'dy|
          for (int r = lane; r < nc; r += 64) {
            a0 = fmax(a0, pa[r]);
            a1 = fma(hs[r], pa[r], a1);
          }
          for (int c = lane; c < no; c += 64) a2 = fmax(a2, fabs(dot4(Gs + c, ld, pa, 1, nc, 0.0)));
        } else {                  // |dx|, q'dx, |P dx|, max(G dx)
          for (int c = lane; c < no; c += 64) {
            a0 = fmax(a0, fabs(pbuf[c]));
            a1 = fma(qs[c], pbuf[c], a1);
            a2 = fmax(a2, fabs(dot4(Pb + (size_t)c * no, 1, pbuf, 1, no, 0.0)));
          }
          for (int r = lane; r < nc; r += 64) a3 = fmax(a3, dot4(Gs + r * ld, 1, pbuf, 1, no, 0.0));
        }
        for (int off = 32; off > 0; off >>= 1) {
          const double b1 = __shfl_xor(a1, off, 64);
          a0 = fmax(a0, __shfl_xor(a0, off, 64));
          a1 = wave >= 2 ? a1 + b1 : fmax(a1, b1);
          a2 = fmax(a2, __shfl_xor(a2, off, 64));
          a3 = fmax(a3, __shfl_xor(a3, off, 64));
        }
        __syncthreads();   // (dx and dy read: their places take the verdicts)
        if (lane == 0) {
          if (wave == 0) pa[0] = a0, pa[1] = a1;
          else if (wave == 1) pa[2] = a0, pa[3] = a1;
          else if (wave == 2)
            pbuf[0] = qp_primal_infeasible(s, a0, a1, a2) ? 1.0 : 0.0;
          else
            pbuf[1] = qp_dual_infeasible(s, a0, a1, a2, a3) ? 1.0 : 0.0;
        }
        __syncthreads();
        const double rp = pa[0], sp = pa[1], rd = pa[2], sd = pa[3];
        const int verdict = qp_verdict(s, rp, sp, rd, sd, pbuf[0] != 0.0, pbuf[1] != 0.0);
        const double rn = qp_next_rho(s, rho, verdict, k, iters, rp, sp, rd, sd);
        __syncthreads();   // (the verdicts read by every thread: the next phase writes over them)
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
          for (int r = tid; r < nc; r += QP_BLOCK) vs[r] = fma(rho, zs[r], -ys[r]);
          __syncthreads();
        }
      }
    }
  }
  if constexpr (SOLVE) {
    if (tid == 0) {
      s.rho[inst] = rho;
      s.status[inst] = status;
      s.iters[inst] = ran;
    }
  }

  // ---- results; OSQP's residuals |Gx - z|_inf, |Px + q + G'y|_inf -------------------------------
  const double bad = __builtin_nan("");
  for (int c = tid; c < no; c += QP_BLOCK) X[(size_t)inst * no + c] = ok ? xs[c] : bad;
  for (int r = tid; r < nc; r += QP_BLOCK) {
    Y[(size_t)inst * nc + r] = ok ? ys[r] : bad;
    Z[(size_t)inst * nc + r] = ok ? zs[r] : bad;
  }
  if (res != nullptr) {
    double rp = 0.0, rd = 0.0;
    for (int r = tid; r < nc; r += QP_BLOCK) rp = fmax(rp, fabs(dot4(Gs + r * ld, 1, xs, 1, no, 0.0) - zs[r]));
    for (int c = tid; c < no; c += QP_BLOCK) {
      double acc = qs[c];
      for (int b = 0; b < no; ++b) acc = fma(Pb[(size_t)c * no + b], xs[b], acc);
      rd = fmax(rd, fabs(dot4(Gs + c, ld, ys, 1, nc, acc)));
    }
    for (int off = 32; off > 0; off >>= 1) {
      rp = fmax(rp, __shfl_xor(rp, off, 64));
      rd = fmax(rd, __shfl_xor(rd, off, 64));
    }
    if (lane == 0) {
      pbuf[wave] = rp;
      pbuf[QP_WAVES + wave] = rd;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < QP_WAVES; ++w) {
        rp = fmax(rp, pbuf[w]);
        rd = fmax(rd, pbuf[QP_WAVES + w]);
      }
      res[inst * 2 + 0] = ok ? rp : bad;
      res[inst * 2 + 1] = ok ? rd : bad;
    }
  }
}

}  // namespace

size_t admm_lds_bytes(int no, int nc) { return (size_t)admm_lds(no, nc).total * sizeof(double); }

int launch_admm(const QpBatch& b, double rho, const QpSolve& s, hipStream_t stream, hipError_t* err) {
  return launch_with_lds(admm_kernel<false>, (unsigned)b.batch, QP_BLOCK, admm_lds_bytes(b.no, b.nc), stream, err,
                         b.no, b.nc, b.P, b.q, b.G, b.h, b.x, b.y, b.z, s.res, rho, s.sigma, s.alpha, s.max_iter,
                         s.warm, b.batch, s.kinv, s.kinv_valid, SolveArgs{});
}

int launch_qp_solve(const QpBatch& b, const QpSolve& s, hipStream_t stream, hipError_t* err) {
  // (the solve mode's scratch lies in the same layout)
  return launch_with_lds(admm_kernel<true>, (unsigned)b.batch, QP_BLOCK, admm_lds_bytes(b.no, b.nc), stream, err,
                         b.no, b.nc, b.P, b.q, b.G, b.h, b.x, b.y, b.z, s.res, 0.0, s.sigma, s.alpha, s.max_iter,
                         s.warm, b.batch, s.kinv, s.kinv_valid, static_cast<const SolveArgs&>(s));
}

size_t admm_soft_lds_bytes(int no, int nc) { return (size_t)admm_lds(no, nc, true).total * sizeof(double); }

int launch_qp_solve_soft(const QpBatch& b, const QpSolve& s, const QpSoft& soft, hipStream_t stream, hipError_t* err) {
  SoftSolveArgs sa;
  static_cast<SolveArgs&>(sa) = s;
  sa.soft = soft;
  return launch_with_lds(admm_kernel<true, SoftSolveArgs>, (unsigned)b.batch, QP_BLOCK, admm_soft_lds_bytes(b.no, b.nc),
                         stream, err, b.no, b.nc, b.P, b.q, b.G, b.h, b.x, b.y, b.z, s.res, 0.0, s.sigma, s.alpha,
                         s.max_iter, s.warm, b.batch, s.kinv, s.kinv_valid, sa);
}

}  // namespace mpcasm
