// sens_core.h -- the sensitivity of a solved QP, written once for the two polish back-ends (polish.hip's LdsPolish,
// polish_wide.hip's SlicePolish; polish_core.h says what a back-end is): at a strictly complementary solution with
// active rows A the KKT conditions are  P x + q + G_A'y_A = 0,  G_A x = h_A,  so both the forward and the adjoint
// derivative of (x, y) are one more solve with the polish's  K = [[P, G_A'], [G_A, 0]]  and a right-hand side of the
// caller's (include/mpcasm.h states the steps, tests/sens_restatement.py restates them, DESIGN.md derives the signs):
//     skip, the active set (the polish's test),  t = (K + dK)^-1 r  refined against the K that is not regularised,
//     u = t[:no], w = t[no:] scattered over the rows, |r - K t|_inf, and the rank-two gradients for P and G.
// Where the polish keeps q, r_d, y^ and x^ this keeps rx, t's two halves and the iterate; h's place holds ry on the
// active rows once the set is known, z's place the mark of an active row, G x's place w on all rows.  The residual
// reads P whole and of G the active rows only.
// One workgroup of QP_BLOCK threads per instance; every thread calls with the same arguments and gets the same
// verdict.  Nothing is written to memory before the verdict is MPCASM_SENS_DONE.
#pragma once
#include "polish_core.h"

namespace mpcasm {

template <typename Backend>
__device__ __forceinline__ int sens_instance(Backend& be, long inst, const QpSens& s, int tid, int lane, int wave) {
  // (an instance that is not solved is not read at all: a NON_CVX one holds NaN)
  if (s.status != nullptr && s.status[inst] != MPCASM_QP_SOLVED) return MPCASM_SENS_SKIPPED;
  const int no = s.no, nc = s.nc;
  const PolishVecs& v = be.v;
  double *xs = v.x, *ty = v.ya, *r1 = v.r1, *r2 = v.r2, *us = v.dx, *ss = v.dy, *rx = v.q, *tx = v.d, *hs = v.h;
  double *ys = v.y, *zs = v.z, *wf = v.gx, *pa = v.pa, *red = v.red;
  double *rya = v.h, *mark = v.z;
  int* idx = v.idx;
  const double* Pb = s.P + (size_t)inst * no * no;
  const double* Gb = s.G + (size_t)inst * nc * no;
  for (int e = tid; e < no; e += QP_BLOCK) {
    rx[e] = s.rx[(size_t)inst * no + e];
    xs[e] = s.x[(size_t)inst * no + e];
  }
  for (int e = tid; e < nc; e += QP_BLOCK) {
    hs[e] = s.h[(size_t)inst * nc + e];
    ys[e] = s.y[(size_t)inst * nc + e];
    zs[e] = s.z[(size_t)inst * nc + e];
  }
  __syncthreads();

  // ---- the active set: the polish's test, the rows kept in ascending order (one wavefront, 64 rows a pass) ----
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
  if (na > no) return MPCASM_SENS_SKIPPED;   // (more active rows than unknowns: no KKT system of full rank)

  // ---- ry on the active rows over h, the marks over z (both were read for the last time above) ----------------
  for (int r = tid; r < nc; r += QP_BLOCK) mark[r] = 0.0;
  for (int a = tid; a < na; a += QP_BLOCK) rya[a] = s.ry[(size_t)inst * nc + idx[a]];
  __syncthreads();
  for (int a = tid; a < na; a += QP_BLOCK) mark[idx[a]] = 1.0;
  if (!be.build(Pb, Gb, na)) return MPCASM_SENS_SINGULAR;   // (a pivot that is not positive, a NaN among them)

  // r - K t of tx, ty into r1, r2, and its infinity norm: P tx a wavefront per row; G_A tx a wavefront per active
  // row, four in flight; G_A'ty cut over the wavefronts by rows, a lane a column
  auto residual = [&]() -> double {
    rows_mv(Pb, no, no, no, tx, r1, lane, wave);
    for (int a0 = wave * QP_ROWS; a0 < na; a0 += QP_WAVES * QP_ROWS) {
      double acc[QP_ROWS];
#pragma unroll
      for (int u = 0; u < QP_ROWS; ++u) {
        acc[u] = 0.0;
        if (a0 + u < na) {
          const double* gr = Gb + (size_t)idx[a0 + u] * no;
          for (int c = lane; c < no; c += 64) acc[u] = fma(gr[c], tx[c], acc[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < QP_ROWS; ++u) acc[u] = wave_sum(acc[u]);
#pragma unroll
      for (int u = 0; u < QP_ROWS; ++u)
        if (lane == 0 && a0 + u < na) r2[a0 + u] = acc[u];
    }
    for (int c = lane; c < no; c += 64) {
      double s0 = 0.0, s1 = 0.0;
      int a = wave;
      for (; a + QP_WAVES < na; a += 2 * QP_WAVES) {
        s0 = fma(Gb[(size_t)idx[a] * no + c], ty[a], s0);
        s1 = fma(Gb[(size_t)idx[a + QP_WAVES] * no + c], ty[a + QP_WAVES], s1);
      }
      if (a < na) s0 = fma(Gb[(size_t)idx[a] * no + c], ty[a], s0);
      pa[wave * no + c] = s0 + s1;
    }
    __syncthreads();
    double m = 0.0;
    for (int c = tid; c < no; c += QP_BLOCK) {
      const double d = rx[c] - (r1[c] + sum4(pa, no, c));
      r1[c] = d;
      m = nmax(m, fabs(d));
    }
    for (int a = tid; a < na; a += QP_BLOCK) {
      const double d = rya[a] - r2[a];
      r2[a] = d;
      m = nmax(m, fabs(d));
    }
    m = wave_nmax(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = nmax(nmax(red[0], red[1]), nmax(red[2], red[3]));
    __syncthreads();   // (red and pa are free again)
    return m;
  };

  // ---- t = (K + dK)^-1 r, then the refinement against the K that is not regularised ---------------------------
  for (int c = tid; c < no; c += QP_BLOCK) r1[c] = rx[c];
  for (int a = tid; a < na; a += QP_BLOCK) r2[a] = rya[a];
  __syncthreads();
  be.kkt_solve(na);
  for (int c = tid; c < no; c += QP_BLOCK) tx[c] = us[c];
  for (int a = tid; a < na; a += QP_BLOCK) ty[a] = ss[a];
  __syncthreads();
  for (int it = 0; it < s.refine_iters; ++it) {
    residual();
    be.kkt_solve(na);
    for (int c = tid; c < no; c += QP_BLOCK) tx[c] += us[c];
    for (int a = tid; a < na; a += QP_BLOCK) ty[a] += ss[a];
    __syncthreads();
  }
  const double lres = residual();

  // ---- u, w on all rows, the residual -------------------------------------------------------------------------
  for (int r = tid; r < nc; r += QP_BLOCK) wf[r] = 0.0;
  __syncthreads();
  for (int a = tid; a < na; a += QP_BLOCK) wf[idx[a]] = ty[a];
  __syncthreads();
  for (int c = tid; c < no; c += QP_BLOCK) s.u[(size_t)inst * no + c] = tx[c];
  for (int r = tid; r < nc; r += QP_BLOCK) s.w[(size_t)inst * nc + r] = wf[r];
  if (tid == 0 && s.lres != nullptr) s.lres[inst] = lres;

  // ---- the dense gradients, whole, the lanes along the rows: -1/2 (u x' + x u') (the same expression either side
  // of the diagonal, so the same bits) and -(y_i u' + w_i x') on the active rows -----------------------------------
  if (s.gP != nullptr) {
    double* gP = s.gP + (size_t)inst * no * no;
    for (int i = wave; i < no; i += QP_WAVES) {
      const double ui = tx[i], xi = xs[i];
      for (int j = lane; j < no; j += 64) {
        const bool low = i < j;   // (the smaller index first)
        const double ua = low ? ui : tx[j], xa = low ? xi : xs[j], ub = low ? tx[j] : ui, xb = low ? xs[j] : xi;
        gP[(size_t)i * no + j] = -0.5 * fma(ua, xb, xa * ub);
      }
    }
  }
  if (s.gG != nullptr) {
    double* gG = s.gG + (size_t)inst * nc * no;
    for (int i = wave; i < nc; i += QP_WAVES) {
      const bool act = mark[i] != 0.0;
      const double yi = ys[i], wi = wf[i];
      for (int j = lane; j < no; j += 64) gG[(size_t)i * no + j] = act ? -fma(yi, tx[j], wi * xs[j]) : 0.0;
    }
  }
  return MPCASM_SENS_DONE;
}

}  // namespace mpcasm
