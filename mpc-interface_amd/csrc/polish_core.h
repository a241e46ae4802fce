// polish_core.h -- the steps of K6 that polish.hip and polish_wide.hip take alike, written once: skip, load, the
// active set, the residuals of the iterate, the right-hand sides, the regularised KKT solve, the refinement against
// the K that is not regularised, the residuals of the polished point, the sign test and OSQP's rule, the write-back
// (include/mpcasm.h states them, tests/polish_restatement.py restates them).  The two kernels differ in how they
// solve  (K + dK) [dx; dy] = [r1; r2]  and where they keep what that takes; each hands polish_instance a backend:
//     v                        a PolishVecs: where the vectors of the steps live in its LDS
//     bool build(Pb, Gb, na)   the operators of the solve for the na active rows v.idx[0..na) of this instance
//                              (false: a matrix that must be positive definite is not)
//     void kkt_solve(na)       v.r1, v.r2 -> dx in v.dx, dy in v.dy
// One workgroup of QP_BLOCK threads per instance; every thread calls with the same arguments and gets the same
// verdict.
#pragma once
#include "qp_prims.h"

namespace mpcasm {

struct PolishVecs {
  double* x;     // [no] x^ (first: the iterate's x)
  double* ya;    // [no] y^ on the active rows, compact
  double* r1;    // [no] the right-hand sides
  double* r2;    // [no]
  double* dx;    // [no] the solve's results
  double* dy;    // [no]
  double* q;     // [no]
  double* d;     // [no] P x + q + G'y
  double* h;     // [nc]
  double* y;     // [nc] the iterate's y, then y^ on all rows
  double* z;     // [nc] the iterate's z
  double* gx;    // [nc] G x
  double* pa;    // [QP_WAVES][no] partial sums
  double* red;   // 16 doubles: reductions and verdicts
  int* idx;      // [no] the active rows, ascending
};

template <typename Backend>
__device__ __forceinline__ int polish_instance(Backend& be, long inst, int no, int nc, const double* __restrict__ P,
                                               const double* __restrict__ q, const double* __restrict__ G,
                                               const double* __restrict__ h, double* __restrict__ X,
                                               double* __restrict__ Y, double* __restrict__ Z,
                                               const int32_t* __restrict__ status, int refine_iters,
                                               double* __restrict__ res, int tid, int lane, int wave) {
  // (an instance that is not solved is not read at all: a NON_CVX one holds NaN)
  if (status != nullptr && status[inst] != MPCASM_QP_SOLVED) return MPCASM_POLISH_SKIPPED;
  const PolishVecs& v = be.v;
  double *xs = v.x, *ya = v.ya, *r1 = v.r1, *r2 = v.r2, *us = v.dx, *ss = v.dy, *qs = v.q, *ds = v.d, *hs = v.h;
  double *ys = v.y, *zs = v.z, *gx = v.gx, *pa = v.pa, *red = v.red;
  int* idx = v.idx;
  const double* Pb = P + (size_t)inst * no * no;
  const double* Gb = G + (size_t)inst * nc * no;
  double* Xb = X + (size_t)inst * no;
  double* Yb = Y + (size_t)inst * nc;
  double* Zb = Z + (size_t)inst * nc;
  for (int e = tid; e < no; e += QP_BLOCK) {
    qs[e] = q[(size_t)inst * no + e];
    xs[e] = Xb[e];
  }
  for (int e = tid; e < nc; e += QP_BLOCK) {
    hs[e] = h[(size_t)inst * nc + e];
    ys[e] = Yb[e];
    zs[e] = Zb[e];
  }
  __syncthreads();

  // ---- the active set: OSQP's test, the rows kept in ascending order (one wavefront, 64 rows a pass) ---------
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
  // kept in gx and ds: a wavefront per row of G and of P, the lanes along the row; G'y cut over the wavefronts
  // by rows, a lane a column (rows whose y is 0 are not read: most of them, for a polished point)
  auto residuals = [&](const double* zv, double* rp_out, double* rd_out) {
    rows_mv(Gb, no, nc, no, xs, gx, lane, wave);
    rows_mv(Pb, no, no, no, xs, ds, lane, wave);
    for (int c = lane; c < no; c += 64) {
      double s0 = 0.0, s1 = 0.0;
      int r = wave;
      for (; r + QP_WAVES < nc; r += 2 * QP_WAVES) {
        const double y0 = ys[r], y1 = ys[r + QP_WAVES];
        if (y0 != 0.0) s0 = fma(Gb[(size_t)r * no + c], y0, s0);
        if (y1 != 0.0) s1 = fma(Gb[(size_t)(r + QP_WAVES) * no + c], y1, s1);
      }
      if (r < nc && ys[r] != 0.0) s0 = fma(Gb[(size_t)r * no + c], ys[r], s0);
      pa[wave * no + c] = s0 + s1;
    }
    __syncthreads();
    double rp = 0.0, rd = 0.0;
    for (int c = tid; c < no; c += QP_BLOCK) {
      const double dv = (ds[c] + qs[c]) + sum4(pa, no, c);
      ds[c] = dv;
      rd = nmax(rd, fabs(dv));
    }
    for (int r = tid; r < nc; r += QP_BLOCK)
      rp = nmax(rp, fabs(gx[r] - (zv != nullptr ? zv[r] : fmin(gx[r], hs[r]))));
    rp = wave_nmax(rp), rd = wave_nmax(rd);
    if (lane == 0) {
      red[wave] = rp;
      red[QP_WAVES + wave] = rd;
    }
    __syncthreads();
    *rp_out = nmax(nmax(red[0], red[1]), nmax(red[2], red[3]));
    *rd_out = nmax(nmax(red[4], red[5]), nmax(red[6], red[7]));
    __syncthreads();   // (red and pa are free again)
  };

  // ---- r_p, r_d of the iterate passed in, then the operators of the solve ----------------------------------
  double rp_in, rd_in;
  residuals(zs, &rp_in, &rd_in);
  if (!be.build(Pb, Gb, na)) return MPCASM_POLISH_REJECTED;   // (a pivot that is not positive, a NaN among them)

  // ---- t0 = (K + dK)^-1 g, then the refinement against the K that is not regularised -------------------------
  for (int c = tid; c < no; c += QP_BLOCK) r1[c] = -qs[c];
  for (int a = tid; a < na; a += QP_BLOCK) r2[a] = hs[idx[a]];
  __syncthreads();
  be.kkt_solve(na);
  for (int c = tid; c < no; c += QP_BLOCK) xs[c] = us[c];
  for (int r = tid; r < nc; r += QP_BLOCK) ys[r] = 0.0;
  __syncthreads();
  for (int a = tid; a < na; a += QP_BLOCK) {
    ya[a] = ss[a];
    ys[idx[a]] = ss[a];
  }
  __syncthreads();
  double rp_hat, rd_hat;
  for (int it = 0; it < refine_iters; ++it) {
    residuals(nullptr, &rp_hat, &rd_hat);   // (gx = G x^ and ds = P x^ + q + G'y^ are what the step needs)
    for (int c = tid; c < no; c += QP_BLOCK) r1[c] = -ds[c];
    for (int a = tid; a < na; a += QP_BLOCK) r2[a] = hs[idx[a]] - gx[idx[a]];
    __syncthreads();
    be.kkt_solve(na);
    for (int c = tid; c < no; c += QP_BLOCK) xs[c] += us[c];
    for (int a = tid; a < na; a += QP_BLOCK) {
      const double yn = ya[a] + ss[a];
      ya[a] = yn;
      ys[idx[a]] = yn;
    }
    __syncthreads();
  }

  // ---- the polished point and the verdict ------------------------------------------------------------------
  residuals(nullptr, &rp_hat, &rd_hat);
  double neg = 0.0;
  for (int a = tid; a < na; a += QP_BLOCK) neg = ya[a] >= 0.0 ? neg : 1.0;   // (a NaN counts as negative)
  neg = wave_max(neg);
  if (lane == 0) red[8 + wave] = neg;
  __syncthreads();
  const bool signs = red[8] == 0.0 && red[9] == 0.0 && red[10] == 0.0 && red[11] == 0.0;
  const bool better = (rp_hat < rp_in && rd_hat < rd_in) || (rp_hat < rp_in && rd_in < 1e-10) ||
                      (rd_hat < rd_in && rp_in < 1e-10);
  if (!(better && signs)) return MPCASM_POLISH_REJECTED;
  for (int c = tid; c < no; c += QP_BLOCK) Xb[c] = xs[c];
  for (int r = tid; r < nc; r += QP_BLOCK) {
    Yb[r] = ys[r];
    Zb[r] = fmin(gx[r], hs[r]);
  }
  if (tid == 0 && res != nullptr) {
    res[inst * 2 + 0] = rp_hat;
    res[inst * 2 + 1] = rd_hat;
  }
  return MPCASM_POLISH_DONE;
}

}  // namespace mpcasm
