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
// both with qp_prims.h's in-LDS code (admm.hip's, as a function), both factors inverted column by column (T = L^-1, Ts = Ls^-1).  With
// W = G_A T' (so that S = W W' + delta I) a solve of (K + dK) [dx; dy] = [r1; r2] is six matrix-vector products
//     u = T r1;  w = W u - r2;  v = Ts w;  dy = Ts' v;  s = u - W' dy;  dx = T' s
// every sum cut over the four wavefronts, none a dependent chain longer than a row.  LDS per instance: four
// matrices of no (no | 1) doubles -- Pd -> L -> W;  T;  G_A -> Ts;  S -> Ls -- and the vectors: see polish_lds.
// The residuals (of the iterate passed in, of every refinement step and of the polished point) read P and G
// from memory, a wavefront per row, the lanes along it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "polish_core.h"
#include "sens_core.h"

namespace mpcasm {

namespace {

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
  L.pa = L.gx + nc;         // [QP_WAVES][no] partial sums
  L.red = L.pa + QP_WAVES * no;   // 16 doubles: reductions and verdicts
  L.idx = L.red + 16;       // no int32: the active rows, ascending
  L.total = L.idx + (no + 1) / 2;
  L.total += L.total & 1;
  return L;
}

// wavefront `wave`'s quarter of out = M v (TRANS: M'v), M [.][ld]: pa[wave][c], c < n_out, over the terms
// wave, wave + 4, ... < n_sum
template <bool TRANS>
__device__ __forceinline__ void mv_part(const double* M, int ld, int n_out, int n_sum, const double* v,
                                        double* pa, int lp, int lane, int wave) {
  const int terms = n_sum > wave ? (n_sum - wave + QP_WAVES - 1) / QP_WAVES : 0;
  for (int c = lane; c < n_out; c += 64)
    pa[wave * lp + c] = TRANS ? pdot(M + wave * ld + c, QP_WAVES * ld, v + wave, QP_WAVES, terms)
                              : pdot(M + c * ld + wave, QP_WAVES, v + wave, QP_WAVES, terms);
}

// polish_core.h's backend with everything in LDS: the four matrices of polish_lds and the six-product solve
struct LdsPolish {
  PolishVecs v;
  double *M1, *T, *M3, *M4, *ws;
  int no, ld, tid, lane, wave;
  double delta;

  __device__ __forceinline__ LdsPolish(double* sm, int no_, int nc, double delta_, int tid_, int lane_, int wave_)
      : no(no_), tid(tid_), lane(lane_), wave(wave_), delta(delta_) {
    const PolishLds L = polish_lds(no, nc);
    ld = L.ld;
    M1 = sm + L.m1, T = sm + L.m2, M3 = sm + L.m3, M4 = sm + L.m4, ws = sm + L.w;
    v = PolishVecs{sm + L.x, sm + L.ya, sm + L.r1, sm + L.r2, sm + L.u,  sm + L.s,  sm + L.q,  sm + L.d,
                   sm + L.h, sm + L.y,  sm + L.z,  sm + L.gx, sm + L.pa, sm + L.red, reinterpret_cast<int*>(sm + L.idx)};
  }

  // T = (P + delta I)'s factor inverted, W = G_A T' in M1, Ts = the Schur complement's factor inverted in M3
  __device__ __forceinline__ bool build(const double* Pb, const double* Gb, int na) {
    const int* idx = v.idx;
    // ---- Pd = P + delta I and the active rows of G, on chip ---------------------------------------------------
    for (int e = tid; e < no * no; e += QP_BLOCK) {
      const int a = e / no, b = e - a * no;
      M1[a * ld + b] = Pb[e] + (a == b ? delta : 0.0);
    }
    for (int e = tid; e < na * no; e += QP_BLOCK) {
      const int a = e / no, c = e - a * no;
      M3[a * ld + c] = Gb[(size_t)idx[a] * no + c];
    }
    __syncthreads();
    bool good = cholesky_lds(M1, no, ld, tid, lane, wave);
    invert_lower_lds(M1, T, no, ld, tid);
    // ---- W = G_A T' over L (T is lower triangular: the sum ends at the diagonal) ------------------------------
    for (int e = tid; e < na * no; e += QP_BLOCK) {
      const int a = e / no, k = e - a * no;
      M1[a * ld + k] = pdot(M3 + a * ld, 1, T + k * ld, 1, k + 1);
    }
    __syncthreads();
    // ---- S = W W' + delta I, factored, the factor inverted over G_A ----------------------------------------------
    for (int e = tid; e < na * na; e += QP_BLOCK) {
      const int a = e / na, b = e - a * na;
      M4[a * ld + b] = pdot(M1 + a * ld, 1, M1 + b * ld, 1, no) + (a == b ? delta : 0.0);
    }
    __syncthreads();
    good = cholesky_lds(M4, na, ld, tid, lane, wave) && good;
    if (!good) return false;
    invert_lower_lds(M4, M3, na, ld, tid);
    return true;
  }

  // u = T r1;  w = W u - r2;  v = Ts w;  dy = Ts' v;  s = u - W' dy;  dx = T' s
  __device__ __forceinline__ void kkt_solve(int na) {
    const double *W = M1, *Ts = M3, *r1 = v.r1, *r2 = v.r2;
    double *us = v.dx, *ss = v.dy, *pa = v.pa;
    mv_part<false>(T, ld, no, no, r1, pa, no, lane, wave);
    __syncthreads();
    for (int c = tid; c < no; c += QP_BLOCK) us[c] = sum4(pa, no, c);            // u = T r1
    __syncthreads();
    mv_part<false>(W, ld, na, no, us, pa, no, lane, wave);
    __syncthreads();
    for (int a = tid; a < na; a += QP_BLOCK) ws[a] = sum4(pa, no, a) - r2[a];    // w = W u - r2
    __syncthreads();
    mv_part<false>(Ts, ld, na, na, ws, pa, no, lane, wave);
    __syncthreads();
    for (int a = tid; a < na; a += QP_BLOCK) ws[a] = sum4(pa, no, a);            // v = Ts w
    __syncthreads();
    mv_part<true>(Ts, ld, na, na, ws, pa, no, lane, wave);
    __syncthreads();
    for (int a = tid; a < na; a += QP_BLOCK) ss[a] = sum4(pa, no, a);            // dy = Ts' v
    __syncthreads();
    mv_part<true>(W, ld, no, na, ss, pa, no, lane, wave);
    __syncthreads();
    for (int c = tid; c < no; c += QP_BLOCK) us[c] -= sum4(pa, no, c);           // s = u - W' dy
    __syncthreads();
    mv_part<true>(T, ld, no, no, us, pa, no, lane, wave);
    __syncthreads();
    for (int c = tid; c < no; c += QP_BLOCK) us[c] = sum4(pa, no, c);            // dx = T' s
    __syncthreads();
  }
};

__global__ __launch_bounds__(QP_BLOCK) void polish_kernel(
    int no, int nc, const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ G,
    const double* __restrict__ h, double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Z,
    const int32_t* __restrict__ status, double delta, int refine_iters, int32_t* __restrict__ polish,
    double* __restrict__ res, int batch) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long inst = blockIdx.x;
  if (inst >= batch) return;
  LdsPolish be(sm, no, nc, delta, tid, lane, wave);
  const int verdict = polish_instance(be, inst, no, nc, P, q, G, h, X, Y, Z, status, refine_iters, res, tid, lane, wave);
  if (tid == 0) polish[inst] = verdict;
}

// mpcasm_qp_sens: sens_core.h's steps on the same back-end, the same LDS layout and the same geometry
__global__ __launch_bounds__(QP_BLOCK) void sens_kernel(QpSens s) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long inst = blockIdx.x;
  if (inst >= s.batch) return;
  LdsPolish be(sm, s.no, s.nc, s.delta, tid, lane, wave);
  const int verdict = sens_instance(be, inst, s, tid, lane, wave);
  if (tid == 0) s.verdict[inst] = verdict;
}

}  // namespace

size_t polish_lds_bytes(int no, int nc) { return (size_t)polish_lds(no, nc).total * sizeof(double); }

int launch_qp_polish(const QpBatch& b, const QpPolish& p, hipStream_t stream, hipError_t* err) {
  return launch_with_lds(polish_kernel, (unsigned)b.batch, QP_BLOCK, polish_lds_bytes(b.no, b.nc), stream, err,
                         b.no, b.nc, b.P, b.q, b.G, b.h, b.x, b.y, b.z, p.status, p.delta, p.refine_iters, p.polish,
                         p.res, b.batch);
}

int launch_qp_sens(const QpSens& s, hipStream_t stream, hipError_t* err) {
  return launch_with_lds(sens_kernel, (unsigned)s.batch, QP_BLOCK, polish_lds_bytes(s.no, s.nc), stream, err, s);
}

}  // namespace mpcasm
