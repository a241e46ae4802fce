// feedback.hip -- pre-stabilised (closed-loop) prediction for a dynamics compiled as ltv: condensing over an
// unstable plant loses the Hessian's digits before any solver sees it ("The loop at C5"), so the input
// becomes u_k = K_k x_k + v_k, the unknowns become v, and sweep.hip / rollout.hip run unchanged on
//     A_cl_k = A_k + B_k K_k
// bound in A's source slot.  Four pieces:
//   ltv_lqr_kernel          the gains, by a backward Riccati sweep over each instance's own sequence -- once per loop
//   ltv_close_kernel        A_cl = A + B K for gains the caller brings -- once per loop
//   ltv_augment_kernel      the closed loop with the true input as a state, z = [x ; u_prev] -- once per loop
//   ltv_true_inputs_kernel  u_k = K_k x_k + v_k along x_{k+1} = A_cl_k x_k + B_k v_k -- every tick
//
// The sweep is a dependent chain of T steps per instance, so the batch is the parallelism: one lane per instance,
// the kernel instantiated for every (n, m) up to SW_NMAX x SW_MMAX so that P, Q, R and a step's matrices are
// registers (no LDS, no scratch: `make resources`), step k - 1's A and B asked for before step k's arithmetic.  A
// lane's loads and stores are runs of n n (n m) doubles a sequence apart from its neighbour's, not coalesced: the
// kernel runs once per loop and its time is recorded in profiles/ltv_feedback_bench.json.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <limits>

#include "device_common.h"
#include "kernels.h"

namespace mpcasm {

namespace {

constexpr int FB_BLOCK = 64;        // a wavefront: few instances are spread over many CUs
constexpr int FB_CLOSE_BLOCK = 256;

struct LqrArgs {
  const double* A;
  long long strideA;
  const double* B;
  long long strideB;
  const double* Q;
  const double* R;
  const double* PT;       // nullptr: Q
  double* K;
  double* Acl;            // nullptr: not wanted
  int32_t* info;
  int T, batch;
};

template <int R_, int C_>
__device__ __forceinline__ void load_block(double (&d)[R_][C_], const double* __restrict__ s) {
#pragma unroll
  for (int i = 0; i < R_; ++i)
#pragma unroll
    for (int j = 0; j < C_; ++j) d[i][j] = s[i * C_ + j];
}

// for k = T - 1 .. 0:  S = R + B^T P B (upper triangle, mirrored);  S = L L^T;  K = -S^-1 (B^T P A) by the two
// triangular solves;  A_cl = A + B K;  P <- Q + A^T (P A_cl);  P <- (P + P^T) / 2.  A pivot that is not positive
// (NaN included) ends the instance: info = k, NaN in the rows of step k and of every earlier step.
template <int NS, int MS>
__global__ __launch_bounds__(FB_BLOCK) void ltv_lqr_kernel(LqrArgs a) {
  const long b = (long)blockIdx.x * FB_BLOCK + threadIdx.x;
  if (b >= a.batch) return;
  const int T = a.T;
  const double* __restrict__ Ab = a.A + b * a.strideA;
  const double* __restrict__ Bb = a.B + b * a.strideB;
  double* __restrict__ Kb = a.K + b * (long)T * MS * NS;
  double* __restrict__ Cb = a.Acl ? a.Acl + b * (long)T * NS * NS : nullptr;
  double Q[NS][NS], R[MS][MS], P[NS][NS], An[NS][NS], Bn[NS][MS];
  load_block(An, Ab + (long)(T - 1) * NS * NS);
  load_block(Bn, Bb + (long)(T - 1) * NS * MS);
  load_block(Q, a.Q);
  load_block(R, a.R);
  load_block(P, a.PT ? a.PT : a.Q);
  int info = -1;
  for (int k = T - 1; k >= 0; --k) {
    double A[NS][NS], B[NS][MS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
#pragma unroll
      for (int j = 0; j < NS; ++j) A[i][j] = An[i][j];
#pragma unroll
      for (int j = 0; j < MS; ++j) B[i][j] = Bn[i][j];
    }
    if (k > 0) {      // step k - 1's matrices are in flight during step k's arithmetic
      load_block(An, Ab + (long)(k - 1) * NS * NS);
      load_block(Bn, Bb + (long)(k - 1) * NS * MS);
    }
    // 1. S = R + B^T (P B)
    double PB[NS][MS], S[MS][MS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
      for (int j = 0; j < MS; ++j) {
        double acc = P[i][0] * B[0][j];
#pragma unroll
        for (int s = 1; s < NS; ++s) acc = fma(P[i][s], B[s][j], acc);
        PB[i][j] = acc;
      }
#pragma unroll
    for (int i = 0; i < MS; ++i)
#pragma unroll
      for (int j = i; j < MS; ++j) {
        double acc = R[i][j];
#pragma unroll
        for (int s = 0; s < NS; ++s) acc = fma(B[s][i], PB[s][j], acc);
        S[i][j] = acc;
        S[j][i] = acc;
      }
    // 2. S = L L^T, by columns, L over S's lower triangle
    bool ok = true;
#pragma unroll
    for (int j = 0; j < MS; ++j) {
      double d = S[j][j];
#pragma unroll
      for (int t = 0; t < j; ++t) d = fma(-S[j][t], S[j][t], d);
      ok = ok && d > 0.0;
      d = sqrt(d);
      S[j][j] = d;
#pragma unroll
      for (int i = j + 1; i < MS; ++i) {
        double v = S[i][j];
#pragma unroll
        for (int t = 0; t < j; ++t) v = fma(-S[i][t], S[j][t], v);
        S[i][j] = v / d;
      }
    }
    if (!ok) {
      info = k;
      const double nan = std::numeric_limits<double>::quiet_NaN();
      for (int kk = k; kk >= 0; --kk) {
        for (int e = 0; e < MS * NS; ++e) Kb[(long)kk * MS * NS + e] = nan;
        if (Cb)
          for (int e = 0; e < NS * NS; ++e) Cb[(long)kk * NS * NS + e] = nan;
      }
      break;
    }
    // 3. K = -S^-1 ((P B)^T A): L Y = W, L^T X = Y
    double K[MS][NS];
#pragma unroll
    for (int j = 0; j < MS; ++j)
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        double acc = PB[0][j] * A[0][c];
#pragma unroll
        for (int s = 1; s < NS; ++s) acc = fma(PB[s][j], A[s][c], acc);
        K[j][c] = acc;
      }
#pragma unroll
    for (int c = 0; c < NS; ++c) {
#pragma unroll
      for (int i = 0; i < MS; ++i) {
        double v = K[i][c];
#pragma unroll
        for (int t = 0; t < i; ++t) v = fma(-S[i][t], K[t][c], v);
        K[i][c] = v / S[i][i];
      }
#pragma unroll
      for (int i = MS - 1; i >= 0; --i) {
        double v = K[i][c];
#pragma unroll
        for (int t = i + 1; t < MS; ++t) v = fma(-S[t][i], K[t][c], v);
        K[i][c] = v / S[i][i];
      }
#pragma unroll
      for (int i = 0; i < MS; ++i) K[i][c] = -K[i][c];
    }
    // 4. A_cl = A + B K
    double C[NS][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        double acc = A[i][c];
#pragma unroll
        for (int j = 0; j < MS; ++j) acc = fma(B[i][j], K[j][c], acc);
        C[i][c] = acc;
      }
#pragma unroll
    for (int j = 0; j < MS; ++j)
#pragma unroll
      for (int c = 0; c < NS; ++c) Kb[(long)k * MS * NS + j * NS + c] = K[j][c];
    if (Cb) {
#pragma unroll
      for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int c = 0; c < NS; ++c) Cb[(long)k * NS * NS + i * NS + c] = C[i][c];
    }
    // 5. P <- Q + A^T (P A_cl)
    double PA[NS][NS], Pn[NS][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        double acc = P[i][0] * C[0][c];
#pragma unroll
        for (int s = 1; s < NS; ++s) acc = fma(P[i][s], C[s][c], acc);
        PA[i][c] = acc;
      }
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        double acc = Q[i][c];
#pragma unroll
        for (int s = 0; s < NS; ++s) acc = fma(A[s][i], PA[s][c], acc);
        Pn[i][c] = acc;
      }
    // 6. P <- (P + P^T) / 2
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
      for (int c = 0; c < NS; ++c) P[i][c] = 0.5 * (Pn[i][c] + Pn[c][i]);
  }
  a.info[b] = info;
}

struct CloseArgs {
  const double* A;
  long long strideA;
  const double* B;
  long long strideB;
  const double* K;
  long long strideK, stepK;
  double* Acl;
  int n, m, T;
  long long total;        // batch T n n
};

// element e of A_cl (batch, T, n, n): a wavefront's stores are one contiguous run
__global__ __launch_bounds__(FB_CLOSE_BLOCK) void ltv_close_kernel(CloseArgs a) {
  const long long e = (long long)blockIdx.x * FB_CLOSE_BLOCK + threadIdx.x;
  if (e >= a.total) return;
  const int n = a.n, m = a.m;
  const long long r = e / n, kk = r / n, b = kk / a.T;
  const int j = (int)(e - r * n), i = (int)(r - kk * n), k = (int)(kk - b * a.T);
  const double* __restrict__ Ak = a.A + b * a.strideA + (long long)k * n * n;
  const double* __restrict__ Bk = a.B + b * a.strideB + (long long)k * n * m;
  const double* __restrict__ Kk = a.K + b * a.strideK + k * a.stepK;
  double acc = Ak[i * n + j];
  for (int s = 0; s < m; ++s) acc = fma(Bk[i * m + s], Kk[s * n + j], acc);
  a.Acl[e] = acc;
}

struct AugmentArgs {
  const double* A;
  long long strideA;
  const double* B;
  long long strideB;
  const double* K;
  long long strideK, stepK;
  double* At;
  double* Bt;
  double* Kt;             // nullptr: not wanted (then totalK = 0)
  int n, m, T;
  long long totalA;       // batch T (n + m) (n + m)
  long long totalB;       // batch T (n + m) m
  long long totalK;       // batch T m (n + m)
  unsigned blocksA, blocksB;
};

// The plant augmented by one delay, z_k = [x_k ; u_{k-1}] with u_k = K_k x_k + v_k:
//     At_k = [[A_k + B_k K_k, 0], [K_k, 0]]    Bt_k = [[B_k], [I]]    Kt_k = [K_k | 0]
// so that row k of the STATE u is z_{k+1}[n:] = K_k x_k + v_k, the true input.  One lane per output element; the
// workgroups of At come first, then Bt's, then Kt's (a workgroup lies in one of them: the branch is uniform), so
// a wavefront's stores are one contiguous run.  The A + B K block is summed as ltv_close_kernel sums it.
__global__ __launch_bounds__(FB_CLOSE_BLOCK) void ltv_augment_kernel(AugmentArgs a) {
  const int n = a.n, m = a.m, nz = n + m;
  const unsigned blk = blockIdx.x;
  if (blk < a.blocksA) {
    const long long e = (long long)blk * FB_CLOSE_BLOCK + threadIdx.x;
    if (e >= a.totalA) return;
    const long long r = e / nz, kk = r / nz, b = kk / a.T;
    const int j = (int)(e - r * nz), i = (int)(r - kk * nz), k = (int)(kk - b * a.T);
    double v = 0.0;
    if (j < n) {
      const double* __restrict__ Kk = a.K + b * a.strideK + k * a.stepK;
      if (i < n) {
        const double* __restrict__ Ak = a.A + b * a.strideA + (long long)k * n * n;
        const double* __restrict__ Bk = a.B + b * a.strideB + (long long)k * n * m;
        v = Ak[i * n + j];
        for (int s = 0; s < m; ++s) v = fma(Bk[i * m + s], Kk[s * n + j], v);
      } else {
        v = Kk[(i - n) * n + j];
      }
    }
    a.At[e] = v;
  } else if (blk < a.blocksA + a.blocksB) {
    const long long e = (long long)(blk - a.blocksA) * FB_CLOSE_BLOCK + threadIdx.x;
    if (e >= a.totalB) return;
    const long long r = e / m, kk = r / nz, b = kk / a.T;
    const int j = (int)(e - r * m), i = (int)(r - kk * nz), k = (int)(kk - b * a.T);
    double v;
    if (i < n)
      v = a.B[b * a.strideB + (long long)k * n * m + i * m + j];
    else
      v = i - n == j ? 1.0 : 0.0;
    a.Bt[e] = v;
  } else {
    const long long e = (long long)(blk - a.blocksA - a.blocksB) * FB_CLOSE_BLOCK + threadIdx.x;
    if (e >= a.totalK) return;
    const long long r = e / nz, kk = r / m, b = kk / a.T;
    const int j = (int)(e - r * nz), s = (int)(r - kk * m), k = (int)(kk - b * a.T);
    a.Kt[e] = j < n ? a.K[b * a.strideK + k * a.stepK + s * n + j] : 0.0;
  }
}

struct TrueArgs {
  const double* A;        // the closed-loop window the plan's sources hold
  long long strideA;
  const double* B;
  long long strideB;
  const double* K;
  long long strideK;
  const double* given;
  long long rows;
  const double* optim;
  const int32_t* index;   // nullptr: instance b is row b
  double* out;
  int count;
};

// lane (instance, axis): u_k = K_k x_k + v_k for k = 0 .. N - 1 along x_{k+1} = A_cl_k x_k + B_k v_k
template <int NS, int MS>
__global__ __launch_bounds__(FB_BLOCK) void ltv_true_inputs_kernel(PlanDev p, TrueArgs a) {
  const int naxes = p.sw_naxes, N = p.sw_horizon;
  const long w = (long)blockIdx.x * FB_BLOCK + threadIdx.x;
  if (w >= (long)a.count * naxes) return;
  const long b = w / naxes;
  const int ax = (int)(w - b * naxes);
  const long row = a.index ? (long)a.index[b] : b;
  if (row < 0 || row >= a.rows) return;       // (as the rollout: such an instance writes nothing)
  const int32_t* aw = p.itab + p.off_sw_axis + ax * SW_AXIS_WORDS;
  const double* __restrict__ Ab = a.A + b * a.strideA;
  const double* __restrict__ Bb = a.B + b * a.strideB;
  const double* __restrict__ Kb = a.K + b * a.strideK;
  const double* __restrict__ v = a.optim + b * p.no;
  double* __restrict__ out = a.out + w * N * MS;
  int ucol[MS];
#pragma unroll
  for (int j = 0; j < MS; ++j) ucol[j] = aw[1 + j];
  double x[NS], An[NS][NS], Bn[NS][MS], Kn[MS][NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) x[i] = a.given[row * p.ng + aw[0] + i];
  load_block(An, Ab);
  load_block(Bn, Bb);
  load_block(Kn, Kb);
  for (int k = 0; k < N; ++k) {
    double A[NS][NS], B[NS][MS], K[MS][NS], vk[MS], y[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
#pragma unroll
      for (int j = 0; j < NS; ++j) A[i][j] = An[i][j];
#pragma unroll
      for (int j = 0; j < MS; ++j) B[i][j] = Bn[i][j];
#pragma unroll
      for (int j = 0; j < MS; ++j) K[j][i] = Kn[j][i];
    }
    if (k + 1 < N) {
      load_block(An, Ab + (long)(k + 1) * NS * NS);
      load_block(Bn, Bb + (long)(k + 1) * NS * MS);
      load_block(Kn, Kb + (long)(k + 1) * MS * NS);
    }
#pragma unroll
    for (int j = 0; j < MS; ++j) {
      vk[j] = v[ucol[j] + k];
      double acc = vk[j];
#pragma unroll
      for (int i = 0; i < NS; ++i) acc = fma(K[j][i], x[i], acc);
      out[(long)k * MS + j] = acc;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      double acc = A[i][0] * x[0];
#pragma unroll
      for (int s = 1; s < NS; ++s) acc = fma(A[i][s], x[s], acc);
#pragma unroll
      for (int j = 0; j < MS; ++j) acc = fma(B[i][j], vk[j], acc);
      y[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) x[i] = y[i];
  }
}

// every (states, inputs) instantiation of a kernel family, [n - 1][m - 1]
#define MPCASM_FB_TABLE(K)                                \
  {{K<1, 1>, K<1, 2>, K<1, 3>, K<1, 4>},                  \
   {K<2, 1>, K<2, 2>, K<2, 3>, K<2, 4>},                  \
   {K<3, 1>, K<3, 2>, K<3, 3>, K<3, 4>},                  \
   {K<4, 1>, K<4, 2>, K<4, 3>, K<4, 4>}}
using LqrKernel = void (*)(LqrArgs);
using TrueInputsKernel = void (*)(PlanDev, TrueArgs);
constexpr LqrKernel lqr_kernels[SW_NMAX][SW_MMAX] = MPCASM_FB_TABLE(ltv_lqr_kernel);
constexpr TrueInputsKernel true_inputs_kernels[SW_NMAX][SW_MMAX] = MPCASM_FB_TABLE(ltv_true_inputs_kernel);
#undef MPCASM_FB_TABLE

}  // namespace

int launch_ltv_lqr(int n, int m, int T, int batch, const double* A, long long strideA, const double* B,
                   long long strideB, const double* Q, const double* R, const double* PT, double* K, double* Acl,
                   int32_t* info, hipStream_t stream, hipError_t* err) {
  *err = hipSuccess;
  if (n < 1 || n > SW_NMAX || m < 1 || m > SW_MMAX) return MPCASM_ERR_LIMIT;
  if (batch == 0) return MPCASM_OK;
  if (T == 0) {     // (no step: every instance went through)
    *err = hipMemsetAsync(info, 0xFF, (size_t)batch * sizeof(int32_t), stream);
    return *err == hipSuccess ? MPCASM_OK : MPCASM_ERR_HIP;
  }
  const LqrArgs a{A, strideA, B, strideB, Q, R, PT, K, Acl, info, T, batch};
  return launch_with_lds(lqr_kernels[n - 1][m - 1], (unsigned)((batch + FB_BLOCK - 1) / FB_BLOCK), FB_BLOCK, 0, stream,
                       err, a);
}

int launch_ltv_close(int n, int m, int T, int batch, const double* A, long long strideA, const double* B,
                     long long strideB, const double* K, long long strideK, long long stepK, double* Acl,
                     hipStream_t stream, hipError_t* err) {
  *err = hipSuccess;
  if (n < 1 || n > SW_NMAX || m < 1 || m > SW_MMAX) return MPCASM_ERR_LIMIT;
  const long long total = (long long)batch * T * n * n;
  if (total == 0) return MPCASM_OK;
  const long long blocks = (total + FB_CLOSE_BLOCK - 1) / FB_CLOSE_BLOCK;
  if (blocks > 0x7FFFFFFFLL) return MPCASM_ERR_LIMIT;
  const CloseArgs a{A, strideA, B, strideB, K, strideK, stepK, Acl, n, m, T, total};
  return launch_with_lds(ltv_close_kernel, (unsigned)blocks, FB_CLOSE_BLOCK, 0, stream, err, a);
}

int launch_ltv_augment(int n, int m, int T, int batch, const double* A, long long strideA, const double* B,
                       long long strideB, const double* K, long long strideK, long long stepK, double* At, double* Bt,
                       double* Kt, hipStream_t stream, hipError_t* err) {
  *err = hipSuccess;
  if (n < 1 || m < 1 || n + m > SW_NMAX || m > SW_MMAX) return MPCASM_ERR_LIMIT;
  const long long nz = n + m, steps = (long long)batch * T;
  const long long totalA = steps * nz * nz, totalB = steps * nz * m, totalK = Kt ? steps * m * nz : 0;
  if (steps == 0) return MPCASM_OK;
  const long long blocksA = (totalA + FB_CLOSE_BLOCK - 1) / FB_CLOSE_BLOCK;
  const long long blocksB = (totalB + FB_CLOSE_BLOCK - 1) / FB_CLOSE_BLOCK;
  const long long blocksK = (totalK + FB_CLOSE_BLOCK - 1) / FB_CLOSE_BLOCK;
  if (blocksA + blocksB + blocksK > 0x7FFFFFFFLL) return MPCASM_ERR_LIMIT;
  const AugmentArgs a{A, strideA, B, strideB, K, strideK, stepK, At, Bt, Kt, n, m, T, totalA, totalB, totalK,
                      (unsigned)blocksA, (unsigned)blocksB};
  return launch_with_lds(ltv_augment_kernel, (unsigned)(blocksA + blocksB + blocksK), FB_CLOSE_BLOCK, 0, stream, err, a);
}

int launch_ltv_true_inputs(const PlanDev& p, const SrcTable& src, const double* K, long long strideK,
                           const double* given, long long rows, const double* optim, const int32_t* index,
                           double* out, int count, hipStream_t stream, hipError_t* err) {
  *err = hipSuccess;
  const int n = p.sw_n, m = p.sw_m;
  if (n < 1 || n > SW_NMAX || m < 1 || m > SW_MMAX || p.sw_naxes < 1 || p.sw_naxes > SW_AXMAX)
    return MPCASM_ERR_LIMIT;
  if (count == 0) return MPCASM_OK;
  const TrueArgs a{src.ptr[p.sw_src_a], src.stride[p.sw_src_a], src.ptr[p.sw_src_b], src.stride[p.sw_src_b],
                   K, strideK, given, rows, optim, index, out, count};
  const long lanes = (long)count * p.sw_naxes;
  return launch_with_lds(true_inputs_kernels[n - 1][m - 1], (unsigned)((lanes + FB_BLOCK - 1) / FB_BLOCK), FB_BLOCK, 0,
                       stream, err, p, a);
}

}  // namespace mpcasm
