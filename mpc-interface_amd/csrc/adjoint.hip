// adjoint.hip -- the derivative of the assembly with respect to `given`, matrix-free.
//
// P and G do not depend on `given`; q and h are affine in it (generate_qp_cost body.py:266-302,
// generate_qp_constraint body.py:236-264).  With V = E Bm the workspace rows (E: the row program
// OFF_ROWPTR / OFF_ENTBASE / OFF_ENTK / DOFF_ENTCOEF, Bm: the base rows read through the column
// tables, as preview_direct_kernel reads them), split over the columns V = [V_g | V_o]:
//   J_q = sum over non-diagonal gterms  s w V_o[a : a+n]' V_g[dd : dd+n]        (s = 1/2 under GT_FLAG_HALF)
//   J_h = - sum over axes  diag(arrow_i) V_g[rows_i]
// One kernel, templated on the direction, applies J = [J_q ; J_h] or J' to one instance per trip
// of a workgroup, everything between the inputs and the result in LDS:
//   JVP  d -> dq, dh          y = Bm_g d,  r = E y,  dh_R = - sum_i arrow_Ri r[row_i(R)],
//                             rho[a+k] += s w r[dd+k],  yt = E' rho,  dq = Bm_o' yt
//   VJP  gq, gh -> ggiven     y = Bm_o gq, r = E y,  rho[dd+k] += s w r[a+k],
//                             rho[row_i(R)] -= arrow_Ri gh_R,  yt = E' rho,  ggiven = Bm_g' yt
// No floating-point atomics and no scatter: every sum is gathered by the thread that owns the
// result, in an order fixed by the plan alone, through a transposed index (the CSC of E, per rho
// row its contributions, per column the base variables that cover it) that the host derives from the
// plan's tables once (adjoint_build_index) and that is kept with the plan handle.
//
// Further down, the derivative with respect to the parameters (mpcasm_assemble_params_vjp): the same first two
// steps three times, then a gather per parameter slot through a parameter index (params_adjoint_build_index).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "device_common.h"
#include "device_prims.h"
#include "kernels.h"

namespace mpcasm {

namespace {

constexpr int BLOCK = 256;
constexpr int NSTREAM = T_SID_CONST + 1;

__device__ __forceinline__ int sext24(int x) { return (x << 8) >> 8; }

struct AdjointArgs {
  const double* params;   // [batch][nparams]
  const double* in_x;     // JVP: d [batch][ng];  VJP: gq [batch][no] or nullptr (a zero cotangent)
  const double* in_h;     // VJP: gh [batch][nc] or nullptr
  double* out_x;          // JVP: dq [batch][no] or nullptr (skipped);  VJP: ggiven [batch][ng]
  double* out_h;          // JVP: dh [batch][nc] or nullptr
  int batch;
};

// Steps 1 and 2, shared by the two kernels of this unit: the workspace rows applied to a vector over the unknowns
// (OPT) or over `given`,  y = Bm_in x  (every base row over those columns only), then  r = E y.  `x` and the stream
// bases are in LDS and visible; `r` is visible to the workgroup on return, `y` is scratch.
template <bool OPT>
__device__ __forceinline__ void workspace_rows(const PlanDev& p, const AdjointView& v, const double* const* s_base,
                                               const double* x, double* y, double* r, int tid) {
  const int ng = p.ng, rtot = p.rtot, nbrow = p.t_nbrow;
  const int32_t* brow0 = p.itab + p.off_t_brow0;
  const int2* cig = reinterpret_cast<const int2*>(p.itab + p.off_t_cig);
  const int2* cio = reinterpret_cast<const int2*>(p.itab + p.off_t_cio);
  const int32_t* bcolptr = p.itab + p.off_t_bcolptr;
  const int32_t* bcols = p.itab + p.off_t_bcols;
  const int32_t* rowptr = p.itab + p.off_rowptr;
  const int32_t* entbase = p.itab + p.off_entbase;
  const int32_t* entk = p.itab + p.off_entk;
  const double* coef = p.dtab + p.doff_entcoef;
  const int32_t* rowbase = v.idx + v.rowbase;
  const int32_t* bsplit = v.idx + v.bsplit;
  const int in0 = OPT ? ng : 0;
  for (int t = tid; t < nbrow; t += BLOCK) {
    const int b = rowbase[t];
    const int k = t - brow0[b];
    const int i0 = OPT ? bsplit[b] : bcolptr[b], i1 = OPT ? bcolptr[b + 1] : bsplit[b];
    const int2* row = OPT ? cio + (size_t)b * p.t_nop - ng : cig + (size_t)b * ng;
    double acc = 0.0;
    for (int i = i0; i < i1; ++i) {
      const int c = bcols[i];
      const int2 ci = row[c];
      acc = fma(s_base[(unsigned)ci.y >> 24][(long)ci.x + (long)k * sext24(ci.y)], x[c - in0], acc);
    }
    y[t] = acc;
  }
  __syncthreads();
  for (int w = tid; w < rtot; w += BLOCK) {
    double acc = 0.0;
    for (int e = rowptr[w]; e < rowptr[w + 1]; ++e) acc = fma(coef[e], y[brow0[entbase[e]] + entk[e]], acc);
    r[w] = acc;
  }
  __syncthreads();
}

// Dynamic LDS (doubles, every part rounded up to even):
//   x   [max(ng, no)]  the direction d / the cotangent gq            dead after step 1
//   gh  [nc]           the cotangent of h (VJP; unused by the JVP, whose dh leaves from registers)
//   y   [base rows]    step 1;  yt of step 5 takes its place: y is dead once r = E y is done
//   r   [RTOT]         step 2
//   rho [RTOT]         steps 3, 4 (r is still read while rho is written: no overlay)
//   stream bases [NSTREAM]
template <bool VJP>
__global__ __launch_bounds__(BLOCK) void assemble_adjoint_kernel(PlanDev p, SrcTable src, AdjointView v,
                                                                 AdjointArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x;
  const int ng = p.ng, no = p.no, nc = p.nc, rtot = p.rtot, nbrow = p.t_nbrow;
  double* x = lds + v.o_x;
  double* gh = lds + v.o_gh;
  double* y = lds + v.o_y;
  double* r = lds + v.o_r;
  double* rho = lds + v.o_rho;
  const double** s_base = reinterpret_cast<const double**>(lds + v.o_bases);
  const int32_t* brow0 = p.itab + p.off_t_brow0;
  const int2* cig = reinterpret_cast<const int2*>(p.itab + p.off_t_cig);
  const int2* cio = reinterpret_cast<const int2*>(p.itab + p.off_t_cio);
  const double* coef = p.dtab + p.doff_entcoef;
  const int32_t* et_ptr = v.idx + v.et_ptr;
  const int2* et_ent = reinterpret_cast<const int2*>(v.idx + v.et_ent);
  const int32_t* rc_ptr = v.idx + (VJP ? v.rv_ptr : v.rj_ptr);
  const int2* rc_ent = reinterpret_cast<const int2*>(v.idx + (VJP ? v.rv_ent : v.rj_ent));
  const int32_t* cb_ptr = v.idx + v.cb_ptr;
  const int32_t* cb_ent = v.idx + v.cb_ent;
  // the columns the direction comes in on and the columns the result goes out on
  const int nin = VJP ? no : ng;
  const int nout = VJP ? ng : no, out0 = VJP ? 0 : ng;
  const bool has_x = VJP ? a.in_x != nullptr : true;          // (VJP: gq given)
  const bool has_h = VJP ? a.in_h != nullptr : a.out_h != nullptr;
  const bool want_x = VJP ? true : a.out_x != nullptr;        // (JVP: dq wanted)
  const int lanes = VJP ? v.lanes_v : v.lanes_j;              // threads per column of step 6
  const int groups = BLOCK / lanes;

  for (long inst = blockIdx.x; inst < a.batch; inst += gridDim.x) {
    const double* pb = a.params + inst * p.nparams;
    if (has_x)
      for (int c = tid; c < nin; c += BLOCK) x[c] = a.in_x[inst * nin + c];
    if (VJP && has_h)
      for (int R = tid; R < nc; R += BLOCK) gh[R] = a.in_h[inst * nc + R];
    if (tid < NSTREAM) {
      const double* b = p.dtab;
      if (tid < T_SID_CONST && tid < p.nsrc) b = src.ptr[tid] + inst * src.stride[tid];
      s_base[tid] = b;
    }
    __syncthreads();
    // 1. y = Bm_in x: every base row over the columns of the direction only
    // 2. r = E y
    if (has_x) workspace_rows<VJP>(p, v, s_base, x, y, r, tid);
    // 3. (JVP) dh_R = - sum over axes arrow_Ri r[row_i(R)]
    if (!VJP && has_h) {
      const int32_t* rowlimit = p.itab + p.off_rowlimit;
      for (int R = tid; R < nc; R += BLOCK) {
        const int32_t* lm = p.itab + p.off_limit + rowlimit[R] * LM_WORDS;
        const int l = R - lm[LM_OUT0];
        const int naxes = lm[LM_NAXES];
        const int32_t* lx = p.itab + p.off_lax + lm[LM_LAX0] * LX_WORDS;
        const double* arrow = pb + lm[LM_ARROW_P] + (lm[LM_ARROW_ROWS] == 1 ? 0 : l) * naxes;
        double acc = 0.0;
        for (int ax = 0; ax < naxes; ++ax) {
          const int rr = lx[ax * LX_WORDS + LX_ROWS] == 1 ? 0 : l;
          acc = fma(arrow[ax], r[lx[ax * LX_WORDS + LX_ROWOFF] + rr], acc);
        }
        a.out_h[inst * nc + R] = -acc;
      }
    }
    if (want_x) {
      // 3., 4. rho: per row its contributions, gathered.  An entry is (source | flags, parameter slot):
      // a gterm's s w r[source], or (VJP) a limit axis' - arrow gh[source]
      for (int w = tid; w < rtot; w += BLOCK) {
        double acc = 0.0;
        for (int e = rc_ptr[w]; e < rc_ptr[w + 1]; ++e) {
          const int2 ce = rc_ent[e];
          const int s = ce.x & ADJ_SRC_MASK;
          if (ce.x & ADJ_LIMIT) {
            if (VJP && has_h) acc = fma(-pb[ce.y], gh[s], acc);
          } else if (has_x) {
            const double sw = (ce.x & ADJ_HALF) ? 0.5 * pb[ce.y] : pb[ce.y];
            acc = fma(sw, r[s], acc);
          }
        }
        rho[w] = acc;
      }
      __syncthreads();
      // 5. yt = E' rho: a thread per base row walks the column of E (yt in y's place)
      for (int t = tid; t < nbrow; t += BLOCK) {
        double acc = 0.0;
        for (int e = et_ptr[t]; e < et_ptr[t + 1]; ++e) {
          const int2 ee = et_ent[e];
          acc = fma(coef[ee.y], rho[ee.x], acc);
        }
        y[t] = acc;
      }
      __syncthreads();
      // 6. out = Bm_out' yt: `lanes` threads per column, each a strided share of the rows of every base
      // variable that covers the column, then a butterfly over the group -- the same order whatever the batch
      double* o = a.out_x + inst * nout;
      const int grp = tid / lanes, l = tid - grp * lanes;
      for (int c0 = 0; c0 < nout; c0 += groups) {
        const int c = c0 + grp;
        double acc = 0.0;
        if (c < nout) {
          const int cc = out0 + c;
          for (int i = cb_ptr[cc]; i < cb_ptr[cc + 1]; ++i) {
            const int b = cb_ent[i];
            const int2 ci = VJP ? cig[(size_t)b * ng + cc] : cio[(size_t)b * p.t_nop + c];
            const double* s = s_base[(unsigned)ci.y >> 24] + ci.x;
            const long rs = sext24(ci.y);
            const int t0 = brow0[b], nb = brow0[b + 1] - t0;
            for (int k = l; k < nb; k += lanes) acc = fma(s[k * rs], y[t0 + k], acc);
          }
        }
        for (int off = lanes >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, lanes);
        if (l == 0 && c < nout) o[c] = acc;
      }
    }
    __syncthreads();
  }
}

// ---- the derivative with respect to the parameters (mpcasm_assemble_params_vjp) --------------------------------
// P, q, G, h are sums of outer products of workspace rows times a parameter, and the cotangent that a solve's
// sensitivity stands for is of rank two:  gP = -1/2 (u x' + x u'),  gq = -u,  gG_R = -(y_R u' + w_R x'),  gh = w.
// So the gradient of every parameter is a short sum of products of entries of three row vectors
//   r_x = V_o x,   r_u = V_o u,   r_g = V_g given                        (steps 1 and 2 above, three times)
// and neither the dense cotangents nor a row of V are ever formed.  Step 3 gathers: the group of lanes that owns a
// parameter slot walks the slot's records (ParamsView), each lane a strided share of a record's rows, then a
// butterfly over the group -- an order fixed by the plan alone.
struct ParamsAdjointArgs {
  const double* params;     // [batch][nparams]
  const double* given;      // [batch][ng] or nullptr (ng == 0)
  const double *x, *u;      // [batch][no]
  const double *y, *w;      // [batch][nc]: y zero off the active set
  const int32_t* verdict;   // [batch] or nullptr: an instance that is not MPCASM_SENS_DONE gets a zero row
  double* gparams;          // [batch][nparams]
  int batch;
};

// Dynamic LDS (doubles, every part rounded up to even):
//   x, u [no] each | given [ng] | y, w [nc] each | base rows (scratch of steps 1, 2) | r_x, r_u, r_g [RTOT] each |
//   stream bases [NSTREAM]
__global__ __launch_bounds__(BLOCK) void assemble_params_adjoint_kernel(PlanDev p, SrcTable src, AdjointView v,
                                                                        ParamsView pv, ParamsAdjointArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x;
  const int ng = p.ng, no = p.no, nc = p.nc, rtot = p.rtot, np = p.nparams;
  double* x = lds + pv.o_x;
  double* u = lds + pv.o_u;
  double* g = lds + pv.o_g;
  double* yy = lds + pv.o_y;
  double* ww = lds + pv.o_w;
  double* yb = lds + pv.o_yb;
  double* rx = lds + pv.o_rx;
  double* ru = lds + pv.o_ru;
  double* rg = lds + pv.o_rg;
  const double** s_base = reinterpret_cast<const double**>(lds + pv.o_bases);
  const int32_t* sl_ptr = pv.idx + pv.sl_ptr;
  const int4* sl_rec = reinterpret_cast<const int4*>(pv.idx + pv.sl_rec);
  const int lanes = pv.lanes, groups = BLOCK / lanes;
  const int grp = tid / lanes, l = tid - grp * lanes;

  for (long inst = blockIdx.x; inst < a.batch; inst += gridDim.x) {
    double* o = a.gparams + inst * np;
    if (a.verdict && a.verdict[inst] != MPCASM_SENS_DONE) {   // (none of its vectors is read: they may hold NaN)
      for (int s = tid; s < np; s += BLOCK) o[s] = 0.0;
      continue;
    }
    const double* pb = a.params + inst * np;
    for (int c = tid; c < no; c += BLOCK) x[c] = a.x[inst * no + c], u[c] = a.u[inst * no + c];
    for (int c = tid; c < ng; c += BLOCK) g[c] = a.given[inst * ng + c];
    for (int R = tid; R < nc; R += BLOCK) yy[R] = a.y[inst * nc + R], ww[R] = a.w[inst * nc + R];
    if (tid < NSTREAM) {
      const double* b = p.dtab;
      if (tid < T_SID_CONST && tid < p.nsrc) b = src.ptr[tid] + inst * src.stride[tid];
      s_base[tid] = b;
    }
    __syncthreads();
    // 1., 2. the three row vectors
    workspace_rows<true>(p, v, s_base, x, yb, rx, tid);
    workspace_rows<true>(p, v, s_base, u, yb, ru, tid);
    if (ng) {
      workspace_rows<false>(p, v, s_base, g, yb, rg, tid);
    } else {
      for (int w = tid; w < rtot; w += BLOCK) rg[w] = 0.0;
      __syncthreads();
    }
    // 3. the gather: a record is two int4, (kind | flags, rows, f0, f1), (f2, f3, f4, f5)
    for (int s0 = 0; s0 < np; s0 += groups) {
      const int slot = s0 + grp;
      double acc = 0.0;
      if (slot < np) {
        for (int e = sl_ptr[slot]; e < sl_ptr[slot + 1]; ++e) {
          const int4 h0 = sl_rec[2 * e], h1 = sl_rec[2 * e + 1];
          const int n = h0.y;
          const double s = (h0.x & PA_HALF) ? 0.5 : 1.0;
          switch (h0.x & PA_KIND_MASK) {
            case PA_GT_WEIGHT: {   // rows a = f0, b = f1 (under PA_P), d rows f2, the aim's slot f3
              const int ra = h0.z, rb = h0.w, rd = h1.x;
              const double aim = pb[h1.y];
              const bool hess = (h0.x & PA_P) != 0;
              for (int k = l; k < n; k += lanes) {
                double t = 0.0;
                if (hess) t = -0.5 * fma(ru[ra + k], rx[rb + k], rx[ra + k] * ru[rb + k]);
                acc += fma(-s * ru[ra + k], rg[rd + k] - aim, t);
              }
            } break;
            case PA_GT_AIM: {      // rows a = f0, the weight's slot f1
              double part = 0.0;
              for (int k = l; k < n; k += lanes) part += ru[h0.z + k];
              acc = fma(s * pb[h0.w], part, acc);
            } break;
            case PA_DIAG_WEIGHT: { // first column f0, coefficients at dtab[f1], the aim's slot f2
              const double* cf = p.dtab + h0.w;
              const double aim = pb[h1.x];
              for (int k = l; k < n; k += lanes) {
                const int c = h0.z + k;
                acc = fma(cf[k] * u[c], fma(-cf[k], x[c], aim), acc);
              }
            } break;
            case PA_DIAG_AIM: {    // first column f0, coefficients at dtab[f1], the weight's slot f2
              const double* cf = p.dtab + h0.w;
              double part = 0.0;
              for (int k = l; k < n; k += lanes) part = fma(cf[k], u[h0.z + k], part);
              acc = fma(pb[h1.x], part, acc);
            } break;
            case PA_LIMIT_ARROW: { // lines from R = f0, workspace rows f1 + k f2, the centre's slots f3 + k f4
              for (int k = l; k < n; k += lanes) {
                const int R = h0.z + k, row = h0.w + k * h1.x;
                const double t = -fma(yy[R], ru[row], ww[R] * rx[row]);
                acc += fma(ww[R], pb[h1.y + k * h1.z] - rg[row], t);
              }
            } break;
            case PA_LIMIT_CENTER:  // lines from R = f0, the arrow's slots f1 + k f2
              for (int k = l; k < n; k += lanes) acc = fma(ww[h0.z + k], pb[h0.w + k * h1.x], acc);
              break;
            default:               // PA_LIMIT_EXTREME: lines from R = f0
              for (int k = l; k < n; k += lanes) acc += ww[h0.z + k];
              break;
          }
        }
      }
      for (int off = lanes >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, lanes);
      if (l == 0 && slot < np) o[slot] = acc;
    }
    __syncthreads();
  }
}

int even(int n) { return n + (n & 1); }

}  // namespace

// The transposed index of a plan and the launch's geometry -- the one function both the launches and
// mpcasm_assemble_adjoint_info decide with.  MPCASM_ERR_LIMIT: a plan compiled with ltv= (no horizon tables:
// its adjoint is the sweep's backward recursion), a plan the column tables do not cover, or one instance beyond
// the LDS a workgroup can have; MPCASM_ERR_PLAN: a gterm or a limit axis that points outside the workspace
// (the checker holds plans to that already; the index is not built on trust).
int adjoint_build_index(const PlanDev& p, const int32_t* h, AdjointIndex* out) {
  if (p.sw_ok || !p.t_ci_ok) return MPCASM_ERR_LIMIT;
  const int ng = p.ng, no = p.no, W = ng + no, nbrow = p.t_nbrow, rtot = p.rtot;
  if (rtot > ADJ_SRC_MASK || p.nc > ADJ_SRC_MASK) return MPCASM_ERR_LIMIT;
  const int32_t* brow0 = h + p.off_t_brow0;
  const int32_t* bcolptr = h + p.off_t_bcolptr;
  const int32_t* bcols = h + p.off_t_bcols;
  const int32_t* rowptr = h + p.off_rowptr;
  const int32_t* entbase = h + p.off_entbase;
  const int32_t* entk = h + p.off_entk;
  if (brow0[p.nbase] != nbrow) return MPCASM_ERR_PLAN;
  std::vector<int32_t>& w = out->words;
  w.clear();
  AdjointView& v = out->view;
  v = AdjointView{};
  auto section = [&](size_t n, bool pairs) {
    if (pairs && (w.size() & 1)) w.push_back(0);   // (int2 reads)
    const int at = (int)w.size();
    w.resize(w.size() + n, 0);
    return at;
  };
  // the base variable of every base row; per base variable where its unknowns begin among its columns
  v.rowbase = section(nbrow, false);
  for (int b = 0; b < p.nbase; ++b) {
    if (brow0[b] < 0 || brow0[b + 1] < brow0[b] || brow0[b + 1] > nbrow) return MPCASM_ERR_PLAN;
    for (int t = brow0[b]; t < brow0[b + 1]; ++t) w[v.rowbase + t] = b;
  }
  v.bsplit = section(p.nbase, false);
  std::vector<std::vector<int32_t>> cover(W);
  for (int b = 0; b < p.nbase; ++b) {
    int split = bcolptr[b + 1];
    for (int i = bcolptr[b]; i < bcolptr[b + 1]; ++i) {
      const int c = bcols[i];
      if (c < 0 || c >= W || (i > bcolptr[b] && c <= bcols[i - 1])) return MPCASM_ERR_PLAN;
      if (c >= ng && split == bcolptr[b + 1]) split = i;
      cover[c].push_back(b);
    }
    w[v.bsplit + b] = split;
  }
  // per column of [given | unknowns] the base variables that cover it
  v.cb_ptr = section(W + 1, false);
  {
    int n = 0;
    for (int c = 0; c < W; ++c) w[v.cb_ptr + c] = n, n += (int)cover[c].size();
    w[v.cb_ptr + W] = n;
    v.cb_ent = section(n, false);
    n = 0;
    for (int c = 0; c < W; ++c)
      for (int b : cover[c]) w[v.cb_ent + n++] = b;
  }
  // the CSC of E: per base row the (workspace row, entry) pairs that read it, by ascending row
  {
    std::vector<int> count(nbrow + 1, 0);
    const int nent = rowptr[rtot];
    for (int r = 0; r < rtot; ++r)
      for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) {
        const int b = entbase[e];
        if (b < 0 || b >= p.nbase || entk[e] < 0 || entk[e] >= brow0[b + 1] - brow0[b]) return MPCASM_ERR_PLAN;
        ++count[brow0[b] + entk[e] + 1];
      }
    for (int t = 0; t < nbrow; ++t) count[t + 1] += count[t];
    v.et_ptr = section(nbrow + 1, false);
    for (int t = 0; t <= nbrow; ++t) w[v.et_ptr + t] = count[t];
    v.et_ent = section(2 * (size_t)nent, true);
    std::vector<int> fill(count.begin(), count.end() - 1);
    for (int r = 0; r < rtot; ++r)
      for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) {
        const int at = fill[brow0[entbase[e]] + entk[e]]++;
        w[v.et_ent + 2 * at] = r;
        w[v.et_ent + 2 * at + 1] = e;
      }
  }
  // per rho row its contributions: (source | flags, parameter slot), gterms in the plan's order, then limits
  std::vector<std::vector<int32_t>> cj(rtot), cv(rtot);
  for (int g = 0; g < p.ngterm; ++g) {
    const int32_t* rec = h + p.off_gterm + g * GT_WORDS;
    if (rec[GT_FLAGS] & GT_FLAG_DIAG) continue;   // (does not depend on `given`)
    const int a = rec[GT_AOFF], dd = rec[GT_DOFF], n = rec[GT_NROWS];
    if (a < 0 || dd < 0 || n < 0 || a + n > rtot || dd + n > rtot || rec[GT_WPARAM] < 0 || rec[GT_WPARAM] >= p.nparams)
      return MPCASM_ERR_PLAN;
    const int32_t half = (rec[GT_FLAGS] & GT_FLAG_HALF) ? ADJ_HALF : 0;
    for (int k = 0; k < n; ++k) {
      cj[a + k].push_back((dd + k) | half), cj[a + k].push_back(rec[GT_WPARAM]);
      cv[dd + k].push_back((a + k) | half), cv[dd + k].push_back(rec[GT_WPARAM]);
    }
  }
  for (int l = 0; l < p.nlimit; ++l) {
    const int32_t* lm = h + p.off_limit + l * LM_WORDS;
    const int naxes = lm[LM_NAXES];
    if (lm[LM_OUT0] < 0 || lm[LM_NROWS] < 0 || lm[LM_OUT0] + lm[LM_NROWS] > p.nc || naxes < 0 ||
        lm[LM_LAX0] < 0 || lm[LM_LAX0] + naxes > p.nlax)
      return MPCASM_ERR_PLAN;
    for (int i = 0; i < lm[LM_NROWS]; ++i)
      for (int ax = 0; ax < naxes; ++ax) {
        const int32_t* lx = h + p.off_lax + (lm[LM_LAX0] + ax) * LX_WORDS;
        const int row = lx[LX_ROWOFF] + (lx[LX_ROWS] == 1 ? 0 : i);
        const int slot = lm[LM_ARROW_P] + (lm[LM_ARROW_ROWS] == 1 ? 0 : i) * naxes + ax;
        if (row < 0 || row >= rtot || slot < 0 || slot >= p.nparams) return MPCASM_ERR_PLAN;
        cv[row].push_back((lm[LM_OUT0] + i) | ADJ_LIMIT), cv[row].push_back(slot);
      }
  }
  for (int dir = 0; dir < 2; ++dir) {
    const std::vector<std::vector<int32_t>>& c = dir ? cv : cj;
    const int ptr = section(rtot + 1, false);
    size_t n = 0;
    for (int r = 0; r < rtot; ++r) w[ptr + r] = (int32_t)(n / 2), n += c[r].size();
    w[ptr + rtot] = (int32_t)(n / 2);
    const int ent = section(n, true);
    n = 0;
    for (int r = 0; r < rtot; ++r)
      for (int32_t word : c[r]) w[ent + n++] = word;
    (dir ? v.rv_ptr : v.rj_ptr) = ptr;
    (dir ? v.rv_ent : v.rj_ent) = ent;
  }
  // threads per column of the last step: as many as keep the workgroup busy in one round
  auto lanes_for = [](int ncols) {
    int l = 1;
    while (l < 64 && 2 * l * std::max(ncols, 1) <= BLOCK) l *= 2;
    return l;
  };
  v.lanes_j = lanes_for(no);
  v.lanes_v = lanes_for(ng);
  v.o_x = 0;
  v.o_gh = v.o_x + even(std::max(ng, no));
  v.o_y = v.o_gh + even(p.nc);
  v.o_r = v.o_y + even(nbrow);
  v.o_rho = v.o_r + even(rtot);
  v.o_bases = v.o_rho + even(rtot);
  out->lds = ((size_t)v.o_bases + NSTREAM) * sizeof(double);
  if (out->lds > (size_t)RESIDENT_LDS_LIMIT) return MPCASM_ERR_LIMIT;
  out->per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (size_t)CU_LDS_BYTES / out->lds));
  return MPCASM_OK;
}

// `eff`: the launch's streams (launch_lti_tables has made the horizon tables of a plan compiled with lti=);
// `view.idx`: the device copy of the index
int launch_assemble_adjoint(const PlanDev& p, const SrcTable& eff, const AdjointIndex& index, bool vjp,
                            const double* params, const double* in_x, const double* in_h, double* out_x,
                            double* out_h, int batch, int num_cus, hipStream_t stream, hipError_t* err) {
  *err = hipSuccess;
  if (batch == 0) return MPCASM_OK;
  const unsigned grid = (unsigned)std::min<long>(batch, (long)num_cus * index.per_cu);
  const AdjointArgs a{params, in_x, in_h, out_x, out_h, batch};
  if (vjp)
    return launch_with_lds(assemble_adjoint_kernel<true>, grid, BLOCK, index.lds, stream, err, p, eff, index.view, a);
  return launch_with_lds(assemble_adjoint_kernel<false>, grid, BLOCK, index.lds, stream, err, p, eff, index.view, a);
}

// The parameter index of a plan and the geometry of mpcasm_assemble_params_vjp's launch -- the one function both the
// launch and mpcasm_assemble_params_vjp_info decide with.  Per parameter slot its records in a fixed order: the
// gterms in the plan's order, then the limits by line and axis.  A record covers the rows of one gterm or the lines
// of one limit axis that the slot is read on (one line where the field has a row per line, all of them where its one
// row is broadcast).  Every row and slot stored is checked again here (MPCASM_ERR_PLAN); MPCASM_ERR_LIMIT: one
// instance beyond the LDS a workgroup can have.  `p` has passed adjoint_build_index (the kernel reads its rowbase
// and bsplit).
int params_adjoint_build_index(const PlanDev& p, const int32_t* h, ParamsIndex* out) {
  if (p.sw_ok || !p.t_ci_ok) return MPCASM_ERR_LIMIT;
  const int ng = p.ng, no = p.no, nc = p.nc, rtot = p.rtot, np = p.nparams;
  std::vector<std::vector<int32_t>> recs(np);
  // (n slots from s0 on, `step` apart, step >= 0)
  const auto slot_ok = [np](long s0, long n, long step) { return s0 >= 0 && s0 < np && s0 + (n - 1) * step < np; };
  const auto rows_ok = [rtot](long r0, long n) { return r0 >= 0 && n >= 0 && r0 + n <= rtot; };
  const auto put = [&recs](int slot, int32_t kind, int n, int f0, int f1 = 0, int f2 = 0, int f3 = 0, int f4 = 0) {
    for (int32_t word : {kind, (int32_t)n, (int32_t)f0, (int32_t)f1, (int32_t)f2, (int32_t)f3, (int32_t)f4, 0})
      recs[slot].push_back(word);
  };
  for (int g = 0; g < p.ngterm; ++g) {
    const int32_t* rec = h + p.off_gterm + g * GT_WORDS;
    const int a = rec[GT_AOFF], b = rec[GT_BOFF], n = rec[GT_NROWS], wp = rec[GT_WPARAM], ap = rec[GT_AIMPARAM];
    if (n < 0 || !slot_ok(wp, 1, 0) || !slot_ok(ap, 1, 0)) return MPCASM_ERR_PLAN;
    if (rec[GT_FLAGS] & GT_FLAG_DIAG) {
      if (a < 0 || a + n > no || b < 0 || b + n > h[H_NDIAGCOEF]) return MPCASM_ERR_PLAN;
      put(wp, PA_DIAG_WEIGHT, n, a, p.doff_diagcoef + b, ap);
      put(ap, PA_DIAG_AIM, n, a, p.doff_diagcoef + b, wp);
      continue;
    }
    const int dd = rec[GT_DOFF];
    const bool hess = (rec[GT_FLAGS] & GT_FLAG_P) != 0;
    if (!rows_ok(a, n) || !rows_ok(dd, n) || (hess && !rows_ok(b, n))) return MPCASM_ERR_PLAN;
    const int32_t flags = ((rec[GT_FLAGS] & GT_FLAG_HALF) ? PA_HALF : 0) | (hess ? PA_P : 0);
    put(wp, PA_GT_WEIGHT | flags, n, a, hess ? b : 0, dd, ap);
    put(ap, PA_GT_AIM | flags, n, a, wp);
  }
  for (int li = 0; li < p.nlimit; ++li) {
    const int32_t* lm = h + p.off_limit + li * LM_WORDS;
    const int naxes = lm[LM_NAXES], nr = lm[LM_NROWS], out0 = lm[LM_OUT0];
    if (out0 < 0 || nr < 0 || out0 + nr > nc || naxes < 0 || lm[LM_LAX0] < 0 || lm[LM_LAX0] + naxes > p.nlax)
      return MPCASM_ERR_PLAN;
    const bool a1 = lm[LM_ARROW_ROWS] == 1, c1 = lm[LM_CENTER_ROWS] == 1, e1 = lm[LM_EXTREME_ROWS] == 1;
    if ((!a1 && lm[LM_ARROW_ROWS] != nr) || (!c1 && lm[LM_CENTER_ROWS] != nr) || (!e1 && lm[LM_EXTREME_ROWS] != nr))
      return MPCASM_ERR_PLAN;
    if (nr == 0) continue;
    // a line's slot of a field: first + (one row ? 0 : line) * step + axis
    const int astep = a1 ? 0 : naxes, cstep = c1 ? 0 : naxes;
    if (!slot_ok(lm[LM_EXTREME_P], nr, e1 ? 0 : 1)) return MPCASM_ERR_PLAN;
    for (int ax = 0; ax < naxes; ++ax)
      if (!slot_ok(lm[LM_ARROW_P] + ax, nr, astep) || !slot_ok(lm[LM_CENTER_P] + ax, nr, cstep)) return MPCASM_ERR_PLAN;
    // by line, then by axis: a field of one row takes all the lines in its one record, at line 0's place
    for (int i = 0; i < nr; ++i) {
      for (int ax = 0; ax < naxes; ++ax) {
        const int32_t* lx = h + p.off_lax + (lm[LM_LAX0] + ax) * LX_WORDS;
        const int rstep = lx[LX_ROWS] == 1 ? 0 : 1;
        if (lx[LX_ROWOFF] < 0 || lx[LX_ROWOFF] + (long)(nr - 1) * rstep >= rtot) return MPCASM_ERR_PLAN;
        const int arrow0 = lm[LM_ARROW_P] + ax, center0 = lm[LM_CENTER_P] + ax;
        if (a1 ? i == 0 : true) {
          const int first = a1 ? 0 : i, n = a1 ? nr : 1;
          put(arrow0 + first * astep, PA_LIMIT_ARROW, n, out0 + first, lx[LX_ROWOFF] + first * rstep, rstep,
              center0 + first * cstep, cstep);
        }
        if (c1 ? i == 0 : true) {
          const int first = c1 ? 0 : i, n = c1 ? nr : 1;
          put(center0 + first * cstep, PA_LIMIT_CENTER, n, out0 + first, arrow0 + first * astep, astep);
        }
      }
      if (e1 ? i == 0 : true) {
        const int first = e1 ? 0 : i, n = e1 ? nr : 1;
        put(lm[LM_EXTREME_P] + (e1 ? 0 : first), PA_LIMIT_EXTREME, n, out0 + first);
      }
    }
  }
  std::vector<int32_t>& w = out->words;
  w.clear();
  ParamsView& v = out->view;
  v = ParamsView{};
  v.sl_ptr = 0;
  w.resize((size_t)np + 1, 0);
  size_t nrec = 0;
  for (int s = 0; s < np; ++s) w[s] = (int32_t)nrec, nrec += recs[s].size() / PA_REC_WORDS;
  w[np] = (int32_t)nrec;
  while (w.size() & 3) w.push_back(0);   // (int4 reads)
  v.sl_rec = (int)w.size();
  for (int s = 0; s < np; ++s) w.insert(w.end(), recs[s].begin(), recs[s].end());
  // lanes per slot: as many as keep the workgroup busy in one round -- fixed by the plan, never by the batch
  v.lanes = 1;
  while (v.lanes < 64 && 2 * v.lanes * std::max(np, 1) <= BLOCK) v.lanes *= 2;
  v.o_x = 0;
  v.o_u = v.o_x + even(no);
  v.o_g = v.o_u + even(no);
  v.o_y = v.o_g + even(ng);
  v.o_w = v.o_y + even(nc);
  v.o_yb = v.o_w + even(nc);
  v.o_rx = v.o_yb + even(p.t_nbrow);
  v.o_ru = v.o_rx + even(rtot);
  v.o_rg = v.o_ru + even(rtot);
  v.o_bases = v.o_rg + even(rtot);
  out->lds = ((size_t)v.o_bases + NSTREAM) * sizeof(double);
  if (out->lds > (size_t)RESIDENT_LDS_LIMIT) return MPCASM_ERR_LIMIT;
  out->per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (size_t)CU_LDS_BYTES / out->lds));
  return MPCASM_OK;
}

// `adj`: the plan's transposed index on the device (its rowbase and bsplit are read); `index.view.idx`: the device
// copy of the parameter index
int launch_assemble_params_adjoint(const PlanDev& p, const SrcTable& eff, const AdjointIndex& adj,
                                   const ParamsIndex& index, const double* params, const double* given,
                                   const double* x, const double* u, const double* y, const double* w,
                                   const int32_t* verdict, double* gparams, int batch, int num_cus,
                                   hipStream_t stream, hipError_t* err) {
  *err = hipSuccess;
  if (batch == 0 || p.nparams == 0) return MPCASM_OK;
  const unsigned grid = (unsigned)std::min<long>(batch, (long)num_cus * index.per_cu);
  const ParamsAdjointArgs a{params, given, x, u, y, w, verdict, gparams, batch};
  return launch_with_lds(assemble_params_adjoint_kernel, grid, BLOCK, index.lds, stream, err, p, eff, adj.view,
                         index.view, a);
}

}  // namespace mpcasm
