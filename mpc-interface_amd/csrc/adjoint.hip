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
  const int32_t* bcolptr = p.itab + p.off_t_bcolptr;
  const int32_t* bcols = p.itab + p.off_t_bcols;
  const int32_t* rowptr = p.itab + p.off_rowptr;
  const int32_t* entbase = p.itab + p.off_entbase;
  const int32_t* entk = p.itab + p.off_entk;
  const double* coef = p.dtab + p.doff_entcoef;
  const int32_t* rowbase = v.idx + v.rowbase;
  const int32_t* bsplit = v.idx + v.bsplit;
  const int32_t* et_ptr = v.idx + v.et_ptr;
  const int2* et_ent = reinterpret_cast<const int2*>(v.idx + v.et_ent);
  const int32_t* rc_ptr = v.idx + (VJP ? v.rv_ptr : v.rj_ptr);
  const int2* rc_ent = reinterpret_cast<const int2*>(v.idx + (VJP ? v.rv_ent : v.rj_ent));
  const int32_t* cb_ptr = v.idx + v.cb_ptr;
  const int32_t* cb_ent = v.idx + v.cb_ent;
  // the columns the direction comes in on and the columns the result goes out on
  const int nin = VJP ? no : ng, in0 = VJP ? ng : 0;
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
    if (has_x) {
      for (int t = tid; t < nbrow; t += BLOCK) {
        const int b = rowbase[t];
        const int k = t - brow0[b];
        const int i0 = VJP ? bsplit[b] : bcolptr[b], i1 = VJP ? bcolptr[b + 1] : bsplit[b];
        const int2* row = VJP ? cio + (size_t)b * p.t_nop - ng : cig + (size_t)b * ng;
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

}  // namespace mpcasm
