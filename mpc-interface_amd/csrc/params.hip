// params.hip -- the piece in front of a tick of a closed loop (mpcasm_params_map): per-walker commands become
// elements of the parameter rows the assembly of that tick reads, on the device, with nothing read back.
// include/mpcasm.h states the rule, tests/param_map_restatement.py restates it.
//
// A record is four int32 (dst, col, flags, 0) in `recs` and two doubles (c0, c1) in `coef`; it writes ONE element
// of every instance's row:   params[b][dst] = [c0 +] (c1 [* sign[b]]) * cmd[index[b]][col].
//
// params_map_kernel: one thread per (instance, record), grid-stride; neighbouring threads take neighbouring
// records of one instance, so the index, the sign and the command row of an instance are the same lines for all
// of them and the records (a few hundred bytes, shared by the launch) stay in cache.  No LDS, no scratch: at fleet
// sizes (4 096 x 18 eight-byte stores) the launch is what it costs.
// Every product and the sum are rounded on their own (contraction is off inside the kernel): a restatement in
// numpy matches bit for bit, and with c1 and the sign in {+1, -1} the element is the host's side * alt * xy exactly.
// A record that names an element outside the row, a column outside the commands or an unknown flag writes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace mpcasm {

namespace {

constexpr int PM_BLOCK = 256;
constexpr unsigned PM_MAX_GRID = 2048;   // (grid-stride beyond: eight workgroups for each of the chip's 256 CUs)

__global__ __launch_bounds__(PM_BLOCK) void params_map_kernel(
    double* __restrict__ params, long n_params, const int32_t* __restrict__ recs, const double* __restrict__ coef,
    int nrecs, const double* __restrict__ cmd, long cmd_stride, int ncmd, const int32_t* __restrict__ index,
    const double* __restrict__ sign, long total) {
#pragma clang fp contract(off)
  const long stride = (long)gridDim.x * PM_BLOCK;
  const bool narrow = total <= 0x7fffffffL;   // (one 32-bit division then)
  for (long i = (long)blockIdx.x * PM_BLOCK + threadIdx.x; i < total; i += stride) {
    long b;
    int r;
    if (narrow) {
      const unsigned q = (unsigned)i / (unsigned)nrecs;
      b = q;
      r = (int)((unsigned)i - q * (unsigned)nrecs);
    } else {
      b = i / nrecs;
      r = (int)(i - b * nrecs);
    }
    const int dst = recs[4 * r], col = recs[4 * r + 1], flags = recs[4 * r + 2];
    if (dst < 0 || dst >= n_params || col < 0 || col >= ncmd) continue;
    if ((flags & ~(MPCASM_PMAP_SIGNED | MPCASM_PMAP_CONST)) != 0) continue;
    if ((flags & MPCASM_PMAP_SIGNED) != 0 && sign == nullptr) continue;
    const long w = index ? (long)index[b] : b;
    const double c0 = coef[2 * r], c1 = coef[2 * r + 1];
    const double t = (flags & MPCASM_PMAP_SIGNED) ? c1 * sign[b] : c1;
    const double v = t * cmd[w * cmd_stride + col];
    params[b * n_params + dst] = (flags & MPCASM_PMAP_CONST) ? c0 + v : v;
  }
}

}  // namespace

int launch_params_map(double* params, int64_t n_params, const int32_t* recs, const double* coef, int nrecs,
                      const double* cmd, int64_t cmd_stride, int ncmd, const int32_t* index, const double* sign,
                      int batch, hipStream_t stream, hipError_t* err) {
  const long total = (long)batch * nrecs;
  const long blocks = (total + PM_BLOCK - 1) / PM_BLOCK;
  const unsigned grid = (unsigned)(blocks < (long)PM_MAX_GRID ? blocks : (long)PM_MAX_GRID);
  return launch_with_lds(params_map_kernel, grid, PM_BLOCK, 0, stream, err, params, (long)n_params, recs, coef, nrecs,
                         cmd, (long)cmd_stride, ncmd, index, sign, total);
}

}  // namespace mpcasm
