// jit.h -- the persistent kernel specialised per plan by hiprtc (jit.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "kernels.h"

namespace mpcasm {

// "plan_spec.h" of a plan: its sizes and trip lists as constants
// (seg_limit: most runs a chunk of a fetch table may have to be fetched by arithmetic, at most FS_MAX)
std::string jit_spec_header(const PlanDev& d, const int32_t* h_itab, int seg_limit = FS_MAX);
// the fetch tables as runs per chunk: [kind, chunk, runs, runs x FS_WORDS] ... (jit.hip)
std::vector<int32_t> jit_fetch_plan(const PlanDev& d, const int32_t* h_itab, int seg_limit);
// resident.hip + that header -> gfx950 code object (needs libhiprtc.so, no device)
// (phases >= 0: the phase mask as a constant of the build; -1: the kernel argument)
int jit_compile(const std::string& header, std::vector<char>* code, std::string* log,
                bool stamps = false, int phases = 0xBF);
// the compiled kernel of (plan structure, device), or nullptr: use the ahead-of-time kernel
// (jit, phase_mask, fetch_runs: the launch's MPCASM_OPT_JIT, _PHASE_MASK and _JIT_FETCH_RUNS)
const void* jit_kernel_for(const PlanDev& d, const int32_t* h_itab, int device, int batch,
                           size_t lds_bytes, int jit, int phase_mask, int fetch_runs);
// the code object of a generated header: from the disk cache ($MPCASM_CACHE_DIR, $XDG_CACHE_HOME/mpcasm
// or ~/.cache/mpcasm; MPCASM_NO_DISK_CACHE=1: never), else compiled and stored there
// (distrust_disk: the cached file was read and did not load -- delete it and compile)
bool jit_code_for(const std::string& header, bool stamps, int phases, std::vector<char>* code,
                  std::string* log, bool distrust_disk = false);
bool jit_available();
// compilations, code objects read from / written to the disk cache, in this process so far
void jit_stats(long out[3]);
// (called when a plan is destroyed: compiled kernels are remembered by the plan's device tables)
void jit_forget(const void* itab);
int jit_launch(const void* kernel, const PlanDev& p, const AssembleCall& call);

}  // namespace mpcasm
