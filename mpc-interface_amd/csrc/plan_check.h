// plan_check.h -- the checker of plan tables (plan_check.cpp): host only, no HIP.  Every kernel trusts every
// index of a plan once validate_plan has returned MPCASM_OK.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mpcasm.h"
#include "plan_dev.h"
#include "plan_tables.h"

namespace mpcasm {

// the zeros toeplitz_assemble_kernel keeps in LDS behind the group's table (doubles; even: what follows stays
// 16-byte aligned): what a stage's window may read past the table's end (the checker holds the stages to it)
inline int toeplitz_zero_pad(int N) { return ((N > 16 ? N : 16) + 16 + 1) & ~1; }

// MPCASM_OK, MPCASM_ERR_PLAN for malformed tables, MPCASM_ERR_LIMIT for more than MAX_SOURCES sources
int validate_plan(const int32_t* itab, const double* dtab, size_t n_itab, size_t n_dtab);

// the int fields of the device-side view, from the (validated) header and tables on the host: everything but
// rs_p_direct, which the persistent kernel's host side chooses (capi.hip host_plan)
void plan_view(const int32_t* itab, PlanDev* out);

}  // namespace mpcasm
