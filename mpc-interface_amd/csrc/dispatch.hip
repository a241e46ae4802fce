// dispatch.hip -- which kernel family mpcasm_assemble runs on, stated once (assemble_route), and the launch that
// follows it (launch_assemble).  Host code only.  Everything that predicts a launch -- mpcasm_plan_prepare,
// mpcasm_tiled_route, mpcasm_assemble_route -- asks assemble_route too.
#include "jit.h"
#include "kernels.h"

namespace mpcasm {

int assemble_route(const PlanDev& plan, int batch, const LaunchOptions& opt, bool inputs_aligned, bool indexed,
                   AssembleRoute* out) {
  *out = AssembleRoute{MPCASM_KERNEL_NONE, 0, 0};
  // a dynamics compiled as ltv: the sweep kernel and nothing else (the other kernels' tables describe
  // the formulation's own horizon matrices, the source slots carry (A_k, B_k))
  if (sweep_eligible(plan)) {
    if (indexed) return MPCASM_ERR_LIMIT;   // (rows of `given` by index: the persistent kernel only)
    out->kernel = MPCASM_KERNEL_SWEEP;
    return MPCASM_OK;
  }
  PlanDev p = plan;
  p.rs_p_direct = p.rs_ok ? resident_p_direct_for(plan, batch) : 0;  // (the launch's size decides)
  out->p_direct = p.rs_p_direct;
  // elsewhere, horizon matrices generated from (A, B) and the CSC form of the results exist in the
  // persistent kernel only
  const bool persistent_only = p.rs_nlti != 0 || p.csc_pnnz != 0 || p.csc_gnnz != 0;
  // the persistent kernel may take a whole CU's LDS (one workgroup of 8 wavefronts per
  // CU still beats the staged pipeline by far); the per-instance fused kernel is only
  // worth it while two workgroups fit
  constexpr size_t FUSED_LDS_LIMIT = 80 * 1024;
  const size_t rs = resident_lds_bytes(p);
  if (rs != 0 && rs <= RESIDENT_LDS_LIMIT && (opt.path == 0 || persistent_only) && inputs_aligned) {
    out->kernel = MPCASM_KERNEL_RESIDENT;
    out->lds = rs;
    return MPCASM_OK;
  }
  if (indexed) return MPCASM_ERR_LIMIT;   // (rows of `given` by index: the persistent kernel only)
  // wide problems: one workgroup per block of P, rows composed straight into the LDS tiles
  if (tiled_eligible(p) && opt.path != 2 && p.csc_pnnz == 0 && p.csc_gnnz == 0) {
    out->kernel = MPCASM_KERNEL_TILED;
    return MPCASM_OK;
  }
  if (persistent_only) return MPCASM_ERR_LIMIT;
  const size_t lds = fused_lds_bytes(p, 4);
  if (lds != 0 && lds <= FUSED_LDS_LIMIT && opt.path <= 1) {
    out->kernel = MPCASM_KERNEL_FUSED;
    out->lds = lds;
    return MPCASM_OK;
  }
  out->kernel = MPCASM_KERNEL_STAGED;
  return MPCASM_OK;
}

int launch_assemble(const PlanDev& plan, const AssembleCall& c) {
  AssembleRoute r;
  const int rc = assemble_route(plan, c.batch, c.opt, resident_inputs_aligned(plan, c.src, c.params, c.given),
                                c.indexed, &r);
  if (rc != MPCASM_OK) return rc;
  PlanDev p = plan;
  p.rs_p_direct = r.p_direct;
  *c.kernel = r.kernel;   // (the tiled path names its scan and shared-model forms itself)
  switch (r.kernel) {
    case MPCASM_KERNEL_SWEEP:
      return launch_assemble_sweep(plan, c);   // (the plan as it was created: no hand-over of P to choose)
    case MPCASM_KERNEL_RESIDENT:
      // large batches: the same kernel compiled for this very plan (jit.hip), when available
      if (const void* k = jit_kernel_for(p, c.h_itab, c.device, c.batch, r.lds, c.opt.jit, c.opt.phase_mask,
                                         c.opt.fetch_runs)) {
        *c.kernel = MPCASM_KERNEL_RESIDENT_JIT;
        return jit_launch(k, p, c);
      }
      return launch_assemble_resident(p, c, r.lds);
    case MPCASM_KERNEL_TILED:
      return launch_assemble_tiled(p, c);
    case MPCASM_KERNEL_FUSED:
      return launch_assemble_fused(p, c, r.lds);
    default:
      return launch_assemble_staged(p, c);
  }
}

}  // namespace mpcasm
