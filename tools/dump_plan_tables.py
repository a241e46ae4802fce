"""Write the tables of a few small valid plans for tools/plan_check_sweep (the sanitizer sweep of the plan
checker): ``python tools/dump_plan_tables.py DIR`` leaves ``DIR/<name>.itab`` (int32) and
``DIR/<name>.dtab`` (float64) per plan.  CPU only: ``tools.extend_matrices`` is served by the oracle, as in the
tests' ``cpu_api`` fixture.  Nothing is kept: the tables come from the plan compiler each time."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (os.path.join(ROOT, "mpc-interface_amd"), ROOT):
    if path not in sys.path:
        sys.path.insert(0, path)


def plans():
    import mpc_interface.tools as tools
    from mpcasm import problems
    from mpcasm.plan import compile_plan
    from oracle import qp_oracle

    tools.extend_matrices = qp_oracle.extend_matrices
    api = problems.load_api("mpc_interface")

    def biped(samples):
        form = problems.biped(api, problems.BipedConfig(step_samples=samples))
        form.update(step_times=np.array([samples - 2, 2 * samples - 2]), step_count=0)
        return form

    yield "body_case", compile_plan(problems.body_case(api))
    yield "biped", compile_plan(biped(8))
    yield "biped_lti", compile_plan(biped(8), lti=["LIP"])
    yield "biped_csc", compile_plan(biped(12), csc="upper")
    yield "lipm3d_compact", compile_plan(problems.lipm3d(api, N=16), lti=["LIP"], workspace="compact")
    yield "lipm_ltv", compile_plan(problems.lipm_ltv(api, N=12), ltv=["LIP"])
    wide = problems.random_lti(api, np.random.default_rng(3), nx=4, nu=4, N=32)
    yield "wide_lti", compile_plan(wide, lti=["plant"])


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for name, plan in plans():
        np.ascontiguousarray(plan.itab, dtype=np.int32).tofile(os.path.join(out_dir, name + ".itab"))
        np.ascontiguousarray(plan.dtab, dtype=np.float64).tofile(os.path.join(out_dir, name + ".dtab"))
        print("%-16s %7d words of itab, %6d of dtab" % (name, plan.itab.size, plan.dtab.size))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "plan_tables")
