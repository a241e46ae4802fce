"""GPU: mpcasm_qp_sens_wide (csrc/sens_core.h in csrc/polish_wide.hip) held to tests/sens_restatement.py as
tests/test_gpu_qp_sens.py holds mpcasm_qp_sens, by the same judge (tests/sens_cases.py): on the shapes at which each
loop of the wide back-end can go wrong (tests/polish_wide_cases.py), on three instances of its largest, on more
instances than the launch has workgroups, and beside mpcasm_qp_sens where both apply -- each entry held to the
yardstick, not to the other's bits."""
import numpy as np
import pytest

import polish_wide_cases as cases
import sens_cases as sc
import sens_restatement as sn
from mpcasm import capi

pytestmark = pytest.mark.gpu
SHAPES = cases.SHAPES + [s for s in cases.BOTH if s not in cases.SHAPES]


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.mark.parametrize("no,nc,na", SHAPES, ids=cases.IDS(SHAPES))
def test_verdicts_accuracy_and_untouched_outputs(gpu_api, torch_gpu, no, nc, na):
    """The seven instances of tests/test_gpu_qp_sens.py, with their status and with status = NULL, with the dense
    gradients and without; on the shapes mpcasm_qp_sens takes too, that entry on the same instances."""
    from mpcasm import engine

    assert engine.qp_sens_wide_info(no, nc, 7) == engine.qp_polish_wide_info(no, nc, 7)
    sc.seven(torch_gpu, engine.qp_sensitivity_wide, no, nc, na, "wide")
    if (no, nc, na) in cases.BOTH:
        sc.seven(torch_gpu, engine.qp_sensitivity, no, nc, na, "lds")


def test_the_largest_shape(gpu_api, torch_gpu):
    """Three plain instances of (512, 520, 100)."""
    from mpcasm import engine

    no, nc, na = cases.LARGEST
    case = sc.problem(no, nc, na, count=3)
    outs, worst = sc.run(torch_gpu, engine.qp_sensitivity_wide, case, tuple(case[k] for k in "xyz"), None,
                         "wide %dx%d na %d" % cases.LARGEST)
    assert all(o.verdict == sn.DONE and np.array_equal(o.active, a) for o, a in zip(outs, case["active"]))
    sc.record("wide %dx%d-na%d" % cases.LARGEST, "residual %.3f  lres %.3f  gP %.3f  gG %.3f" % tuple(worst))


def test_more_instances_than_workgroups(gpu_api, torch_gpu, monkeypatch):
    """Two workgroups striding seven instances: each reuses its LDS and its slice of the workspace, a skipped and a
    singular instance among them."""
    from mpcasm import engine

    monkeypatch.setenv("MPCASM_QP_POLISH_WIDE_GROUPS", "2")
    assert engine.qp_sens_wide_info(36, 76, 7)[2] == 2
    sc.seven(torch_gpu, engine.qp_sensitivity_wide, 36, 76, 20, "wide, 2 groups")


def test_a_workspace_that_is_too_small_is_refused(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm import engine

    no, nc, na = 36, 76, 20
    case = sc.problem(no, nc, na, count=3)
    dev = lambda a: torch.as_tensor(np.array(a), device="cuda")
    args = (dev(case["P"]), dev(case["G"]), dev(case["h"]), tuple(dev(case[k]) for k in "xyz"), dev(case["rx"]),
            dev(case["ry"]))
    need = engine.qp_sens_wide_info(no, nc, 3)[1]
    out = engine.qp_sensitivity(*args)
    verdict = torch.full((3,), -99, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.MpcasmError) as err:
        engine.qp_sensitivity_wide(*args, work=torch.empty((need - 8,), dtype=torch.uint8, device="cuda"),
                                   out=(None, None, None, None, verdict, None))
    assert err.value.status == capi.ERR_ARG and verdict.tolist() == [-99] * 3      # (nothing was launched)
    got = engine.qp_sensitivity_wide(*args, work=torch.empty((need,), dtype=torch.uint8, device="cuda"))
    assert got.verdict.tolist() == [capi.SENS_DONE] * 3 == out.verdict.tolist()
