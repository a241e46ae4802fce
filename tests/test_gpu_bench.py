"""GPU: a plain `bench.py` run -- the headline line and nothing else -- and what --dump-outputs
writes: P, q, G, h of the last timed step, the same in a second run with the same arguments and
the same as the assembly of those instances called directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import RTOL_TIGHT, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 2048


def _bench(out):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    proc = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
         "--batch", str(BATCH), "--dump-outputs", out],
        env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    return json.loads(lines[0])


def _direct(idx):
    """The bench's workload (same seed) through the Assembler, rows ``idx``."""
    import torch

    saved = dict(os.environ)
    sys.path.insert(0, ROOT)
    import bench                               # (sets defaults of its own in the environment)

    os.environ.clear()
    os.environ.update(saved)
    work = bench.build_workload(BATCH, 20260)
    asm = work["engine"].Assembler(work["form"], batch=BATCH, device="cuda", lti=["LIP"])
    asm.bind_lti("LIP", torch.as_tensor(work["A"], device="cuda"), torch.as_tensor(work["B"], device="cuda"))
    asm.set_param("cost", "track vel_x", "aim", work["aims"])
    return [t.cpu().numpy()[idx] for t in asm.assemble(torch.as_tensor(work["given"], device="cuda"))]


def test_plain_run_and_its_outputs(tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    rec = _bench(str(tmp_path / "a"))
    assert rec["steps"] == 7 and rec["warmup"] == 2 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "assemblies/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    for key in ("roofline", "cpu_baseline", "fill", "variants", "c4", "B65536"):
        assert key not in rec, key                      # (--full only)

    names = ("P", "q", "G", "h", "instances")
    out = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    idx = out["instances"].astype(np.int64)
    assert len(idx) == 1024 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < BATCH
    assert out["P"].shape == (1024, 36, 36) and out["q"].shape == (1024, 36)
    assert out["G"].shape == (1024, 76, 36) and out["h"].shape == (1024, 76)
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20

    _bench(str(tmp_path / "b"))                          # the same arguments: the same inputs
    for n in names:
        again = np.load(tmp_path / "b" / (n + ".npy"))
        assert rel_err(again, out[n]) <= RTOL_TIGHT, n
    for n, ref in zip("PqGh", _direct(idx)):
        assert rel_err(out[n], ref) <= RTOL_TIGHT, n
