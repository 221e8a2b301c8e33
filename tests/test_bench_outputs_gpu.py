"""A plain bench.py run: exactly --steps timed steps, the headline line only (no --full blocks), and --dump-outputs writes
what the last timed step returned to its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_steps_outputs(dev, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--pool", "3", "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["unit"] == "pairs/s" and out["dtype"] == "f32"
    B = out["config"]["pairs_per_step"]
    assert abs(out["value"] - B * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    assert not {"roofline", "workloads", "cpu_baseline"} & set(out)
    files = sorted(os.listdir(tmp_path / "out"))
    assert "poses.npy" in files and "n_valid.npy" in files and "n0.npy" in files, files
    d = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and len(a) == B for a in d.values())
    T = d["poses"]
    assert T.shape == (B, 4, 4) and np.isfinite(T).all()
    R = T[:, :3, :3]
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-5) and np.allclose(T[:, 3], [0, 0, 0, 1])
    # the line's last-pair fields come from the same step
    assert int(d["n_valid"][-1]) == out["config"]["ransac_valid_hypotheses_last_pair"]
    assert int((d["n0"][-1] + d["n1"][-1]) / 2) == out["config"]["voxels_per_frame"]
