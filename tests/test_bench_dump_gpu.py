"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, reproducible from run to run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, tag, steps, extra=()):
    out_dir = tmp_path / tag
    env = dict(os.environ, PYTHONPATH=ROOT, EFM_AUTOTUNE="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", "16", "--image", "32", "--no-cpu-baseline", "--no-secondary", "--no-host-loops",
                        "--dump-outputs", str(out_dir), *extra], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    files = sorted(glob.glob(str(out_dir / "*.npy")))
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    return json.loads(lines[0]), {os.path.basename(f)[:-4]: np.load(f) for f in files}


def test_dump_outputs_reproducible_and_follow_steps(tmp_path):
    line_a, a = _bench(tmp_path, "a", 2)
    line_b, b = _bench(tmp_path, "b", 2)
    line_c, c = _bench(tmp_path, "c", 3)
    assert line_a["steps"] == 2 and line_c["steps"] == 3
    assert {"loss", "embedding", "param.conv1_weight", "param.head_weight"} <= set(a)
    assert a["loss"].shape == (8,) and a["embedding"].shape == (16, 128)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert abs(float(a["loss"].mean()) - line_a["loss"]) <= 1e-5 * max(1.0, abs(line_a["loss"]))
    # same arguments -> same inputs -> the same outputs (summation order of the kernels is fixed)
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-6, err_msg=k)
    # one more timed step moves the parameters: --steps is the number of steps that ran
    assert max(float(np.abs(c[k] - a[k]).max()) for k in a if k.startswith("param.")) > 0
