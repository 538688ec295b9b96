"""-m gpu: a plain bench.py run (no --full) on a tiny shape: exactly --steps timed steps, one result line with the headline
fields and nothing of what --full adds, and --dump-outputs writing float32 / float64 arrays within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_with_dumped_outputs(tmp_path):
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--ng-burn-in", "2",
                        "--chunk", "150", "--minibatch", "8", "--den-states", "500", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "f32" and out["metric"]
    assert out["value"] == pytest.approx(8 * 150 * 1e3 / out["ms_per_step"], rel=1e-3)
    assert not {"parity", "cpu_baseline", "alt", "also", "strong"} & set(out)
    names = sorted(p.name for p in out_dir.iterdir())
    assert names == ["params.npy", "params_delta.npy", "results.npy", "stats.npy"], names
    total = 0
    for name in names:
        a = np.load(out_dir / name)
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 << 20
    res = np.load(out_dir / "results.npy")
    assert res[5] == 1.0 and res[0] == pytest.approx(out["config"]["objf_per_frame"] * res[2], rel=1e-6)
    assert np.abs(np.load(out_dir / "params_delta.npy")).max() > 0
