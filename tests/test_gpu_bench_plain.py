"""bench.py without --full: the headline run.  One JSON line whose headline fields say what they always did, the dumped
frame, and none of the side measurements that --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("stage_ms", "roofline", "cpu_baseline", "cpu_reference_tracer", "parity", "parity_metal", "parity_spec",
             "mrays_per_s_1spp", "mrays_per_s_metal", "big_scene", "roofline_hbm_scene", "device_bvh_build_ms")


def test_plain_run_prints_headline_only(tmp_path):
    steps = 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "Mrays/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["metric"].startswith("Mrays/sec, cornell_dragon 1920x1080")
    assert out["steps"] == steps and out["warmup"] == 1
    # value = counted ray segments of the timed steps / their wall time; the bench room is closed: W * H * depth * spp each step
    cfg = out["config"]
    assert cfg["closed_scene"] is True and cfg["rays_per_step"] == 1920 * 1080 * 4 * 16
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - cfg["rays_per_step"] / (out["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * out["value"]
    assert not [k for k in FULL_ONLY if k in out], sorted(out)
    # the frame of the last timed step, as --dump-outputs always wrote it
    assert out["dumped_outputs"] == {"accum": [1080, 1920, 3], "rgba8": [1080, 1920, 3]}
    accum = np.load(tmp_path / "accum.npy")
    rgba8 = np.load(tmp_path / "rgba8.npy")
    assert accum.dtype == np.float32 and accum.shape == (1080, 1920, 3) and np.isfinite(accum).all() and accum.max() > 0
    assert rgba8.dtype == np.float32 and rgba8.shape == (1080, 1920, 3) and rgba8.min() >= 0 and rgba8.max() <= 255
