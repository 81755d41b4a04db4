"""The plain bench line (`python bench.py --steps K --warmup W`, no --full): exactly K timed steps, the headline fields and nothing that needs a
run of its own; --dump-outputs writes the map the timed steps built, and two runs with the same arguments write the same map."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(out_dir):
    # 30 steps over a loop of 20 poses: two timed segments (20 + 10), the map emptied before each
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "3", "--unique-frames", "20",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_times_exactly_k_steps_and_dumps_the_map(tmp_path):
    a = _plain(tmp_path / "a")
    assert a["steps"] == 30 and a["warmup"] == 3 and a["repeats"] == 2, a
    assert a["ms_per_step"] > 0 and a["higher_is_better"] is True and a["unit"] == "frames/s" and a["dtype"] == "f32"
    assert abs(a["value"] - 1e3 / a["ms_per_step"]) <= 0.01 * a["value"], a
    for k in ("parity", "cpu_baseline", "roofline", "kernels", "ms_per_step_revisit", "frame_latency"):
        assert k not in a, k                               # (--full only)
    files = sorted(glob.glob(str(tmp_path / "a" / "*.npy")))
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    assert {"tsdf_block_indices", "tsdf_distance", "tsdf_weight", "color_r", "esdf_squared_distance_vox", "esdf_slice"} <= set(arrays), sorted(arrays)
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
    assert sum(os.path.getsize(f) for f in files) <= 64 * 10 ** 6
    n = len(arrays["tsdf_block_indices"])
    assert n > 100 and arrays["tsdf_distance"].shape == (n, 512) and float(arrays["tsdf_weight"].max()) > 0
    assert arrays["tsdf_blocks_total"][0] == n                            # (the room's map is far below the size budget: no sampling)
    b = _plain(tmp_path / "b")
    for name, va in arrays.items():
        vb = np.load(str(tmp_path / "b" / (name + ".npy")))
        assert va.shape == vb.shape and float(np.abs(va.astype(np.float64) - vb).max(initial=0.0)) <= 1e-4, name
    assert b["steps"] == 30 and b["repeats"] == 2
