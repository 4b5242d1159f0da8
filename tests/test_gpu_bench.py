"""bench.py as it is run for every change: a plain run times exactly --steps steps and prints the contract fields; two runs with the same
arguments and --dump-outputs write the same arrays; --full still carries the figures that need runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
WORKLOAD = "lot-2x100-small-3res"


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", WORKLOAD] + list(args), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    lines = [_bench("--steps", str(k), "--warmup", "1", "--dump-outputs", str(tmp_path / tag)) for k, tag in ((2, "a"), (3, "b"))]
    for k, d in zip((2, 3), lines):
        assert d["steps"] == k and d["metric"] == "keyframe-pairs/sec (removert+diff)" and d["unit"] == "keyframe-pairs/s"
        assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["ms_per_step"] > 0
        assert abs(d["value"] * d["ms_per_step"] / 1e3 - d["config"]["keyframe_pairs_per_step"]) <= 0.01 * d["config"]["keyframe_pairs_per_step"]
        assert "roofline" not in d and "cpu_baseline" not in d, "a plain run measures the headline figure only"
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"map_updated_map.npy", "map_OriginalNoisyCentralMapGlobal.size.npy", "scans_scans_updated.npy", "scans_scans_updated.offsets.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype and a.shape == b.shape, n
        assert a.tobytes() == b.tobytes(), f"{n} differs between two runs with the same inputs"
        total += a.nbytes
    assert total <= 64 << 20
    sizes = [np.load(tmp_path / "a" / f"map_OriginalNoisy{s}MapGlobal.size.npy").tolist() for s in ("Central", "Query")]
    assert sizes == [[n] for n in lines[0]["config"]["map_points_last_pair"]]


def test_full_run_still_carries_the_kernel_classes():
    d = _bench("--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--extra-out", os.devnull)
    assert d["steps"] == 1 and d["ms_per_step"] > 0
    assert d["roofline"] and d["roofline"]["class"] and d["classes"], "per-kernel figures of the --full run"
    assert d["lanes"] == 2 and d["one_lane_ms_per_step"] > 0
