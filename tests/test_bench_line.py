"""The printed bench line must be parseable from the tail of stdout the driver keeps (round 4's 21 KB line was not, BENCH_r04.parsed = null)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _synthetic_full():
    """a `full` record as bench.py builds it, with every list at its real length and prose in every string field"""
    prose = "x" * 400
    classes = ["vote_map_cull", "reproject_map", "voxel", "merge", "knn_query", "knn_query_p2", "partition", "vote_scan", "vote_compare", "vote_fill", "vote_map_exact",
               "knn_build", "reproject_gather", "voxel_scanset", "voxel_grid_scanset"]
    rl = [{"class": c, "kernels": prose, "bound": "hbm", "ms_per_step": 12.345, "launches_per_step": 21.0, "units_per_step": 1.0e9, "algorithmic_bytes_per_step": 6.2e11,
           "compulsory_bytes_per_step": 1.0e11, "hbm_algorithmic_frac": 1.0071, "hbm_compulsory_frac": 0.1712, "valu_frac": 0.6123, "traffic": 1.03e11, "traffic_scope": prose,
           "hbm_measured_frac": 0.1673, "traffic_over_compulsory": 1.023, "frac": 0.6123, "class_kernels_counted": [prose] * 4} for c in classes]
    return {
        "metric": "keyframe-pairs/sec (removert+diff)", "value": 2921.123, "unit": "keyframe-pairs/s", "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 171.123,
        "cxx_host_ms_per_step": 170.63, "cxx_host_one_shot_steps123_ms": 200.1, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "dtype_detail": prose,
        "data": "synthetic (tools/synth.py synth-v1, seed 20250224)",
        "config": {"workload": "lot-2x500-os1-64-3res", "sessions": prose, "keyframes_per_session": 500, "keyframe_pairs_per_step": 500, "sensor": "os1-64",
                   "remove_resolution_list": [2.5, 2.0, 1.5], "self_removert": True, "knn": {"k": 2, "thr": 0.01}, "voxel": 0.05, "map_points_last_pair": [6831259, 6789012],
                   "scan_points": [27000000, 27000000], "parallelism": prose, "step": prose},
        "roofline": dict(rl[0], kernel="k_vote_map_cull", achieved=48.1, peak=78.6, unit="T VALU lane-inst/s", avg_launch_ms=3.672, share_of_step=0.45, pmc=True, pmc_source=prose,
                         definitions=prose, algorithmic_bytes_per_launch=2.9e10, compulsory_bytes_per_launch=5.0e9),
        "cpu_baseline": {"value": 0.3314, "unit": "keyframe-pairs/s", "cores": 1, "kind": "port", "reference_compiled": {"what": prose, "port_speedup_over_reference_compiled": 1.41},
                         "sample": prose * 2, "sample_short": prose, "measured_s": 52.1, "keyframe_stride": 50, "extrapolated_step_s": 1509.0, "host_cores": 256, "cgroup_cpu_quota_cpus": 16.0,
                         "all_cores": {"value": 2.7171, "cores": 256, "quota_note": prose * 2, "cgroup_cpu_quota_cpus": 16.0, "measured_s": 187.0,
                                       "quoted_from": "profiles/cpu_allcore_latest.json (same oracle sources, " + prose + ")"},
                         "full_unsampled_runs_committed": {"1thread": {"cpu": prose}, "allcore": {"cpu": prose}}},
        "rooflines": rl, "traffic_groups": [{"group": prose, "classes": classes}] * 5,
        "t_total": {"what": prose, "configs[1] 2x500 3-res": {"T_total_s": 0.416, "T_step0_s": 0.189, "T_steps123_s": 0.2, "x": prose}, "cxx_host_bench": {"classes": {c: 1.0 for c in classes}}},
        "parity_fullsize": {"record": prose, "matches_sources": True}, "scaling_model": {"what": prose * 5}, "stage_ms": {c: 1.0 for c in classes},
        "kernel_classes_ms_per_step": {c: 1.0 for c in classes}, "voxel_grids": {"what": prose}, "vote_cull": {"fraction": 0.1}, "synth_generation_s": 9.9,
    }


def test_printed_line_is_short_and_parses_from_an_8000_byte_tail():
    import bench
    full = _synthetic_full()
    assert len(json.dumps(full)) > 20000          # the record itself is as large as round 4's line
    line = json.dumps(bench.slim_line(full, "profiles/bench_extra_latest.json"))
    assert len(line) < 6000, len(line)
    # what a driver that keeps the last 8000 bytes of stdout sees: warnings before, the line last
    stdout = ("some runtime warning\n" * 2000 + line + "\n").encode()
    tail = stdout[-8000:].decode()
    got = json.loads(tail.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
              "cpu_baseline", "extra"):
        assert k in got, k
    assert got["config"]["workload"] == "lot-2x500-os1-64-3res"
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in got["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in got["cpu_baseline"], k
    assert all(isinstance(v, (int, float, str, bool, type(None))) for v in got["roofline"].values())      # numbers and names, no prose objects
    # a number that was not measured in this run says so in the printed line itself, with the file it comes from
    assert got["cpu_baseline"]["all_cores"]["quoted_from"] == "profiles/cpu_allcore_latest.json" and got["cpu_baseline"]["all_cores"]["measured_now"] is False


def test_the_committed_round4_record_also_slims_down():
    """round 4's actual 21 KB record through the same function"""
    import bench
    path = os.path.join(ROOT, "profiles", "r4_final_bench_default.json")
    full = json.loads(open(path).read().strip().splitlines()[-1])
    assert len(json.dumps(full)) > 15000
    line = json.dumps(bench.slim_line(full, None))
    assert len(line) < 6000 and json.loads(line)["value"] == full["value"]


def test_plain_run_is_the_default_and_full_is_an_option():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_plain_line_carries_the_contract_fields():
    import bench
    full = _synthetic_full()
    head = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                                 "dtype_detail", "data", "config")}
    got = json.loads(json.dumps(bench.head_line(head)))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert got[k] == full[k], k
    assert got["config"]["workload"] == "lot-2x500-os1-64-3res" and len(got["config"]["parallelism"]) <= 120


class _FakeCtx:
    def select(self, cloud, idx):
        assert (idx >= 0).all() and (idx < len(cloud)).all() and (idx[1:] > idx[:-1]).all()
        return _FakeCloud(cloud.pts[idx])


class _FakeCloud:
    """stands in for capi.Cloud: rows of float32 (x, y, z, intensity)"""
    ctx = _FakeCtx()

    def __init__(self, pts):
        self.pts, self.freed = pts, False

    def __len__(self):
        return len(self.pts)

    def download(self):
        return self.pts.copy()

    def free(self):
        self.freed = True


class _FakeScans:
    def __init__(self, pts, offsets):
        self.pts, self.off = pts, offsets

    def offsets(self):
        return self.off

    def as_cloud(self):
        return _FakeCloud(self.pts)


class _FakeRun:
    def __init__(self, outputs, scans):
        self.outputs, self._scans = outputs, scans

    def scan_outputs(self):
        return self._scans


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path):
    import numpy as np
    import bench
    rng = np.random.default_rng(1)
    big = rng.standard_normal((bench.DUMP_ROWS * 3 + 5, 4)).astype(np.float32)
    small = rng.standard_normal((100, 4)).astype(np.float32)
    off = np.array([0, 10, 10, bench.DUMP_ROWS + 7], dtype=np.uint64)
    scans = rng.standard_normal((int(off[-1]), 4)).astype(np.float32)
    run = _FakeRun({"updated_map": _FakeCloud(big), "nd_map": _FakeCloud(small), "strong_nd_map": None}, {"scans_updated": _FakeScans(scans, off)})
    dirs = []
    for tag in ("a", "b"):
        d = tmp_path / tag
        bench.dump_outputs(run, str(d))
        dirs.append(d)
    names = sorted(p.name for p in dirs[0].iterdir())
    assert names == sorted(["map_nd_map.npy", "map_nd_map.size.npy", "map_updated_map.npy", "map_updated_map.size.npy",
                            "scans_scans_updated.npy", "scans_scans_updated.size.npy", "scans_scans_updated.offsets.npy"])
    total = 0
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), n
        total += a.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    assert (np.load(dirs[0] / "map_nd_map.npy") == small).all()
    sample = np.load(dirs[0] / "map_updated_map.npy")
    assert sample.shape == (bench.DUMP_ROWS, 4) and np.load(dirs[0] / "map_updated_map.size.npy").tolist() == [len(big)]
    rows = {r.tobytes() for r in big}
    assert all(r.tobytes() in rows for r in sample[:1000])
    assert np.load(dirs[0] / "scans_scans_updated.offsets.npy").tolist() == off.tolist()
    assert np.load(dirs[0] / "scans_scans_updated.npy").shape == (bench.DUMP_ROWS, 4)
