"""RANSAC plane segmentation (ltm_scanset_segment_planes) on the outputs of a BASELINE configs[1] run (synthetic lot, os1-64, 2 x --n-kf keyframes, 3-res
removert): the central session's static-projected scans with axis (0, 0, 1), eps 10 deg, threshold 0.1 m, 128 hypotheses.
 (a) all scans in one batch, against one call per scan (the same entry point over the range [k, k + 1)) and against the numpy restatement
     (tools/plane_numpy.py), with the counters of the batch;
 (b) the figure that motivates the entry point: clusters and the size of the largest cluster per scan from Context.cluster at tolerance 0.5 m, min_size 10,
     once on the scans as they are and once on split(...)'s rest after search_index_batch.
Times are host clocks around calls that end in a device synchronise: the median of --steps samples after --warmup, with every sample and the spread (min,
max) in the record; the callables alternate inside every step; index builds and uploads are outside the timed region.  The restatement runs once, on all
scans unless --baseline-scans says fewer.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_planes.py [--n-kf 500] [--steps 9] [--warmup 2] [--baseline-scans 0] [--out profiles/planes_lot-2x500.json]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

THR, ITERATIONS, AXIS, EPS = 0.1, 128, (0.0, 0.0, 1.0), math.radians(10.0)
TOL, MIN_SIZE = 0.5, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-kf", type=int, default=500)
    ap.add_argument("--sensor", default="os1-64")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-scans", type=int, default=0, help="0: the restatement runs on every scan; N: on N evenly spaced scans")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_planes needs a GPU (there is no CPU fallback)")
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    from ltmapper_amd.removerter import HipOps, Params, Removerter, Session
    from tools import plane_numpy as pref
    from tools import synth

    dev = "cuda:0"
    sess = [synth.make_session(s, args.n_kf, args.sensor, device=dev) for s in (1, 2)]
    torch.cuda.synchronize()
    ctx = capi.Context(vfov=50.0, hfov=360.0, device=0)

    def load(S):
        scans = ctx.scans_from_device(S["scans"].data_ptr(), S["offsets"].numpy().astype(np.uint64))
        return ctx.preclean(scans, 2.5), ctx.poses(S["poses"], S["inv"])

    (cs, cp), (qs, qp) = load(sess[0]), load(sess[1])
    P = Params(gpu_use_self_removert=True, remove_resolution_list=[2.5, 2.0, 1.5], num_nn_points_within=2, dist_nn_points_within=0.01, downsample_voxel_size=0.05)
    rm = Removerter(HipOps(ctx), P, Session("Central", cs, cp), Session("Query", qs, qp))
    rm.run()
    ctx.synchronize()
    scans_pts, scans_off = rm.central_sess_.keyframe_scans_static_projected_.download()
    n_kf = len(scans_off) - 1

    def timed(fns):
        for _ in range(args.warmup):
            for f in fns:
                f()
        ts = [[] for _ in fns]
        for _ in range(args.steps):
            for k, f in enumerate(fns):
                t0 = time.perf_counter()
                f()
                ts[k].append(1e3 * (time.perf_counter() - t0))
        return [{"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3), "samples": [round(x, 3) for x in t]} for t in ts]

    ss = ctx.upload_scans(scans_pts, scans_off)

    def batch():
        ctx.segment_planes(ss, THR, ITERATIONS, AXIS, EPS).close()
        ctx.synchronize()

    def each():
        for k in range(n_kf):
            ctx.segment_planes(ss, THR, ITERATIONS, AXIS, EPS, kf_begin=k, kf_end=k + 1).close()
        ctx.synchronize()

    t_batch, t_each = timed([batch, each])
    ctx.plane_stats(reset=True)
    planes = ctx.segment_planes(ss, THR, ITERATIONS, AXIS, EPS)
    ctx.synchronize()
    counters = ctx.plane_stats(reset=True)
    out = {"tool": "bench_planes", "workload": f"lot-2x{args.n_kf}-{args.sensor}-3res", "distance_threshold": THR, "max_iterations": ITERATIONS, "axis": list(AXIS),
           "eps_angle_deg": 10.0, "steps": args.steps, "warmup": args.warmup, "scans": n_kf, "points": int(scans_off[-1]),
           "batch_ms": t_batch["median"], "one_call_per_scan_ms": t_each["median"], "batch_timing": t_batch, "one_call_per_scan_timing": t_each,
           "counters": counters, "found": int(planes.found.sum()), "refined": int(planes.refined.sum()),
           "ground_points": int(planes.n_inliers.sum()), "valid_hypotheses_per_scan": round(float(planes.n_valid.mean()), 2) if n_kf else 0.0}
    out["point_hypothesis_tests_per_ms"] = round(counters["point_hypothesis_tests"] / max(t_batch["median"], 1e-9), 1)

    # the restatement, once
    sub = sorted(set(np.linspace(0, n_kf - 1, min(args.baseline_scans or n_kf, n_kf)).astype(int).tolist())) if n_kf else []
    p = pref.params(THR, ITERATIONS, AXIS, EPS)
    counts_dev, best_dev = planes.hypothesis_counts(), planes.best
    t0 = time.perf_counter()
    agree = True
    for k in sub:
        r = pref.segment(scans_pts[int(scans_off[k]):int(scans_off[k + 1])], p)
        agree = agree and (r["counts"] == counts_dev[k]).all() and r["best"] == best_dev[k]
    dt = time.perf_counter() - t0
    print(f"bench_planes: the restatement took {dt:.1f} s on {len(sub)} scans", file=sys.stderr, flush=True)
    out["restatement"] = {"scans": len(sub), "ms": round(1e3 * dt, 1), "agrees": bool(agree)}
    out["batch_beats_one_call_per_scan"] = t_batch["median"] < t_each["median"]

    # ---- (b) clusters with and without the ground
    def cluster_figures(scanset):
        indices = ctx.search_index_batch(scanset)
        sets = ctx.cluster(indices, TOL, MIN_SIZE)
        n_clusters = [s.info()[1] for s in sets]
        largest = [int(s.sizes[0]) if s.info()[1] else 0 for s in sets]
        for s in sets:
            s.close()
        for i in indices:
            i.close()
        pts = np.diff(scanset.offsets().astype(np.int64))
        share = [l / n for l, n in zip(largest, pts.tolist()) if n]
        return {"clusters_per_scan_mean": round(float(np.mean(n_clusters)), 2), "clusters_per_scan_median": float(np.median(n_clusters)),
                "largest_cluster_mean": round(float(np.mean(largest)), 1), "largest_cluster_median": float(np.median(largest)),
                "largest_cluster_share_of_scan_mean": round(float(np.mean(share)), 4) if share else 0.0, "points": int(pts.sum()),
                "clusters_per_scan": n_clusters, "largest_cluster": largest}

    ground, rest = planes.split(ss)
    out["clusters"] = {"tolerance": TOL, "min_size": MIN_SIZE, "scans_as_they_are": cluster_figures(ss), "rest_after_split": cluster_figures(rest)}
    ground.free()
    rest.free()
    planes.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
