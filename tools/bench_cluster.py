"""Euclidean cluster extraction (ltm_search_cluster) on the outputs of a BASELINE configs[1] run (synthetic lot, os1-64, 2 x --n-kf keyframes, 3-res removert):
the ND and PD maps in one call, and the central session's static-projected scans as one batch and as one call per scan, at tolerance 0.5 m, min_size 10.
Beside each, in the same run, what a caller could do before this entry point existed -- ltm_radius_search of the cloud against itself, the CSR
downloaded, scipy's connected_components on the host -- and the scipy restatement alone (tools/cluster_numpy.py: cKDTree pairs + connected_components).
The fused path is timed with the clique leaves on and off (context switch LTM_CLUSTER_CLIQUE), the two alternating, with the counters of each.
Times are host clocks around calls that end in a device synchronise: the median of --steps samples after --warmup, with every sample and the
spread (min, max) in the record; a sample of the two small maps is --map-reps calls back to back, so that it lasts tens of milliseconds.  The host
baselines run once, on all scans unless --baseline-scans says fewer.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_cluster.py [--n-kf 500] [--steps 9] [--warmup 2] [--map-reps 20] [--baseline-scans 0] [--out profiles/cluster_lot-2x500.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOL, MIN_SIZE = 0.5, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-kf", type=int, default=500)
    ap.add_argument("--sensor", default="os1-64")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--map-reps", type=int, default=20, help="calls per timed sample of the two maps")
    ap.add_argument("--baseline-scans", type=int, default=0, help="0: the host baselines run on every scan; N: on N evenly spaced scans (the fused path is timed on the same set)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_cluster needs a GPU (there is no CPU fallback)")
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    from ltmapper_amd.removerter import HipOps, Params, Removerter, Session
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from tools import cluster_numpy as cref
    from tools import synth

    dev = "cuda:0"
    sess = [synth.make_session(s, args.n_kf, args.sensor, device=dev) for s in (1, 2)]
    torch.cuda.synchronize()
    ctx = capi.Context(vfov=50.0, hfov=360.0, device=0)
    os.environ["LTM_CLUSTER_CLIQUE"] = "0"
    ctx_off = capi.Context(vfov=50.0, hfov=360.0, device=0)      # the same kernels without clique leaves
    del os.environ["LTM_CLUSTER_CLIQUE"]

    def load(S):
        scans = ctx.scans_from_device(S["scans"].data_ptr(), S["offsets"].numpy().astype(np.uint64))
        return ctx.preclean(scans, 2.5), ctx.poses(S["poses"], S["inv"])

    (cs, cp), (qs, qp) = load(sess[0]), load(sess[1])
    P = Params(gpu_use_self_removert=True, remove_resolution_list=[2.5, 2.0, 1.5], num_nn_points_within=2, dist_nn_points_within=0.01, downsample_voxel_size=0.05)
    rm = Removerter(HipOps(ctx), P, Session("Central", cs, cp), Session("Query", qs, qp))
    rm.run()
    ctx.synchronize()
    maps = {k: rm.outputs[k].download() for k in ("nd_map", "pd_map")}
    scans_pts, scans_off = rm.central_sess_.keyframe_scans_static_projected_.download()

    def timed(fns, reps=1):
        """per callable: dict of the median, the spread and every sample [ms per call]; a sample is `reps` calls, the callables alternate inside every step"""
        for _ in range(args.warmup):
            for f in fns:
                f()
        ts = [[] for _ in fns]
        for _ in range(args.steps):
            for k, f in enumerate(fns):
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                ts[k].append(1e3 * (time.perf_counter() - t0) / reps)
        return [{"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3), "samples": [round(x, 3) for x in t],
                 "calls_per_sample": reps} for t in ts]

    def fused(c, indices, each=False):
        def run():
            if each:
                for i in indices:
                    i.cluster(TOL, MIN_SIZE).close()
            else:
                for s in c.cluster(indices, TOL, MIN_SIZE):
                    s.close()
            c.synchronize()
        return run

    def counters(c, run):
        c.cluster_stats(reset=True)
        run()
        return c.cluster_stats(reset=True)

    def radius_baseline(indices, clouds):
        """ltm_radius_search of every cloud against its own index, the CSR on the host, scipy components, the size filter"""
        def run():
            out = []
            for index, pts in zip(indices, clouds):
                n = len(pts)
                if not n:
                    out.append(0)
                    continue
                off, idx, _ = index.radius(pts, TOL)
                rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off.astype(np.int64)))
                _, lab = connected_components(coo_matrix((np.ones(len(idx), np.int8), (rows, idx)), shape=(n, n)), directed=False)
                out.append(int((np.bincount(lab) >= MIN_SIZE).sum()))
            return out
        return run

    def scipy_baseline(clouds):
        return lambda: [len(cref.cluster(p, TOL, MIN_SIZE)["sizes"]) for p in clouds]

    def host_time(f):
        t0 = time.perf_counter()
        r = f()
        dt = time.perf_counter() - t0
        print(f"bench_cluster: a host baseline took {dt:.1f} s", file=sys.stderr, flush=True)
        return dt, r

    out = {"tool": "bench_cluster", "workload": f"lot-2x{args.n_kf}-{args.sensor}-3res", "tolerance": TOL, "min_size": MIN_SIZE, "steps": args.steps, "warmup": args.warmup}

    # ---- the two maps in one call
    clouds = [maps["nd_map"], maps["pd_map"]]
    idx_on = [ctx.search_index(p) for p in clouds]
    idx_off = [ctx_off.search_index(p) for p in clouds]
    t_on, t_off = timed([fused(ctx, idx_on), fused(ctx_off, idx_off)], reps=args.map_reps)
    sets = ctx.cluster(idx_on, TOL, MIN_SIZE)
    m = {"points": [len(p) for p in clouds], "clusters": [s.info()[1] for s in sets], "clustered_points": [s.info()[2] for s in sets],
         "fused_ms": t_on["median"], "fused_no_clique_ms": t_off["median"], "fused_timing": t_on, "fused_no_clique_timing": t_off,
         "counters": counters(ctx, fused(ctx, idx_on)), "counters_no_clique": counters(ctx_off, fused(ctx_off, idx_off))}
    n_pts = max(sum(m["points"]), 1)
    m["pair_tests_per_point"] = round(m["counters"]["pairs_tested"] / n_pts, 2)
    m["pair_tests_per_point_no_clique"] = round(m["counters_no_clique"]["pairs_tested"] / n_pts, 2)
    try:
        t, got = host_time(radius_baseline(idx_on, clouds))
        m["radius_search_plus_scipy_ms"] = round(1e3 * t, 1)
        m["radius_baseline_agrees"] = got == m["clusters"]
    except capi.LtmError as e:
        m["radius_search_plus_scipy_ms"] = None
        m["radius_baseline_error"] = str(e)
    t, got = host_time(scipy_baseline(clouds))
    m["scipy_restatement_ms"] = round(1e3 * t, 1)
    m["restatement_agrees"] = got == m["clusters"] and all((s.sizes == cref.cluster(p, TOL, MIN_SIZE)["sizes"]).all() for s, p in zip(sets, clouds))
    for s in sets:
        s.close()
    out["maps"] = m

    # ---- the static-projected scans of the central session
    ss = ctx.upload_scans(scans_pts, scans_off)
    indices = ctx.search_index_batch(ss)
    ss_off = ctx_off.upload_scans(scans_pts, scans_off)
    indices_off = ctx_off.search_index_batch(ss_off)
    n_kf = len(indices)
    t_batch, t_batch_off, t_each = timed([fused(ctx, indices), fused(ctx_off, indices_off), fused(ctx, indices, each=True)])
    sub = sorted(set(np.linspace(0, n_kf - 1, min(args.baseline_scans or n_kf, n_kf)).astype(int).tolist()))
    sub_idx = [indices[k] for k in sub]
    sub_clouds = [scans_pts[int(scans_off[k]):int(scans_off[k + 1])] for k in sub]
    (t_sub,) = timed([fused(ctx, sub_idx)])
    sets = ctx.cluster(sub_idx, TOL, MIN_SIZE)
    sub_clusters = [s.info()[1] for s in sets]
    for s in sets:
        s.close()
    s_ = {"scans": n_kf, "points": int(scans_off[-1]), "fused_batch_ms": t_batch["median"], "fused_batch_no_clique_ms": t_batch_off["median"],
          "fused_one_call_per_scan_ms": t_each["median"], "fused_batch_timing": t_batch, "fused_batch_no_clique_timing": t_batch_off,
          "fused_one_call_per_scan_timing": t_each, "counters": counters(ctx, fused(ctx, indices)),
          "counters_no_clique": counters(ctx_off, fused(ctx_off, indices_off)),
          "baseline_set": {"scans": len(sub), "points": int(sum(len(p) for p in sub_clouds)), "fused_batch_ms": t_sub["median"], "fused_batch_timing": t_sub}}
    s_["pair_tests_per_point"] = round(s_["counters"]["pairs_tested"] / max(s_["points"], 1), 2)
    s_["pair_tests_per_point_no_clique"] = round(s_["counters_no_clique"]["pairs_tested"] / max(s_["points"], 1), 2)
    t, got = host_time(radius_baseline(sub_idx, sub_clouds))
    s_["baseline_set"]["radius_search_plus_scipy_ms"] = round(1e3 * t, 1)
    s_["baseline_set"]["radius_baseline_agrees"] = got == sub_clusters
    t, got = host_time(scipy_baseline(sub_clouds))
    s_["baseline_set"]["scipy_restatement_ms"] = round(1e3 * t, 1)
    s_["baseline_set"]["restatement_agrees"] = got == sub_clusters
    out["scans"] = s_
    for c in (m, s_):
        for key in ("counters", "counters_no_clique"):
            k = c[key]
            k["clique_exit_share_of_edges"] = round(k["clique_early_exits"] / max(k["edges_found"], 1), 4)
    out["fused_beats_radius_baseline"] = {
        "maps": None if m["radius_search_plus_scipy_ms"] is None else m["fused_ms"] < m["radius_search_plus_scipy_ms"],
        "scans": s_["baseline_set"]["fused_batch_ms"] < s_["baseline_set"]["radius_search_plus_scipy_ms"]}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)
    ctx_off.close()
    ctx.close()


if __name__ == "__main__":
    main()
