"""Throughput of the device search index (ltm_search_build / ltm_knn_search / ltm_radius_search) on the central map of BASELINE configs[1]
(synthetic lot, os1-64, 500 keyframes, pre-cleaned at 2.5 m, merged and voxel-gridded at 0.05 m), queried with the query session's scans in
the global frame.  In the same run: ltm_knn_partition at the yaml's k = 2, thr = 0.01 on the same pair, and scipy's cKDTree with 16 workers on
this host as the CPU baseline.  Prints one JSON line.

    python tools/bench_search.py [--n-kf 500] [--steps 5] [--warmup 2]

Radius searches at 2 m return thousands of points per query on a 5 cm map, so they run on an evenly spaced subset of the queries
(--radius-queries); cKDTree runs on subsets as well (--cpu-queries).  Rates are queries per second of the median step."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-kf", type=int, default=500)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radius-queries", type=int, default=100000)
    ap.add_argument("--cpu-queries", type=int, default=1000000)
    ap.add_argument("--no-cpu", action="store_true", help="skip the cKDTree baseline (profiling runs)")
    args = ap.parse_args()

    import torch
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    from tools import synth

    dev = "cuda:0"
    Cs = synth.make_session(1, args.n_kf, "os1-64", device=dev)
    Qs = synth.make_session(2, args.n_kf, "os1-64", device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(vfov=50.0, hfov=360.0, device=0)
    lib = ctx.lib

    def load(S):
        scans = ctx.scans_from_device(S["scans"].data_ptr(), S["offsets"].numpy().astype(np.uint64))
        return ctx.preclean(scans, 2.5), ctx.poses(S["poses"], S["inv"])     # Removerter.cpp:1660

    c_scans, c_poses = load(Cs)
    q_scans, q_poses = load(Qs)
    cmap = ctx.voxel_centroid(ctx.merge_to_global(c_scans, c_poses), 0.05)
    gq = ctx.merge_to_global(q_scans, q_poses)
    n_map, n_q = len(cmap), len(gq)
    host_q = gq.download()
    sub = host_q[np.linspace(0, n_q - 1, min(args.radius_queries, n_q)).astype(np.int64)]
    rq = ctx.upload(sub)
    ctx.synchronize()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ctx.synchronize()
        ts = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    out = {"tool": "bench_search", "workload": f"lot-2x{args.n_kf}-os1-64 central map (0.05 m voxel) <- query session scans, global frame",
           "map_points": n_map, "queries": n_q, "radius_queries": len(sub), "steps": args.steps, "warmup": args.warmup}

    holder = {}

    def build():
        s = C.c_void_p()
        ctx._ck(lib.ltm_search_build(ctx.h, cmap.h, C.byref(s)))
        if "s" in holder:
            lib.ltm_search_free(ctx.h, holder["s"])
        holder["s"] = s
    out["build_ms"] = round(1e3 * timed(build), 3)
    s = holder["s"]

    knn = {}
    for k in (1, 2, 8, 32):
        pi, pd = C.c_void_p(), C.c_void_p()
        ctx._ck(lib.ltm_buffer_alloc(ctx.h, n_q * k * 4, C.byref(pi)))
        ctx._ck(lib.ltm_buffer_alloc(ctx.h, n_q * k * 4, C.byref(pd)))
        dt = timed(lambda: ctx._ck(lib.ltm_knn_search(ctx.h, s, gq.h, k, pi, pd)))
        knn[f"k{k}"] = {"ms": round(1e3 * dt, 3), "queries_per_s": round(n_q / dt)}
        lib.ltm_buffer_free(ctx.h, pd)
        lib.ltm_buffer_free(ctx.h, pi)
    out["knn"] = knn

    rad = {}
    for r in (0.5, 2.0):
        hits = {}

        def radius():
            res = C.c_void_p()
            ctx._ck(lib.ltm_radius_search(ctx.h, s, rq.h, r, 0, C.byref(res)))
            tot = C.c_size_t()
            lib.ltm_search_result_info(ctx.h, res, None, C.byref(tot), None, None, None)
            hits["n"] = tot.value
            lib.ltm_search_result_free(ctx.h, res)
        dt = timed(radius)
        rad[f"r{r}"] = {"ms": round(1e3 * dt, 3), "queries_per_s": round(len(sub) / dt), "mean_hits": round(hits["n"] / max(len(sub), 1), 1)}
    out["radius"] = rad

    dt = timed(lambda: ctx.knn_partition(cmap, q_scans, q_poses, 2, 0.01))
    out["knn_partition_k2_thr0.01"] = {"ms": round(1e3 * dt, 3), "queries_per_s": round(n_q / dt)}
    lib.ltm_search_free(ctx.h, s)

    if not args.no_cpu:
        from scipy.spatial import cKDTree
        t_host = cmap.download()[:, :3].astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(t_host)
        cpu = {"build_ms": round(1e3 * (time.perf_counter() - t0), 1), "workers": 16, "host_cpus_visible": os.cpu_count()}
        cq = host_q[np.linspace(0, n_q - 1, min(args.cpu_queries, n_q)).astype(np.int64), :3].astype(np.float64)
        for k in (1, 8):
            t0 = time.perf_counter()
            tree.query(cq, k=k, workers=16)
            dt = time.perf_counter() - t0
            cpu[f"k{k}"] = {"queries": len(cq), "queries_per_s": round(len(cq) / dt)}
        t0 = time.perf_counter()
        tree.query_ball_point(sub[:, :3].astype(np.float64), 0.5, workers=16, return_sorted=True)
        dt = time.perf_counter() - t0
        cpu["r0.5"] = {"queries": len(sub), "queries_per_s": round(len(sub) / dt)}
        out["ckdtree"] = cpu
        out["speedup_vs_ckdtree"] = {"k1": round(knn["k1"]["queries_per_s"] / cpu["k1"]["queries_per_s"], 1),
                                     "k8": round(knn["k8"]["queries_per_s"] / cpu["k8"]["queries_per_s"], 1),
                                     "r0.5": round(rad["r0.5"]["queries_per_s"] / cpu["r0.5"]["queries_per_s"], 1)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
