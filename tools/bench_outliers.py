"""Statistical and radius outlier removal (ltm_search_filter_statistical, ltm_search_filter_radius) on the outputs of a BASELINE configs[1] run (synthetic lot,
os1-64, 2 x --n-kf keyframes, 3-res removert):
 (a) nd_map + pd_map in one call (mean_k 50, PCL's tutorial setting; radius 0.5 m, 5 neighbours);
 (b) the central session's static-projected scans in one batch and with one call per scan.
Both filters are timed against the composition that exists without them: ltm_knn_search (resp. ltm_radius_search) with the target as the query, one cloud at a
time, and the reduction in torch (square roots and row sums in float64, mean and unbiased variance, the threshold; resp. the row lengths of the CSR).
Times are host clocks around calls that end in a device synchronise: the median of --steps samples after --warmup, with every sample and the spread (min,
max) in the record; the forms alternate inside every step, all rows in ONE run; index builds and uploads are outside the timed region.  The scans' mean_k is
the first of --scan-mean-k whose probe (one sample of every form) fits --budget-s when repeated warmup + steps times; the record says which.
 (c) what the statistical filter does to the clusters of nd_map (Context.cluster at tolerance 0.5 m, min_size 10) when it runs first.
The restatement (tools/outlier_numpy.py, scipy candidates) checks --check-scans scans and the maps' statistical result.  Prints one JSON line; --out also
writes it to a file.

    python tools/bench_outliers.py [--n-kf 500] [--steps 9] [--warmup 2] [--budget-s 150] [--out profiles/outliers_lot-2x500.json]"""
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

MAP_MEAN_K, STDDEV_MUL = 50, 1.0
RADIUS, MIN_NEIGHBORS = 0.5, 5
TOL, MIN_SIZE = 0.5, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-kf", type=int, default=500)
    ap.add_argument("--sensor", default="os1-64")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scan-mean-k", type=int, nargs="+", default=[50, 16, 8], help="candidates for the scans' mean_k, tried in this order")
    ap.add_argument("--budget-s", type=float, default=150.0, help="what the timed samples of one filter of one row may take in all")
    ap.add_argument("--check-scans", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_outliers needs a GPU (there is no CPU fallback)")
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    from ltmapper_amd.removerter import HipOps, Params, Removerter, Session
    from tools import outlier_numpy as oref
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
    maps = {k: rm.outputs[k].download() for k in ("nd_map", "pd_map")}
    scans_pts, scans_off = rm.central_sess_.keyframe_scans_static_projected_.download()
    n_kf = len(scans_off) - 1

    def sample(fns):
        ts = []
        for f in fns:
            t0 = time.perf_counter()
            f()
            ts.append(1e3 * (time.perf_counter() - t0))
        return ts

    def timed(fns):
        """--steps samples after --warmup; fewer samples (at least 3, the record says how many) only where the last warm-up says that they would not fit --budget-s"""
        last = [0.0]
        for _ in range(args.warmup):
            last = sample(fns)
        steps = args.steps if sum(last) / 1e3 * args.steps <= args.budget_s else max(3, int(args.budget_s / (sum(last) / 1e3)))
        ts = [[] for _ in fns]
        for _ in range(min(steps, args.steps)):
            for k, t in enumerate(sample(fns)):
                ts[k].append(t)
        return [{"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3), "samples": [round(x, 3) for x in t]} for t in ts]

    # ---- the forms.  clouds[i] is the target of indices[i]
    def sor_fused(indices, mean_k, each=False):
        def run():
            if each:
                for i in indices:
                    i.statistical_outliers(mean_k, STDDEV_MUL).close()
            else:
                ctx.statistical_outliers(indices, mean_k, STDDEV_MUL).close()
            ctx.synchronize()
        return run

    def ror_fused(indices, each=False):
        def run():
            if each:
                for i in indices:
                    i.radius_outliers(RADIUS, MIN_NEIGHBORS).close()
            else:
                ctx.radius_outliers(indices, RADIUS, MIN_NEIGHBORS).close()
            ctx.synchronize()
        return run

    def sor_baseline(indices, clouds, mean_k, keep=None):
        """ltm_knn_search of every cloud against its own index and the reduction in torch; keep: a list that receives the labels"""
        def run():
            for index, cloud in zip(indices, clouds):
                n = len(cloud)
                if not n:
                    continue
                _, d2 = index.knn(cloud, mean_k + 1, as_torch=True)
                fin = torch.isfinite(d2[:, 0])      # a non-finite query has no neighbours: its row is padding
                d = torch.where(torch.isfinite(d2[:, 1:]), d2[:, 1:], torch.zeros((), device=d2.device)).double().sqrt().sum(dim=1).div(mean_k).float()
                d = torch.where(fin, d, torch.zeros((), device=d.device))
                nf = int(fin.sum())
                mean = d.double().sum() / max(nf, 1)
                var = ((d.double() ** 2).sum() - d.double().sum() ** 2 / max(nf, 1)) / max(nf - 1, 1)
                labels = fin & (d.double() <= mean + STDDEV_MUL * var.clamp_min(0.0).sqrt())
                if keep is not None:
                    keep.append(labels.to(torch.uint8).cpu().numpy())
            torch.cuda.synchronize()
        return run

    def ror_baseline(indices, clouds, keep=None):
        """ltm_radius_search of every cloud against its own index; the count of a point is the length of its CSR row"""
        def run():
            for index, cloud in zip(indices, clouds):
                if not len(cloud):
                    continue
                off, _, _ = index.radius(cloud, RADIUS, as_torch=True)
                labels = (off[1:] - off[:-1]) >= MIN_NEIGHBORS
                if keep is not None:
                    keep.append(labels.to(torch.uint8).cpu().numpy())
            torch.cuda.synchronize()
        return run

    def counters(run):
        ctx.outlier_stats(reset=True)
        run()
        return ctx.outlier_stats(reset=True)

    def row(name, indices, clouds, mean_k, with_each):
        """both filters over `indices`: the batch, (one call per index,) the composition; agreement of the composition's labels with the batch's"""
        r = {"points": int(sum(len(c) for c in clouds)), "records": len(indices), "mean_k": mean_k, "stddev_mul": STDDEV_MUL, "radius": RADIUS,
             "min_neighbors": MIN_NEIGHBORS}
        for filt, fused, base in (("statistical", lambda each=False: sor_fused(indices, mean_k, each), lambda keep=None: sor_baseline(indices, clouds, mean_k, keep)),
                                  ("radius", lambda each=False: ror_fused(indices, each), lambda keep=None: ror_baseline(indices, clouds, keep))):
            fns = [fused(), base()] + ([fused(True)] if with_each else [])
            t = timed(fns)
            f = {"batch_ms": t[0]["median"], "composition_ms": t[1]["median"], "batch_timing": t[0], "composition_timing": t[1],
                 "composition_over_batch": round(t[1]["median"] / max(t[0]["median"], 1e-9), 2)}
            if with_each:
                f.update({"one_call_per_index_ms": t[2]["median"], "one_call_per_index_timing": t[2],
                          "one_call_per_index_over_batch": round(t[2]["median"] / max(t[0]["median"], 1e-9), 2)})
            f["counters"] = counters(fns[0])
            f["points_per_ms"] = round(f["counters"]["finite_points"] / max(t[0]["median"], 1e-9), 1)
            f["distance_evaluations_per_point"] = round(f["counters"]["distance_evaluations"] / max(f["counters"]["finite_points"], 1), 2)
            kept = []
            base(kept)()
            with (ctx.statistical_outliers(indices, mean_k, STDDEV_MUL) if filt == "statistical" else ctx.radius_outliers(indices, RADIUS, MIN_NEIGHBORS)) as out:
                labels = out.labels()
                f["kept"], f["removed"] = int(out.n_kept.sum()), int(out.n_target.sum() - out.n_kept.sum())
            theirs = np.concatenate(kept) if kept else np.zeros(0, np.uint8)
            f["labels_that_differ_from_the_composition"] = int((labels != theirs).sum())      # torch sums in another order: a point within rounding of the threshold may differ
            r[filt] = f
            print(f"bench_outliers: {name} {filt}: batch {f['batch_ms']} ms, composition {f['composition_ms']} ms", file=sys.stderr, flush=True)
        return r

    out = {"tool": "bench_outliers", "workload": f"lot-2x{args.n_kf}-{args.sensor}-3res", "steps": args.steps, "warmup": args.warmup}

    # ---- (a) the two maps in one call
    map_pts = [maps["nd_map"], maps["pd_map"]]
    map_clouds = [ctx.upload(p) for p in map_pts]
    map_idx = [ctx.search_index(c) for c in map_clouds]
    out["maps"] = row("maps", map_idx, map_clouds, MAP_MEAN_K, with_each=False)
    out["maps"]["points_each"] = [len(p) for p in map_pts]
    with ctx.statistical_outliers(map_idx, MAP_MEAN_K, STDDEV_MUL) as dev_out:
        off, lab, dist, thr = dev_out.offsets(), dev_out.labels(), dev_out.distances(), dev_out.threshold
        agree = True
        for k, p in enumerate(map_pts):
            want = oref.statistical_large(p, MAP_MEAN_K, STDDEV_MUL)
            a, b = int(off[k]), int(off[k + 1])
            agree = agree and want["distances"].tobytes() == dist[a:b].tobytes() and want["threshold"] == thr[k] and (want["labels"] == lab[a:b]).all()
        out["maps"]["statistical"]["restatement_agrees"] = bool(agree)

        # ---- (c) the clusters of nd_map with and without the statistical filter in front
        def cluster_figures(index):
            with index.cluster(TOL, MIN_SIZE) as cl:
                nt, nc, npts = cl.info()
                return {"points": nt, "clusters": nc, "clustered_points": npts, "largest_cluster": int(cl.sizes[0]) if nc else 0}
        with ctx.statistical_outliers(map_idx[:1], MAP_MEAN_K, STDDEV_MUL) as nd_out:
            kept, removed = nd_out.split(map_clouds[0])
        with ctx.search_index(kept) as kept_idx:
            out["nd_map_clusters"] = {"tolerance": TOL, "min_size": MIN_SIZE, "mean_k": MAP_MEAN_K, "stddev_mul": STDDEV_MUL, "as_it_is": cluster_figures(map_idx[0]),
                                      "after_the_statistical_filter": cluster_figures(kept_idx)}
        kept.free()
        removed.free()
    for i in map_idx:
        i.close()

    # ---- (b) the static-projected scans of the central session
    ss = ctx.upload_scans(scans_pts, scans_off)
    indices = ctx.search_index_batch(ss)
    clouds = [ctx.upload(scans_pts[int(scans_off[k]):int(scans_off[k + 1])]) for k in range(n_kf)]
    probes = {}
    scan_mean_k = args.scan_mean_k[-1]
    for mk in args.scan_mean_k:      # the probe is one sample of every form (and warms them up)
        probes[mk] = round(sum(sample([sor_fused(indices, mk), sor_baseline(indices, clouds, mk), sor_fused(indices, mk, True)])) / 1e3, 2)
        print(f"bench_outliers: probe mean_k {mk}: {probes[mk]} s per sample of the three forms", file=sys.stderr, flush=True)
        if probes[mk] * (args.steps + args.warmup) <= args.budget_s:
            scan_mean_k = mk
            break
    out["scans"] = row("scans", indices, clouds, scan_mean_k, with_each=True)
    out["scans"]["mean_k_probe_s"] = probes
    out["scans"]["budget_s"] = args.budget_s
    sub = sorted(set(np.linspace(0, n_kf - 1, min(args.check_scans, n_kf)).astype(int).tolist())) if n_kf else []
    agree = True
    for k in sub:
        p = scans_pts[int(scans_off[k]):int(scans_off[k + 1])]
        with indices[k].statistical_outliers(scan_mean_k, STDDEV_MUL) as a, indices[k].radius_outliers(RADIUS, MIN_NEIGHBORS) as b:
            ws, wr = oref.statistical_large(p, scan_mean_k, STDDEV_MUL), oref.radius_large(p, RADIUS, MIN_NEIGHBORS)
            agree = agree and ws["distances"].tobytes() == a.distances().tobytes() and (ws["labels"] == a.labels()).all() and ws["threshold"] == a.threshold[0]
            agree = agree and (wr["counts"] == b.counts()).all() and (wr["labels"] == b.labels()).all()
    out["scans"]["restatement"] = {"scans": len(sub), "agrees": bool(agree)}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
