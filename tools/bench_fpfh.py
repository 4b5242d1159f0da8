"""FPFH descriptors (ltm_search_fpfh) on the outputs of a BASELINE configs[1] run (synthetic lot, os1-64, 2 x --n-kf keyframes, 3-res removert):
 (a) nd_map + pd_map in one call;
 (b) the central session's static-projected scans in one batch and with one call per scan;
each at every k of --k (10: the register lists, 32: the LDS lists), normals estimated beforehand at k = 10 (outside the timed region, like the index builds
and uploads).  The call is timed against the composition that exists without it: ltm_knn_search with the target as the query, the normals download, and the
histogram step of the restatement (tools/fpfh_numpy.py: pair features, bins, counts, weights, normalisation) written in torch on the device in float64, one
cloud at a time.  A second context created with LTM_FPFH_LISTS=0 runs the same batch with the weights collecting the neighbourhoods again instead of reading the
lists the first pass stored (the "collect twice" column).  Times are host clocks around calls that end in a device synchronise: the median of --steps samples after --warmup, with every sample and
the spread (min, max) in the record; the forms alternate inside every step, all rows in ONE run.  Where the last warm-up says that --steps samples of a row
would not fit --budget-s, fewer are taken (at least 3; the record says how many).  The composition is compared with the call's result (rows that differ:
torch may fuse or reorder, so equality is not expected of it), and tools/fpfh_numpy.py checks --check-scans scans for equality.  Prints one JSON line; --out
also writes it to a file.

    python tools/bench_fpfh.py [--n-kf 500] [--k 10 32] [--steps 5] [--warmup 1] [--budget-s 60] [--out profiles/fpfh_lot-2x500.json]"""
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

NORMALS_K = 10


def torch_histogram_step(torch, pts, normals, idx, d2):
    """the restatement's steps after the neighbourhoods, in torch float64 on the device: pts (n, 3) float32, normals (n, 3) float32, idx (n, k) int64 (-1:
    padding), d2 (n, k) float32 -> (n, 33) float32.  Rows of non-finite points come out NaN."""
    from tools import fpfh_numpy as fref
    n, k = idx.shape
    dev = pts.device
    p, nr = pts.double(), normals.double()
    valid = torch.isfinite(p).all(dim=1) & torch.isfinite(nr).all(dim=1)
    rows = torch.arange(n, device=dev)[:, None].expand(n, k)
    live = idx >= 0
    q = idx.clamp_min(0)

    def dot(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    def cross(a, b):
        return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                            a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)

    n_p, n_q = nr[:, None, :].expand(n, k, 3), nr[q]
    d = p[q] - p[:, None, :]
    f4 = dot(d, d).sqrt()
    a1, a2 = dot(n_p, d) / f4, dot(n_q, d) / f4
    swap = a1.abs() < a2.abs()
    u = torch.where(swap[..., None], n_q, n_p)
    other = torch.where(swap[..., None], n_p, n_q)
    d = torch.where(swap[..., None], -d, d)
    phi = torch.where(swap, -a2, a1)
    v = cross(d, u)
    vn = dot(v, v).sqrt()
    v = v / vn[..., None]
    w = cross(u, v)
    alpha, y, x = dot(v, other), dot(w, other), dot(u, other)
    use = live & (q != rows) & valid[:, None] & (f4 != 0.0) & (vn != 0.0) & torch.isfinite(n_q).all(dim=-1)

    def bin_unit(f):
        return torch.nan_to_num(torch.floor(11.0 * ((f + 1.0) * 0.5)), nan=0.0).clamp(0.0, 10.0).long()

    upper = ~torch.signbit(y)
    bt = torch.zeros_like(q)
    for j, (c, s) in enumerate(fref.THETA_TABLE, start=1):
        side = (c * y - s * x) >= 0.0
        bt += ((upper | side) if j <= 5 else (upper & side)).long()
    bt = torch.where((x == 0.0) & (y == 0.0), torch.full_like(bt, 5), bt)
    counts = torch.zeros((n, 33), dtype=torch.float64, device=dev)
    one = use.double().reshape(-1)
    flat_rows = rows.reshape(-1)
    for base, b in ((0, bin_unit(alpha)), (11, bin_unit(phi)), (22, bt)):
        counts.index_put_((flat_rows, (base + b).reshape(-1)), one, accumulate=True)      # integers below 64 in float64: exact in any order
    S = torch.zeros((n, 33), dtype=torch.float64, device=dev)
    for j in range(k):
        wj = 1.0 / d2[:, j].double()
        ok = live[:, j] & (d2[:, j] != 0.0)
        S = torch.where(ok[:, None], S + wj[:, None] * counts[q[:, j]], S)
    S = S.reshape(n, 3, 11)
    T = S[:, :, 0]
    for b in range(1, 11):
        T = T + S[:, :, b]
    out = torch.where((T == 0.0)[..., None], torch.zeros((), dtype=torch.float64, device=dev), 100.0 * S / T[..., None]).reshape(n, 33).float()
    out[~valid] = math.nan
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-kf", type=int, default=500)
    ap.add_argument("--sensor", default="os1-64")
    ap.add_argument("--k", type=int, nargs="+", default=[10, 32])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--budget-s", type=float, default=60.0, help="what the timed samples of one row may take in all")
    ap.add_argument("--check-scans", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fpfh needs a GPU (there is no CPU fallback)")
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    from ltmapper_amd.removerter import HipOps, Params, Removerter, Session
    from tools import fpfh_numpy as fref
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
    print(f"bench_fpfh: maps {[len(m) for m in maps.values()]}, {n_kf} scans of {len(scans_pts)} points", file=sys.stderr, flush=True)

    def sample(fns):
        ts = []
        for f in fns:
            t0 = time.perf_counter()
            f()
            ts.append(1e3 * (time.perf_counter() - t0))
        return ts

    def timed(fns):
        last = [0.0]
        for _ in range(args.warmup):
            last = sample(fns)
        steps = args.steps if sum(last) / 1e3 * args.steps <= args.budget_s else max(3, int(args.budget_s / (sum(last) / 1e3)))
        ts = [[] for _ in fns]
        for _ in range(min(steps, args.steps)):
            for j, t in enumerate(sample(fns)):
                ts[j].append(t)
        return [{"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3), "samples": [round(x, 3) for x in t]} for t in ts]

    def fused(indices, k, each=False, on=None):
        on = on or ctx

        def run():
            if each:
                for i in indices:
                    i.fpfh(k).close()
            else:
                on.fpfh(indices, k).close()
            on.synchronize()
        return run

    os.environ["LTM_FPFH_LISTS"] = "0"
    ctx_twice = capi.Context(vfov=50.0, hfov=360.0, device=0)      # the weights collect again: never the stored lists
    del os.environ["LTM_FPFH_LISTS"]

    def composition(indices, clouds, xyz, k, keep=None):
        """per cloud: ltm_knn_search against its own index, the normals download, the histogram step in torch (xyz: the cloud's points as a torch tensor on the
        device, made outside the timed region); keep: a list that receives the rows"""
        def run():
            for index, cloud, pts in zip(indices, clouds, xyz):
                if not len(cloud):
                    continue
                idx, d2 = index.knn(cloud, k, as_torch=True)
                normals = torch.from_numpy(index.normals()[:, :3].copy()).to(dev)
                rows = torch_histogram_step(torch, pts, normals, idx.reshape(len(cloud), k).long(), d2.reshape(len(cloud), k))
                if keep is not None:
                    keep.append(rows.cpu().numpy())
            torch.cuda.synchronize()
        return run

    def row(name, indices, clouds, xyz, k, with_each, twice):
        r = {"points": int(sum(len(c) for c in clouds)), "records": len(indices), "k": k, "normals_k": NORMALS_K}
        fns = [fused(indices, k), composition(indices, clouds, xyz, k)] + ([fused(indices, k, True)] if with_each else []) + [fused(twice, k, on=ctx_twice)]
        t = timed(fns)
        r.update({"collect_twice_ms": t[-1]["median"], "collect_twice_timing": t[-1], "collect_twice_over_stored_lists": round(t[-1]["median"] / max(t[0]["median"], 1e-9), 2)})
        with ctx_twice.fpfh(twice[:4], k) as out:
            twice_rows = out.descriptors()
        r.update({"batch_ms": t[0]["median"], "composition_ms": t[1]["median"], "batch_timing": t[0], "composition_timing": t[1],
                  "composition_over_batch": round(t[1]["median"] / max(t[0]["median"], 1e-9), 2)})
        if with_each:
            r.update({"one_call_per_index_ms": t[2]["median"], "one_call_per_index_timing": t[2],
                      "one_call_per_index_over_batch": round(t[2]["median"] / max(t[0]["median"], 1e-9), 2)})
        ctx.fpfh_stats(reset=True)
        fns[0]()
        r["counters"] = ctx.fpfh_stats(reset=True)
        r["points_per_ms"] = round(r["counters"]["finite_points"] / max(t[0]["median"], 1e-9), 1)
        r["distance_evaluations_per_point"] = round(r["counters"]["distance_evaluations"] / max(r["counters"]["finite_points"], 1), 2)
        theirs = []
        composition(indices[:4], clouds[:4], xyz[:4], k, theirs)()
        with ctx.fpfh(indices[:4], k) as out:
            mine = out.descriptors()
        theirs = np.concatenate(theirs) if theirs else np.zeros((0, 33), np.float32)
        same = (mine.view(np.uint32) == theirs.view(np.uint32)) | (np.isnan(mine) & np.isnan(theirs))
        r["collect_twice_equals_stored_lists"] = bool(twice_rows.tobytes() == mine.tobytes())
        r["composition_check"] = {"records": min(4, len(indices)), "rows": int(len(mine)), "rows_that_differ": int((~same.all(axis=1)).sum()),
                                  "largest_difference": float(np.nanmax(np.abs(mine - theirs))) if len(mine) else 0.0}
        print(f"bench_fpfh: {name} k {k}: batch {r['batch_ms']} ms, composition {r['composition_ms']} ms"
              + (f", one call per index {r['one_call_per_index_ms']} ms" if with_each else "") + f", collect twice {r['collect_twice_ms']} ms", file=sys.stderr, flush=True)
        return r

    out = {"tool": "bench_fpfh", "workload": f"lot-2x{args.n_kf}-{args.sensor}-3res", "steps": args.steps, "warmup": args.warmup, "budget_s": args.budget_s,
           "timing": "host clock around calls that end in a device synchronise; median of the samples listed; forms alternate inside every step"}

    # ---- (a) the two maps in one call
    map_pts = [maps["nd_map"], maps["pd_map"]]
    map_clouds = [ctx.upload(p) for p in map_pts]
    map_idx = [ctx.search_index(c) for c in map_clouds]
    ctx.estimate_normals(map_idx, NORMALS_K)
    map_xyz = [torch.from_numpy(np.ascontiguousarray(p[:, :3])).to(dev) for p in map_pts]
    map_twice = [ctx_twice.search_index(p) for p in map_pts]
    ctx_twice.estimate_normals(map_twice, NORMALS_K)
    out["maps"] = {f"k{k}": row("maps", map_idx, map_clouds, map_xyz, k, True, map_twice) for k in args.k}
    for i in map_twice:
        i.close()
    out["maps"]["points_each"] = [len(p) for p in map_pts]
    for i in map_idx:
        i.close()
    for c in map_clouds:
        c.free()

    # ---- (b) the static-projected scans of the central session
    ss = ctx.upload_scans(scans_pts, scans_off)
    indices = ctx.search_index_batch(ss)
    ctx.estimate_normals(indices, NORMALS_K)
    clouds = [ctx.upload(scans_pts[int(scans_off[j]):int(scans_off[j + 1])]) for j in range(n_kf)]
    all_xyz = torch.from_numpy(np.ascontiguousarray(scans_pts[:, :3])).to(dev)
    xyz = [all_xyz[int(scans_off[j]):int(scans_off[j + 1])] for j in range(n_kf)]
    ss_twice = ctx_twice.upload_scans(scans_pts, scans_off)
    twice = ctx_twice.search_index_batch(ss_twice)
    ctx_twice.estimate_normals(twice, NORMALS_K)
    out["scans"] = {f"k{k}": row("scans", indices, clouds, xyz, k, True, twice) for k in args.k}
    sub = sorted(set(np.linspace(0, n_kf - 1, min(args.check_scans, n_kf)).astype(int).tolist())) if n_kf else []
    agree = True
    for j in sub:
        p = scans_pts[int(scans_off[j]):int(scans_off[j + 1])][:4000]      # brute-force neighbourhoods: the first 4000 points of the scan, as a cloud of their own
        with ctx.search_index(p) as index:
            index.estimate_normals(NORMALS_K)
            normals = index.normals()[:, :3]
            for k in args.k:
                with index.fpfh(k) as a:
                    want = fref.fpfh(p, normals, k)
                    got = a.descriptors()
                    same = (got.view(np.uint32) == want["descriptors"].view(np.uint32)) | (np.isnan(got) & np.isnan(want["descriptors"]))
                    agree = agree and bool(same.all()) and bool((a.spfh_counts() == want["spfh_counts"]).all())
    out["scans"]["restatement"] = {"scans": len(sub), "points_each": 4000, "agrees": bool(agree)}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)
    ctx_twice.close()
    ctx.close()


if __name__ == "__main__":
    main()
