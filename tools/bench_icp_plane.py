"""Point-to-plane against point-to-point ICP on the device, on the workload of tools/bench_icp.py: --pairs loop pairs between two sessions of --n-kf
keyframes of the synthetic lot (os1-64), source one keyframe of the query session, target the keyframes within +-25 of the same index of the central
session, both in map coordinates and voxel-gridded at 0.3 m.  Timed in one run: the normals of all targets in one call (ltm_search_estimate_normals,
--normal-k neighbours, the viewpoint at the key keyframe's position), the plane batch (ltm_icp_align_plane) and the point batch (ltm_icp_align); reported
with them the iteration counts and the accept counts (converged and fitness <= --fitness-threshold) of both methods and how far their transforms are
apart.  Device times are HIP-event times on the context's stream, median of --steps runs after --warmup.  Writes one JSON line to --out (default
profiles/icp_plane_lot-<pairs>.json) and prints it.

    python tools/bench_icp_plane.py [--pairs 64] [--n-kf 128] [--normal-k 10] [--steps 7] [--warmup 2]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--n-kf", type=int, default=128)
    ap.add_argument("--half-window", type=int, default=25)
    ap.add_argument("--leaf", type=float, default=0.3)
    ap.add_argument("--normal-k", type=int, default=10)
    ap.add_argument("--fitness-threshold", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    from tools import synth

    torch.set_num_threads(1)
    dev = "cuda:0"
    ctx = capi.Context(vfov=50.0, hfov=360.0, device=0)
    stream = torch.cuda.ExternalStream(ctx.stream())

    def global_points(sess):
        """every scan point in map coordinates (float), the keyframe offsets and the keyframe positions"""
        off = sess["offsets"].numpy().astype(np.int64)
        kf = torch.repeat_interleave(torch.arange(len(off) - 1, device=dev), torch.as_tensor(np.diff(off), device=dev))
        poses = np.asarray(sess["poses"]).reshape(-1, 4, 4)
        P = torch.as_tensor(poses, device=dev)
        x = sess["scans"][:, :3].double()
        g = torch.einsum("nij,nj->ni", P[kf, :3, :3], x) + P[kf, :3, 3]
        out = sess["scans"].clone()
        out[:, :3] = g.float()
        return out.contiguous(), off, poses[:, :3, 3]

    Cg, Coff, Cpos = global_points(synth.make_session(1, args.n_kf, "os1-64", device=dev))
    Qg, Qoff, _ = global_points(synth.make_session(2, args.n_kf, "os1-64", device=dev))
    torch.cuda.synchronize()

    def gridded(pts, off, a, b):
        raw = ctx.cloud_from_device(pts[off[a]:off[b]].data_ptr(), int(off[b] - off[a]))
        out = ctx.voxel_centroid(raw, args.leaf)
        raw.free()
        return out

    kfs = np.linspace(0, args.n_kf - 1, args.pairs).astype(np.int64)
    sources = [gridded(Qg, Qoff, int(k), int(k) + 1) for k in kfs]
    targets = [gridded(Cg, Coff, max(int(k) - args.half_window, 0), min(int(k) + args.half_window + 1, args.n_kf)) for k in kfs]
    indices = [ctx.search_index(t) for t in targets]
    viewpoints = np.ascontiguousarray(Cpos[kfs], dtype=np.float32)
    pairs = list(zip(indices, sources))
    ctx.synchronize()

    def timed(fn):
        """(median event ms, median wall ms)"""
        for _ in range(args.warmup):
            fn()
        ctx.synchronize()
        ev, wall = [], []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(a.elapsed_time(b))
        return statistics.median(ev), statistics.median(wall)

    res = {}
    n_src = [len(s) for s in sources]
    n_tgt = [len(t) for t in targets]
    out = {"tool": "bench_icp_plane", "workload": f"lot-2x{args.n_kf}-os1-64, {args.pairs} pairs, leaf {args.leaf} m, target +-{args.half_window} keyframes",
           "pairs": args.pairs, "source_points_mean": round(float(np.mean(n_src))), "target_points_mean": round(float(np.mean(n_tgt))),
           "normal_k": args.normal_k, "fitness_threshold": args.fitness_threshold, "steps": args.steps, "warmup": args.warmup}

    ev, wall = timed(lambda: ctx.estimate_normals(indices, args.normal_k, viewpoints))
    out["normals"] = {"event_ms": round(ev, 3), "wall_ms": round(wall, 3), "target_points": int(np.sum(n_tgt)),
                      "points_per_s": round(float(np.sum(n_tgt)) / (1e-3 * ev), 1) if ev > 0 else None}

    def summary(r, ev, wall):
        it = r["iterations"]
        return {"event_ms": round(ev, 3), "wall_ms": round(wall, 3), "ms_per_pair": round(wall / args.pairs, 4),
                "iterations": {"min": int(it.min()), "median": float(np.median(it)), "max": int(it.max())},
                "converged": int(r["converged"].sum()), "accepted": int(((r["converged"] != 0) & (r["fitness"] <= args.fitness_threshold)).sum()),
                "states": {capi.ICP_STATES[s]: int((r["state"] == s).sum()) for s in range(len(capi.ICP_STATES))},
                "fitness_median": float(np.median(r["fitness"]))}

    for method in ("plane", "point"):
        ev, wall = timed(lambda: res.__setitem__(method, ctx.icp_align(pairs, method=method)))
        out[method] = summary(res[method], ev, wall)
    out["plane_with_normals_vs_point_wall"] = round(out["point"]["wall_ms"] / (out["plane"]["wall_ms"] + out["normals"]["wall_ms"]), 2)
    out["plane_vs_point_wall"] = round(out["point"]["wall_ms"] / out["plane"]["wall_ms"], 2)
    both = (res["plane"]["converged"] != 0) & (res["point"]["converged"] != 0)
    dT = np.abs(res["plane"]["T"] - res["point"]["T"]).reshape(args.pairs, -1).max(axis=1)
    out["max_abs_T_difference_between_methods"] = {"pairs": int(both.sum()), "median": float(np.median(dT[both])) if both.any() else None,
                                                   "max": float(dT[both].max()) if both.any() else None}

    for i in indices:
        i.close()
    ctx.close()
    line = json.dumps(out)
    path = args.out or os.path.join(ROOT, "profiles", f"icp_plane_lot-{args.pairs}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
