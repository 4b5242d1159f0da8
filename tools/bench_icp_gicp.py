"""Generalized ICP beside point-to-plane and point-to-point ICP on the device, on the workload of tools/bench_icp_plane.py: --pairs loop pairs between
two sessions of --n-kf keyframes of the synthetic lot (os1-64), source one keyframe of the query session, target the keyframes within +-25 of the same
index of the central session, both in map coordinates and voxel-gridded at 0.3 m.  All three methods are timed in ONE run.  Reported separately, because
a caller pays them once per index and not per alignment: the builds of the source indices (ltm_search_build, one call per source) and the normals of
sources and targets at --normal-k neighbours (one ltm_search_estimate_normals call each).  The generalized batch reads its sources in place from their
indices -- no per-call sort and no copy, which the other two methods pay inside their call ("prepare_ms": the profile class icp_prepare of one call;
absent from the generalized call).  Device times are HIP-event times on the context's stream, median of --steps runs after --warmup.  Writes one JSON
line to --out (default profiles/icp_gicp_lot-<pairs>.json) and prints it.

    python tools/bench_icp_gicp.py [--pairs 64] [--n-kf 128] [--normal-k 20] [--gicp-epsilon 1e-3] [--steps 7] [--warmup 2]"""
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
    ap.add_argument("--normal-k", type=int, default=20)
    ap.add_argument("--gicp-epsilon", type=float, default=1e-3)
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
    Qg, Qoff, Qpos = global_points(synth.make_session(2, args.n_kf, "os1-64", device=dev))
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
    t_view = np.ascontiguousarray(Cpos[kfs], dtype=np.float32)
    s_view = np.ascontiguousarray(Qpos[kfs], dtype=np.float32)
    ctx.synchronize()

    def timed(fn, warmup=None):
        """(median event ms, median wall ms)"""
        for _ in range(args.warmup if warmup is None else warmup):
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
    out = {"tool": "bench_icp_gicp", "workload": f"lot-2x{args.n_kf}-os1-64, {args.pairs} pairs, leaf {args.leaf} m, target +-{args.half_window} keyframes",
           "pairs": args.pairs, "source_points_mean": round(float(np.mean(n_src))), "target_points_mean": round(float(np.mean(n_tgt))),
           "normal_k": args.normal_k, "gicp_epsilon": args.gicp_epsilon, "fitness_threshold": args.fitness_threshold, "steps": args.steps,
           "warmup": args.warmup}

    # one-off costs: the sources' indices (rebuilt every run, the last set is kept), then the normals of both sides
    held = []

    def build_sources():
        for i in held:
            i.close()
        held[:] = [ctx.search_index(s) for s in sources]

    ev, wall = timed(build_sources)
    src_idx = list(held)
    out["one_off"] = {"source_index_builds": {"event_ms": round(ev, 3), "wall_ms": round(wall, 3), "calls": args.pairs, "points": int(np.sum(n_src))}}
    for what, idx, view, n in (("source_normals", src_idx, s_view, n_src), ("target_normals", indices, t_view, n_tgt)):
        ev, wall = timed(lambda: ctx.estimate_normals(idx, args.normal_k, view))
        out["one_off"][what] = {"event_ms": round(ev, 3), "wall_ms": round(wall, 3), "points": int(np.sum(n)),
                                "points_per_s": round(float(np.sum(n)) / (1e-3 * ev), 1) if ev > 0 else None}

    def summary(r, ev, wall):
        it = r["iterations"]
        return {"event_ms": round(ev, 3), "wall_ms": round(wall, 3), "ms_per_pair": round(wall / args.pairs, 4),
                "iterations": {"min": int(it.min()), "median": float(np.median(it)), "max": int(it.max())},
                "converged": int(r["converged"].sum()), "accepted": int(((r["converged"] != 0) & (r["fitness"] <= args.fitness_threshold)).sum()),
                "states": {capi.ICP_STATES[s]: int((r["state"] == s).sum()) for s in range(len(capi.ICP_STATES))},
                "fitness_median": float(np.median(r["fitness"]))}

    calls = {"gicp": lambda: ctx.icp_align(list(zip(indices, src_idx)), method="gicp", gicp_epsilon=args.gicp_epsilon),
             "plane": lambda: ctx.icp_align(list(zip(indices, sources)), method="plane"),
             "point": lambda: ctx.icp_align(list(zip(indices, sources)), method="point")}
    for method, call in calls.items():
        ev, wall = timed(lambda: res.__setitem__(method, call()))
        out[method] = summary(res[method], ev, wall)
        # what the call spends before its first iteration, from the library's own profile of one more call
        ctx.profile_enable(True)
        ctx.profile_reset()
        call()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        out[method]["prepare_ms"] = round(float(prof["icp_prepare"]["ms"]), 3) if "icp_prepare" in prof and "ms" in prof["icp_prepare"] else 0.0
        out[method]["iter_launches"] = int(prof["icp_iter"]["launches"]) if "icp_iter" in prof else None
    for a in ("plane", "point"):
        both = (res["gicp"]["converged"] != 0) & (res[a]["converged"] != 0)
        dT = np.abs(res["gicp"]["T"] - res[a]["T"]).reshape(args.pairs, -1).max(axis=1)
        out[f"max_abs_T_difference_gicp_{a}"] = {"pairs": int(both.sum()), "median": float(np.median(dT[both])) if both.any() else None,
                                                 "max": float(dT[both].max()) if both.any() else None}
    one_off = sum(v["wall_ms"] for v in out["one_off"].values())
    out["gicp_with_one_off_vs_point_wall"] = round(out["point"]["wall_ms"] / (out["gicp"]["wall_ms"] + one_off), 2)
    out["gicp_vs_point_wall"] = round(out["point"]["wall_ms"] / out["gicp"]["wall_ms"], 2)
    out["gicp_vs_plane_wall"] = round(out["plane"]["wall_ms"] / out["gicp"]["wall_ms"], 2)

    for i in indices + src_idx:
        i.close()
    ctx.close()
    line = json.dumps(out)
    path = args.out or os.path.join(ROOT, "profiles", f"icp_gicp_lot-{args.pairs}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
