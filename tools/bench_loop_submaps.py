"""The step between a loop proposal and its ICP verification on the device, on the workload of tools/bench_icp.py: the synthetic lot, two sessions of
--n-kf keyframes (os1-64), --pairs loop pairs (k, k), target submaps of +-25 keyframes (CentralCoord: every keyframe moved by the float affine of its
pose), source submaps of one keyframe, pcl::VoxelGrid at 0.3 m.  Timed:
  (a) batched       Context.loop_submaps + Context.search_index_batch for all targets and all sources;
  (b) per window    the same outputs made window by window from calls the library had before: scan_of_keyframe per keyframe, concat, one
                    voxel_grid_scanset and one search_index per window (the baseline; the float transform of every keyframe is done once on the host
                    beforehand and timed on its own); the ICP results over (a)'s and (b)'s outputs must be the same bytes;
  (c) order         (a) with order "input" against order "pcl";
  (d) end to end    scan_contexts(...).detect -> verify_loops -> accepted loops.
Device times are HIP-event times on the context's stream, wall times perf_counter around the same region, median of --steps runs after --warmup.  The
gather's own time comes from the library's profile class submap_assemble (32 B / point) and is quoted as a fraction of an 8 TB/s HBM roofline.
Writes one JSON line to --out (default profiles/loop_submaps_lot-<pairs>.json) and prints it.

    python tools/bench_loop_submaps.py [--pairs 64] [--n-kf 128] [--steps 7] [--warmup 2]"""
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

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--n-kf", type=int, default=128)
    ap.add_argument("--half-window", type=int, default=25)
    ap.add_argument("--leaf", type=float, default=0.3)
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

    def session(i):
        s = synth.make_session(i, args.n_kf, "os1-64", device=dev)
        off = s["offsets"].cpu().numpy().astype(np.uint64)
        P = np.asarray(s["poses"]).reshape(-1, 4, 4)
        p6 = np.stack([P[:, 0, 3], P[:, 1, 3], P[:, 2, 3], np.zeros(len(P)), np.zeros(len(P)), np.arctan2(P[:, 1, 0], P[:, 0, 0])], axis=1).astype(np.float32)
        aff = capi.pose6d_to_affine3f(p6)
        pts = s["scans"].contiguous()
        torch.cuda.synchronize()
        return ctx.scans_from_device(pts.data_ptr(), off), aff, off

    tscans, taff, toff = session(1)
    sscans, saff, soff = session(2)
    keys = np.linspace(0, args.n_kf - 1, args.pairs).astype(np.int64)
    sn = args.half_window

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

    keep = {}

    def drop(name):
        for x in keep.pop(name, ()):
            x.close() if isinstance(x, capi.SearchIndex) else x.free()

    def batched(order="pcl", name="a"):
        drop(name)
        tsub = ctx.loop_submaps(tscans, keys, sn, args.leaf, taff, order)
        ssub = ctx.loop_submaps(sscans, keys, 0, args.leaf, saff, order)
        idx = ctx.search_index_batch(tsub)
        sidx = ctx.search_index_batch(ssub)
        keep[name] = [tsub, ssub] + idx + sidx
        return tsub, ssub, idx

    # (b): what the library offered before.  It had no float-affine transform on the device (ltm_cloud_transform is the double-matrix one), so the keyframes
    # are moved ONCE each on the host by the numpy restatement of the same float arithmetic and uploaded again (timed on its own, outside the per-window
    # time: a caller would do it once per session); then every window is scan_of_keyframe x n, concat, one voxel_grid_scanset, one search_index
    from tools import submap_numpy as ref

    def pretransform(scans, aff, off):
        pts = scans.download()[0]
        moved = np.concatenate([ref.transform(pts[int(off[k]):int(off[k + 1])], aff[k]) for k in range(len(off) - 1)])
        return ctx.upload_scans(moved, off)

    t0 = time.perf_counter()
    tpre, spre = pretransform(tscans, taff, toff), pretransform(sscans, saff, soff)
    pre_ms = 1e3 * (time.perf_counter() - t0)

    def old_window(scans, key, half):
        parts = [ctx.scan_of_keyframe(scans, k) for k in range(max(key - half, 0), min(key + half, args.n_kf - 1) + 1)]
        cat = ctx.concat(parts)
        for p in parts:
            p.free()
        one = ctx.scans_from_device(cat.device_ptr(), np.array([0, len(cat)], np.uint64))
        grid = ctx.voxel_grid_scanset(one, args.leaf)
        sub = ctx.scan_of_keyframe(grid, 0)
        for x in (cat, one, grid):
            x.free()
        return sub, ctx.search_index(sub)

    def per_window():
        drop("b")
        made = []
        for k in keys:
            made += list(old_window(tpre, int(k), sn))
            made += list(old_window(spre, int(k), 0))
        keep["b"] = made

    out = {"tool": "bench_loop_submaps", "workload": f"lot-2x{args.n_kf}-os1-64, {args.pairs} pairs, leaf {args.leaf} m, target +-{sn} keyframes",
           "pairs": args.pairs, "steps": args.steps, "warmup": args.warmup}

    ev_a, wall_a = timed(batched)
    tsub, ssub, idx = batched()
    pre = int(sum(int(toff[min(int(k) + sn, args.n_kf - 1) + 1] - toff[max(int(k) - sn, 0)]) for k in keys) + sum(int(soff[int(k) + 1] - soff[int(k)]) for k in keys))
    out["points_before_grid"] = pre
    out["target_points_mean"] = round(tsub.info()[1] / args.pairs)
    out["source_points_mean"] = round(ssub.info()[1] / args.pairs)
    out["batched"] = {"event_ms": round(ev_a, 3), "wall_ms": round(wall_a, 3), "indices": 2 * args.pairs,
                      "host_read_backs_per_index_batch": 1, "host_read_backs_per_gridded_assembly": 3}
    res_a = ctx.icp_align([(idx[j], (ssub, j)) for j in range(args.pairs)])

    ev_b, wall_b = timed(per_window)
    made = keep["b"]
    res_b = ctx.icp_align([(made[4 * j + 1], made[4 * j + 2]) for j in range(args.pairs)])
    out["per_window"] = {"event_ms": round(ev_b, 3), "wall_ms": round(wall_b, 3), "host_pretransform_once_wall_ms_not_included": round(pre_ms, 1)}
    out["batched_vs_per_window_wall"] = round(wall_b / wall_a, 2)
    out["icp_results_equal_bytes"] = bool(res_a.tobytes() == res_b.tobytes())
    out["icp_max_abs_T_difference"] = float(np.abs(res_a["T"] - res_b["T"]).max())
    out["icp_discrete_fields_equal"] = bool(all((res_a[f] == res_b[f]).all() for f in ("converged", "iterations", "state", "n_corr")))
    drop("b")

    # the gather alone, from the library's profile class
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(args.steps):
        ctx.loop_submaps(tscans, keys, sn, 0.0, taff).free()
    prof = ctx.profile_read().get("submap_assemble")
    ctx.profile_enable(False)
    if prof and prof["ms"] > 0:
        out["gather"] = {"launches": prof["launches"], "points_per_launch": int(prof["units"] / prof["launches"]), "ms_per_launch": round(prof["ms"] / prof["launches"], 4),
                         "bytes_per_point": 32, "hbm_roofline_frac_of_8TBs": round(prof["bytes"] / (1e-3 * prof["ms"]) / HBM_BYTES_PER_S, 3)}

    ev_i, wall_i = timed(lambda: batched("input", "c"))
    drop("c")
    out["order"] = {"pcl": {"event_ms": round(ev_a, 3), "wall_ms": round(wall_a, 3)}, "input": {"event_ms": round(ev_i, 3), "wall_ms": round(wall_i, 3)},
                    "pcl_vs_input_wall": round(wall_a / wall_i, 2)}

    def end_to_end():
        with ctx.scan_contexts(tscans) as db, ctx.scan_contexts(sscans) as qs:
            det = db.detect(qs)
        loop_id = det["loop_id"]
        pairs = [(int(t), int(q)) for q, t in enumerate(loop_id) if t >= 0]
        keep["d"] = (pairs,) + tuple(ctx.verify_loops(tscans, sscans, pairs, taff, saff, search_num=sn, leaf=args.leaf)) if pairs else (pairs, None, None)

    ev_d, wall_d = timed(end_to_end)
    pairs, res_d, acc = keep.pop("d")
    out["detect_to_accepted"] = {"event_ms": round(ev_d, 3), "wall_ms": round(wall_d, 3), "proposed": len(pairs), "accepted": int(acc.sum()) if acc is not None else 0}

    drop("a")
    ctx.close()
    line = json.dumps(out)
    path = args.out or os.path.join(ROOT, "profiles", f"loop_submaps_lot-{args.pairs}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
