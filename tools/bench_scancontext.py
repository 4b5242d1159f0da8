"""Scan Context on the device (ltm_sc_*) on the synthetic lot, two sessions of --n-kf keyframes (os1-64): descriptor construction of a session,
loop detection of the query session against the central one in the reference's default mode (3 ring-key candidates, 7 shifts) and in the
exhaustive mode (every database entry, every shift), each against the numpy restatement of the reference (tools/sc_numpy.py) on one CPU thread.
Device times are HIP-event times on the context's stream, median of --steps runs after --warmup; detection returns host arrays, so its wall
time (with the read-back) is given as well.  The CPU side runs on --cpu-kf keyframes / --cpu-queries queries and is scaled to the full size.
Writes one JSON line to --out (default profiles/scancontext_lot-2x<n-kf>.json) and prints it.

    python tools/bench_scancontext.py [--n-kf 500] [--steps 7] [--warmup 2]"""
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
    ap.add_argument("--n-kf", type=int, default=500)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-kf", type=int, default=20)
    ap.add_argument("--cpu-queries", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    from tools import sc_numpy as ref
    from tools import synth

    torch.set_num_threads(1)
    dev = "cuda:0"
    Cs = synth.make_session(1, args.n_kf, "os1-64", device=dev)
    Qs = synth.make_session(2, args.n_kf, "os1-64", device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(vfov=50.0, hfov=360.0, device=0)
    stream = torch.cuda.ExternalStream(ctx.stream())
    c_scans = ctx.scans_from_device(Cs["scans"].data_ptr(), Cs["offsets"].numpy().astype(np.uint64))
    q_scans = ctx.scans_from_device(Qs["scans"].data_ptr(), Qs["offsets"].numpy().astype(np.uint64))
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

    n_pts = int(Cs["offsets"][-1])
    out = {"tool": "bench_scancontext", "workload": f"lot-2x{args.n_kf}-os1-64, 20 x 60 descriptors", "keyframes": args.n_kf, "central_points": n_pts,
           "steps": args.steps, "warmup": args.warmup}

    def build():
        ctx.scan_contexts(c_scans).close()
    ev, _ = timed(build)
    out["build_session"] = {"event_ms": round(ev, 3), "points_per_s": round(n_pts / (ev * 1e-3))}

    db, qs = ctx.scan_contexts(c_scans), ctx.scan_contexts(q_scans)
    res = {}
    for name, over in (("detect_default", {}), ("detect_exhaustive", {"num_candidates": 0, "search_ratio": 1.0})):
        ev, wall = timed(lambda: res.__setitem__(name, db.detect(qs, **over)))
        pairs = args.n_kf * (3 if not over else args.n_kf)
        out[name] = {"event_ms": round(ev, 3), "wall_ms": round(wall, 3), "pairs": pairs, "pairs_per_s": round(pairs / (ev * 1e-3)),
                     "loops_found": int((res[name]["loop_id"] >= 0).sum())}

    # the numpy restatement on one thread, on a subset, scaled to the full size
    p = ref.params()
    desc_c, _, _ = db.download()
    desc_q, _, _ = qs.download()
    scans = Cs["scans"].cpu().numpy()
    off = Cs["offsets"].numpy()
    kfs = np.linspace(0, args.n_kf - 1, min(args.cpu_kf, args.n_kf)).astype(np.int64)
    t0 = time.perf_counter()
    same = 0
    for k in kfs:
        d = ref.descriptor(scans[int(off[k]):int(off[k + 1])], p)
        same += int((d == desc_c[k]).sum())
    cpu_build = (time.perf_counter() - t0) / len(kfs) * args.n_kf
    out["descriptor_bins_equal_to_restatement"] = round(same / (len(kfs) * d.size), 6)
    sub = np.linspace(0, args.n_kf - 1, min(args.cpu_queries, args.n_kf)).astype(np.int64)
    cpu = {"threads": 1, "build_session_ms_scaled": round(1e3 * cpu_build, 1), "keyframes_timed": len(kfs), "queries_timed": len(sub)}
    for name, pp in (("detect_default", p), ("detect_exhaustive", ref.params(num_candidates=0, search_ratio=1.0))):
        t0 = time.perf_counter()
        want = ref.detect(desc_c, desc_q[sub], pp)
        cpu[name + "_ms_scaled"] = round(1e3 * (time.perf_counter() - t0) / len(sub) * args.n_kf, 1)
        cpu[name + "_agrees"] = bool((want["nn_idx"] == res[name]["nn_idx"][sub]).all() and (want["nn_align"] == res[name]["nn_align"][sub]).all()
                                     and np.abs(want["min_dist"] - res[name]["min_dist"][sub]).max() <= 1e-12)
    out["numpy_restatement"] = cpu
    out["speedup_vs_numpy_1thread"] = {"build_session": round(cpu["build_session_ms_scaled"] / out["build_session"]["event_ms"], 1),
                                       "detect_default": round(cpu["detect_default_ms_scaled"] / out["detect_default"]["wall_ms"], 1),
                                       "detect_exhaustive": round(cpu["detect_exhaustive_ms_scaled"] / out["detect_exhaustive"]["wall_ms"], 1)}
    db.close()
    qs.close()
    ctx.close()
    line = json.dumps(out)
    path = args.out or os.path.join(ROOT, "profiles", f"scancontext_lot-2x{args.n_kf}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
