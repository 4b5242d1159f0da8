"""Batched ICP on the device (ltm_icp_align) on the synthetic lot: --pairs loop pairs between two sessions of --n-kf keyframes (os1-64).  The source of
a pair is one keyframe of the query session, the target the keyframes within +-25 of the same index of the central session, both in map coordinates
and voxel-gridded at 0.3 m as the reference's loader does (Session.cpp:18-19); the sessions' pose noise is the misalignment ICP removes.  Timed: the
whole batch in one call, the same pairs one per call, and the numpy restatement (tools/icp_numpy.py) on one thread on a subset, scaled.  Device
times are HIP-event times on the context's stream, median of --steps runs after --warmup.  LTM_ICP_POLL (iterations enqueued between two looks at
the unfinished-pairs counter) is swept over --poll.  Writes one JSON line to --out (default profiles/icp_lot-<pairs>.json) and prints it.

    python tools/bench_icp.py [--pairs 64] [--n-kf 128] [--steps 7] [--warmup 2]"""
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
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-pairs", type=int, default=2)
    ap.add_argument("--cpu-stride", type=int, default=16)
    ap.add_argument("--cpu-iterations", type=int, default=4)
    ap.add_argument("--poll", default="1,2,4,8,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    from tools import icp_numpy as ref
    from tools import synth

    torch.set_num_threads(1)
    dev = "cuda:0"
    ctx = capi.Context(vfov=50.0, hfov=360.0, device=0)
    stream = torch.cuda.ExternalStream(ctx.stream())

    def global_points(sess):
        """every scan point in map coordinates (float), and the keyframe offsets"""
        off = sess["offsets"].numpy().astype(np.int64)
        kf = torch.repeat_interleave(torch.arange(len(off) - 1, device=dev), torch.as_tensor(np.diff(off), device=dev))
        P = torch.as_tensor(np.asarray(sess["poses"]).reshape(-1, 4, 4), device=dev)
        x = sess["scans"][:, :3].double()
        g = torch.einsum("nij,nj->ni", P[kf, :3, :3], x) + P[kf, :3, 3]
        out = sess["scans"].clone()
        out[:, :3] = g.float()
        return out.contiguous(), off

    Cg, Coff = global_points(synth.make_session(1, args.n_kf, "os1-64", device=dev))
    Qg, Qoff = global_points(synth.make_session(2, args.n_kf, "os1-64", device=dev))
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
    out = {"tool": "bench_icp", "workload": f"lot-2x{args.n_kf}-os1-64, {args.pairs} pairs, leaf {args.leaf} m, target +-{args.half_window} keyframes",
           "pairs": args.pairs, "source_points_mean": round(float(np.mean(n_src))), "target_points_mean": round(float(np.mean(n_tgt))),
           "steps": args.steps, "warmup": args.warmup}

    sweep = {}
    for poll in [int(v) for v in args.poll.split(",") if v]:
        os.environ["LTM_ICP_POLL"] = str(poll)
        ev, wall = timed(lambda: res.__setitem__("batch", ctx.icp_align(pairs)))
        sweep[str(poll)] = {"event_ms": round(ev, 3), "wall_ms": round(wall, 3)}
    os.environ.pop("LTM_ICP_POLL", None)
    out["poll_interval_sweep"] = sweep
    ev, wall = timed(lambda: res.__setitem__("batch", ctx.icp_align(pairs)))
    out["batch"] = {"event_ms": round(ev, 3), "wall_ms": round(wall, 3), "ms_per_pair": round(wall / args.pairs, 4)}

    def one_per_call():
        res["single"] = np.concatenate([ctx.icp_align([p]) for p in pairs])
    ev1, wall1 = timed(one_per_call)
    out["one_pair_per_call"] = {"event_ms": round(ev1, 3), "wall_ms": round(wall1, 3), "ms_per_pair": round(wall1 / args.pairs, 4)}
    out["batch_vs_one_per_call"] = round(wall1 / wall, 2)
    out["batch_equals_one_per_call_bytes"] = bool(res["batch"].tobytes() == res["single"].tobytes())
    it = res["batch"]["iterations"]
    out["iterations"] = {"min": int(it.min()), "median": float(np.median(it)), "max": int(it.max()), "converged": int(res["batch"]["converged"].sum())}
    out["states"] = {capi.ICP_STATES[s]: int((res["batch"]["state"] == s).sum()) for s in range(5)}
    out["fitness_median"] = float(np.median(res["batch"]["fitness"]))

    # the numpy restatement on one thread: brute-force neighbours cost source x target per pass, so it runs --cpu-pairs pairs on every
    # --cpu-stride-th source point for --cpu-iterations iterations (checked against the device on the same input) and is scaled by points, passes and pairs
    sub = np.linspace(0, args.pairs - 1, min(args.cpu_pairs, args.pairs)).astype(np.int64)
    agree, worst, scaled = True, 0.0, []
    for k in sub:
        tgt, src = targets[k].download(), sources[k].download()
        part = np.ascontiguousarray(src[::args.cpu_stride])
        t0 = time.perf_counter()
        want = ref.align(tgt, part, max_iterations=args.cpu_iterations)
        dt = time.perf_counter() - t0
        got = ctx.icp_align([(indices[k], part)], max_iterations=args.cpu_iterations)[0]
        agree = agree and (want["iterations"], want["state"], want["n_corr"]) == (int(got["iterations"]), int(got["state"]), int(got["n_corr"]))
        worst = max(worst, float(np.abs(want["T"] - got["T"]).max()))
        scaled.append(dt / (want["iterations"] + 1) * (int(it[k]) + 1) * len(src) / len(part))
    cpu_ms = 1e3 * float(np.mean(scaled)) * args.pairs
    out["numpy_restatement"] = {"threads": 1, "pairs_timed": len(sub), "source_stride": args.cpu_stride, "iterations_run": args.cpu_iterations,
                                "batch_ms_scaled": round(cpu_ms, 1), "iterations_state_n_corr_agree": bool(agree), "max_abs_T_difference": worst}
    out["speedup_vs_numpy_1thread"] = round(cpu_ms / wall, 1)

    for i in indices:
        i.close()
    ctx.close()
    line = json.dumps(out)
    path = args.out or os.path.join(ROOT, "profiles", f"icp_lot-{args.pairs}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
