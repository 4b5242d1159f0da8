"""FPFH matches and the sample-consensus start on the device (ltm_fpfh_match, ltm_sac_align) on the 64-pair lot of tools/bench_icp.py: the source of a pair
is one keyframe of the query session, the target the keyframes within +-25 of the same index of the central session, both in map coordinates and
voxel-gridded at 0.3 m.  Normals (k = 10) and FPFH rows (--fpfh-k) of all targets and sources are made once, outside the timed regions.  Timed, wall clock
around calls that end in a device synchronise, median [min - max] of --steps runs after --warmup, the forms alternating inside every round:
  matches    all pairs in one call; one call per pair; torch.cdist + topk over Fpfh.device_view() on --cdist-pairs pairs, source rows in chunks (the
             distance matrix of a whole pair does not fit), scaled to all pairs: a time baseline only, its sums are not in the stated order
  alignment  max_iterations 1000 at eval_stride 1 and 4: all pairs in one call; one call per pair (each over its own match handle, made before)
Also: the share of hypotheses prerejected, and how many pairs ICP (ltm_icp_align, the reference's parameters, fitness <= 0.5) accepts started from T
against started from identity.  Writes one JSON line to --out (default profiles/sac_lot-<pairs>.json) and prints it.

    python tools/bench_sac.py [--pairs 64] [--n-kf 128] [--steps 3] [--warmup 1]"""
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fpfh-k", type=int, default=16)
    ap.add_argument("--kc", type=int, default=4)
    ap.add_argument("--max-iterations", type=int, default=1000)
    ap.add_argument("--inlier-distance", type=float, default=0.5)
    ap.add_argument("--cdist-pairs", type=int, default=4)
    ap.add_argument("--cdist-chunk", type=int, default=2048)
    ap.add_argument("--fitness-threshold", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    from tools import synth

    torch.set_num_threads(1)
    dev = "cuda:0"
    ctx = capi.Context(vfov=50.0, hfov=360.0, device=0)

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

    n = args.pairs
    kfs = np.linspace(0, args.n_kf - 1, n).astype(np.int64)
    sources = [gridded(Qg, Qoff, int(k), int(k) + 1) for k in kfs]
    targets = [gridded(Cg, Coff, max(int(k) - args.half_window, 0), min(int(k) + args.half_window + 1, args.n_kf)) for k in kfs]
    tidx = [ctx.search_index(t) for t in targets]
    sidx = [ctx.search_index(s) for s in sources]
    ctx.estimate_normals(tidx + sidx, 10)
    rows = ctx.fpfh(tidx + sidx, args.fpfh_k)      # records 0 .. n - 1 the targets, n .. 2 n - 1 the sources
    rec = [(i, n + i) for i in range(n)]
    index_pairs = list(zip(tidx, sidx))
    ctx.synchronize()

    def rounds(forms):
        """forms: name -> callable; every round runs each once, in order; name -> [median, min, max] wall ms"""
        samples = {k: [] for k in forms}
        for r in range(args.warmup + args.steps):
            for name, fn in forms.items():
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                if r >= args.warmup:
                    samples[name].append(1e3 * (time.perf_counter() - t0))
        return {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in samples.items()}

    n_src, n_tgt = [len(s) for s in sources], [len(t) for t in targets]
    work = float(sum(a * b for a, b in zip(n_src, n_tgt)))
    out = {"tool": "bench_sac", "workload": f"lot-2x{args.n_kf}-os1-64, {n} pairs, leaf {args.leaf} m, target +-{args.half_window} keyframes",
           "pairs": n, "source_points_mean": round(float(np.mean(n_src))), "target_points_mean": round(float(np.mean(n_tgt))),
           "fpfh_k": args.fpfh_k, "kc": args.kc, "steps": args.steps, "warmup": args.warmup, "timing": "wall ms, [median, min, max]"}

    # ---- matches
    keep = {}

    def match_batch():
        keep["batch"] = ctx.fpfh_match(rows, rows, rec, args.kc)

    def match_single():
        for h in keep.pop("single", []):
            h.close()
        keep["single"] = [ctx.fpfh_match(rows, rows, [r], args.kc) for r in rec]

    view = rows.device_view()
    off = rows.offsets().astype(np.int64)
    sub = np.linspace(0, n - 1, min(args.cdist_pairs, n)).astype(np.int64)
    sub_work = float(sum(n_src[i] * n_tgt[i] for i in sub))

    def match_torch():
        got = []
        for i in sub:
            t = view[off[i]:off[i + 1]]
            s = view[off[n + i]:off[n + i + 1]]
            for a in range(0, len(s), args.cdist_chunk):
                d = torch.cdist(s[a:a + args.cdist_chunk], t)
                got.append(torch.topk(d, min(args.kc, len(t)), dim=1, largest=False))
        torch.cuda.synchronize()
        keep["torch"] = got

    def match_batch_timed():
        old = keep.pop("batch", None)
        if old is not None:
            old.close()
        match_batch()

    m = rounds({"batch": match_batch_timed, "one_pair_per_call": match_single, "torch_cdist_topk_subset": match_torch})
    keep.pop("torch", None)
    batch = keep["batch"]
    bi, bd = batch.indices(), batch.distances()
    si = np.concatenate([h.indices() for h in keep["single"]])
    sd = np.concatenate([h.distances() for h in keep["single"]])
    torch_scaled = m["torch_cdist_topk_subset"][0] * work / sub_work
    out["match"] = {"row_pairs": work, "batch_ms": m["batch"], "one_pair_per_call_ms": m["one_pair_per_call"],
                    "torch_cdist_topk_ms_on_subset": m["torch_cdist_topk_subset"], "torch_pairs_timed": int(len(sub)),
                    "torch_cdist_topk_ms_scaled_to_all_pairs": round(torch_scaled, 1),
                    "batch_vs_one_per_call": round(m["one_pair_per_call"][0] / m["batch"][0], 3), "batch_vs_torch": round(torch_scaled / m["batch"][0], 3),
                    "row_pairs_per_s": round(work / (1e-3 * m["batch"][0])), "multiply_adds_per_s": round(33.0 * work / (1e-3 * m["batch"][0])),
                    "batch_equals_one_per_call_bytes": bool(bi.tobytes() == si.tobytes() and bd.tobytes() == sd.tobytes())}

    # ---- alignment
    singles = keep["single"]
    out["align"] = {}
    for stride in (1, 4):
        params = dict(inlier_distance=args.inlier_distance, max_iterations=args.max_iterations, eval_stride=stride)
        got = {}

        def sac_batch():
            old = got.pop("batch", None)
            if old is not None:
                old.close()
            got["batch"] = ctx.sac_align(index_pairs, batch, **params)

        def sac_single():
            for h in got.pop("single", []):
                h.close()
            got["single"] = [ctx.sac_align([index_pairs[i]], singles[i], **params) for i in range(n)]

        a = rounds({"batch": sac_batch, "one_pair_per_call": sac_single})
        b = got["batch"]
        same = bool(b.T.tobytes() == np.concatenate([h.T for h in got["single"]]).tobytes()
                    and b.hypothesis_counts().tobytes() == np.concatenate([h.hypothesis_counts() for h in got["single"]]).tobytes())
        found, T = b.found.astype(bool), b.T
        init = np.where(found[:, None, None], T, np.eye(4)[None])
        icp_pairs = list(zip(tidx, sources))
        from_T = ctx.icp_align(icp_pairs, init=init)
        from_identity = ctx.icp_align(icp_pairs)

        def accepted(r):
            return int(((r["converged"] != 0) & (r["fitness"] <= args.fitness_threshold)).sum())

        out["align"][f"eval_stride_{stride}"] = {
            "batch_ms": a["batch"], "one_pair_per_call_ms": a["one_pair_per_call"], "batch_vs_one_per_call": round(a["one_pair_per_call"][0] / a["batch"][0], 3),
            "batch_equals_one_per_call_bytes": same, "voting_points_mean": round(float(b.n_eval.mean())),
            "prerejected_share": round(float(b.n_prerejected.sum()) / float(n * args.max_iterations), 4),
            "valid_share": round(float(b.n_valid.sum()) / float(n * args.max_iterations), 4), "found": int(found.sum()),
            "consensus_share_median": round(float(np.median(b.consensus / np.maximum(b.n_eval, 1))), 4),
            "icp_accepts_from_T": accepted(from_T), "icp_accepts_from_identity": accepted(from_identity)}
        for h in got["single"] + [b]:
            h.close()
    out["sac_params"] = dict(max_iterations=args.max_iterations, inlier_distance=args.inlier_distance, similarity_threshold=0.9, inlier_fraction=0.25, seed=0)
    out["counters_last_call"] = ctx.sac_stats()

    for h in singles + [batch, rows] + tidx + sidx:
        h.close()
    ctx.close()
    line = json.dumps(out)
    path = args.out or os.path.join(ROOT, "profiles", f"sac_lot-{n}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
