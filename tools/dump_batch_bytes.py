"""One SHA-256 per output of the batched entry points on one fixed scene set, for comparing two builds of libltm_hip.so byte for byte: the batched index
build (kNN and radius answers on a fixed query set), normals, the three forms of ICP with trace, clusters (labels, offsets, indices and the per-cluster
tables) and loop submaps.  Run it once per library, each in a fresh process, and compare the listings:

    python tools/dump_batch_bytes.py --lib PATH"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [1023, 0, 1024, 2049, 257, 33, 5000]      # keyframes of the scene set: chunk and block edges, an empty one


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def scene(rng, n):
    """n points on a floor and two walls, 16 m across, with 2 cm of noise: surfaces for the normals, structure for ICP and clusters"""
    kind = rng.integers(0, 3, n)
    u, v, h = rng.uniform(-8.0, 8.0, n), rng.uniform(-8.0, 8.0, n), rng.uniform(0.0, 3.0, n)
    p = np.where((kind == 0)[:, None], np.stack([u, v, np.zeros(n)], 1), np.where((kind == 1)[:, None], np.stack([u, np.full(n, 8.0), h], 1),
                                                                                 np.stack([np.full(n, -8.0), v, h], 1)))
    return (p + rng.normal(0.0, 0.02, (n, 3))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the libltm_hip.so to run")
    args = ap.parse_args()
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    # load_library(path) declares the entry points of that file but keeps it to itself; Context() asks load_library() for the module's library, so
    # that is set here: every Context of this process runs --lib
    capi._lib = capi.load_library(os.path.abspath(args.lib))
    ctx = capi.Context(vfov=50.0, hfov=360.0, device=0)
    rng = np.random.default_rng(5)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
    pts = np.concatenate([scene(rng, int(off[-1])), np.zeros((int(off[-1]), 1), np.float32)], axis=1)
    pts[int(off[3]) + 2048, 2] = np.inf
    pts[int(off[6]) + 7, 1] = np.nan
    queries = np.concatenate([rng.uniform(-9.0, 9.0, (510, 3)), [[np.nan, 0.0, 0.0]], [[100.0, 100.0, 100.0]]]).astype(np.float32)
    qc = ctx.upload(np.concatenate([queries, np.zeros((len(queries), 1), np.float32)], axis=1))
    scans = ctx.upload_scans(pts, off)
    out = []

    batch = ctx.search_index_batch(scans)
    for kf, b in enumerate(batch):
        out.append((f"build kf{kf} info", sha(np.asarray(b.info(), np.int64))))
        for k in (1, 8, 20):
            out.append((f"build kf{kf} knn k{k}", sha(*b.knn(qc, k))))
        for max_nn in (0, 5):
            out.append((f"build kf{kf} radius max_nn {max_nn}", sha(*b.radius(qc, 1.5, max_nn))))

    for k in (10, 20):      # lists in registers, lists in LDS
        ctx.estimate_normals(batch, k, viewpoints=np.tile(np.float32([0.0, 0.0, 10.0]), (len(batch), 1)))
        for kf, b in enumerate(batch):
            out.append((f"normals k{k} kf{kf}", sha(b.normals())))

    # ICP: the big keyframe as target, the others moved a little as sources (clouds for point and plane, indices for generalized)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(0.03), -np.sin(0.03), 0.0], [np.sin(0.03), np.cos(0.03), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = (0.05, -0.04, 0.03)
    moved = pts.copy()
    moved[:, :3] = (pts[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    mscans = ctx.upload_scans(moved, off)
    mbatch = ctx.search_index_batch(mscans)
    ctx.estimate_normals(mbatch, 20)
    src_kf = [0, 1, 2, 3, 4, 5]
    for method in ("point", "plane"):
        res, tr = ctx.icp_align([(batch[6], (mscans, k)) for k in src_kf], trace=True, method=method, max_iterations=30)
        out.append((f"icp {method} results", sha(res)))
        out.append((f"icp {method} trace", sha(tr)))
    res, tr = ctx.icp_align([(batch[6], mbatch[k]) for k in src_kf], trace=True, method="gicp", max_iterations=30)
    out.append(("icp gicp results", sha(res)))
    out.append(("icp gicp trace", sha(tr)))

    clusters = ctx.cluster(batch + [batch[3]], 0.35, min_size=3, max_size=1500)
    for i, cl in enumerate(clusters):
        offs, idx = cl.indices()
        out.append((f"clusters {i} info", sha(np.asarray(cl.info(), np.int64))))
        out.append((f"clusters {i} labels", sha(cl.labels())))
        out.append((f"clusters {i} offsets", sha(offs)))
        out.append((f"clusters {i} indices", sha(idx)))
        out.append((f"clusters {i} tables", sha(cl.sizes, cl.first_index, cl.boxes, cl.centroids)))
        cl.close()

    p6 = np.concatenate([rng.uniform(-30.0, 30.0, (len(SIZES), 3)), rng.uniform(-np.pi, np.pi, (len(SIZES), 3))], axis=1).astype(np.float32)
    aff = capi.pose6d_to_affine3f(p6)
    for name, a, leaf in (("local", None, 0.0), ("central", aff, 0.0), ("central gridded", aff, 0.3)):
        sub = ctx.loop_submaps(scans, [-3, 0, 3, 6, 100], 2, leaf=leaf, affines=a, order="input")
        got = sub.download()[0]
        fin = np.isfinite(got[:, :3]).all(axis=1)      # (the bits of a NaN the device makes are not part of the interface: listed both ways)
        out.append((f"submaps {name} offsets", sha(sub.offsets())))
        out.append((f"submaps {name} raw bytes", sha(got)))
        out.append((f"submaps {name} finite mask", sha(fin)))
        out.append((f"submaps {name} finite points", sha(got[fin])))
        sub.free()

    for name, digest in out:
        print(f"{digest}  {name}")
    for b in batch + mbatch:
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
