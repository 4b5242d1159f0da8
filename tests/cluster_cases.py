"""Fixtures of the cluster tests (tests/test_cluster_api_cpu.py, tests/test_unionfind_cpu.py, tests/test_gpu_cluster.py): small clouds at the seams of
ltm_k_cluster.hip -- leaves of 32 points, workgroups of 256, clique leaves, the strict < of the relation, the size filter, the tie rule of the numbering.
Every cloud is given in a permuted order, so that a point's original index is not its sorted position.  A case is (points float32 [n, 4], tolerance,
min_size, max_size or None); reference(name) is its restatement by tools/cluster_numpy.py, computed once."""
import functools

import numpy as np

from tools import cluster_numpy as cref


def _xyzi(xyz, seed):
    """float32 XYZI rows of xyz in a permuted order (the intensity carries the row's number before the permutation)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.concatenate([xyz, np.arange(len(xyz), dtype=np.float32)[:, None]], axis=1)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(len(p))])


def zigzag_chain(n, step, row=50, z=0.0):
    """n points `step` apart along a serpentine path: rows of `row` steps along x, joined by two steps along y (rows 2 * step apart: only the path joins them)"""
    out = np.zeros((n, 3))
    x = y = 0
    dirx = 1
    along = 0      # steps made in the current row / in the current turn
    turning = 0
    for i in range(n):
        out[i] = (x * step, y * step, z)
        if turning:
            y += 1
            turning -= 1
        elif along == row:
            along = 0
            dirx = -dirx
            y += 1
            turning = 1
        else:
            x += dirx
            along += 1
    return out


def _uniform(n, seed):
    """n uniform points in a cube of side n^(1/3): about one point per unit volume, so a tolerance of 0.7 gives components of many sizes"""
    return np.random.default_rng(seed).uniform(0.0, max(n, 1) ** (1.0 / 3.0), (n, 3))


def _blobs(seed, n_blobs=20, noise=500):
    rng = np.random.default_rng(seed)
    parts = []
    for b in range(n_blobs):
        parts.append(rng.uniform(-10.0, 10.0, 3) + rng.normal(0.0, 0.15, (int(rng.integers(20, 400)), 3)))
    parts.append(rng.uniform(-10.0, 10.0, (noise, 3)))
    return np.concatenate(parts)


def _groups(sizes, seed, spread=0.01, pitch=5.0):
    """tight groups of the given sizes, `pitch` apart: components of exactly those sizes at any tolerance between spread and pitch"""
    rng = np.random.default_rng(seed)
    return np.concatenate([np.array([pitch * g, 0.0, 0.0]) + rng.uniform(0.0, spread, (s, 3)) for g, s in enumerate(sizes)])


def _with_nonfinite(xyz, seed, share=0.1):
    rng = np.random.default_rng(seed)
    xyz = np.array(xyz, np.float32)
    rows = rng.choice(len(xyz), int(share * len(xyz)), replace=False)
    xyz[rows, rng.integers(0, 3, len(rows))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(rows))
    return xyz


def _build():
    c = {}
    c["empty"] = (np.zeros((0, 4), np.float32), 0.5, 1, None)
    c["one_point"] = (_xyzi([[1.0, 2.0, 3.0]], 1), 0.5, 1, None)
    c["all_nonfinite"] = (_xyzi(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]] * 10), 2), 0.5, 1, None)
    c["nonfinite_mixed"] = (_xyzi(_with_nonfinite(_blobs(3, 8, 200), 4), 5), 0.3, 3, None)
    # d2 == r2 exactly: 0.5 and 0.25 are floats, 0.5 * 0.5 is exact; the relation is strict, so the two points stay apart ...
    c["boundary_equal"] = (_xyzi([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], 6), 0.5, 1, None)
    # ... and join at the next float below
    c["boundary_below"] = (_xyzi([[0.0, 0.0, 0.0], [np.nextafter(np.float32(0.5), np.float32(0.0)), 0.0, 0.0]], 6), 0.5, 1, None)
    c["chain_5000"] = (_xyzi(zigzag_chain(5000, 0.45), 7), 0.5, 1, None)                                     # spacing 0.9 x tolerance
    c["two_chains"] = (_xyzi(np.concatenate([zigzag_chain(5000, 0.45), zigzag_chain(5000, 0.45, z=0.55)]), 8), 0.5, 1, None)      # 1.1 x tolerance apart
    for n in (31, 32, 33, 255, 256, 257, 1025):
        c[f"uniform_{n}"] = (_xyzi(_uniform(n, 100 + n), 200 + n), 0.7, 1, None)
    c["duplicates"] = (_xyzi(np.concatenate([np.tile([[1.0, 1.0, 1.0]], (1000, 1)), np.tile([[3.0, 1.0, 1.0]], (1000, 1))]), 9), 0.5, 1, None)
    c["blobs"] = (_xyzi(_blobs(10), 11), 0.3, 10, None)
    c["blobs_shifted"] = (_xyzi(_blobs(10) + np.array([3000.0, -2000.0, 100.0]), 11), 0.3, 10, None)
    c["tolerance_above_cloud"] = (_xyzi(np.random.default_rng(12).uniform(0.0, 1.0, (1500, 3)), 13), 10.0, 1, None)
    g = np.arange(12, dtype=np.float64)
    c["tolerance_below_pairs"] = (_xyzi(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3), 14), 0.5, 1, None)      # 1728 = 54 leaves
    c["filter_seams"] = (_xyzi(_groups([4, 5, 9, 10, 7], 15), 16), 0.5, 5, 9)      # min_size - 1, min_size, max_size, max_size + 1, and one inside
    c["equal_sizes"] = (_xyzi(_groups([8, 8, 8, 8, 8, 8, 3, 12], 17), 18), 0.5, 1, None)
    return c


CASES = _build()
SMALL = [k for k, v in CASES.items() if len(v[0]) <= 2000]      # the cases the O(n^2) brute force of the CPU tests runs over


@functools.lru_cache(maxsize=None)
def reference(name):
    pts, tol, lo, hi = CASES[name]
    r = cref.cluster(pts, tol, lo, hi)
    for v in r.values():
        v.setflags(write=False)
    return r
