"""Fixtures of the plane-segmentation tests (tests/test_plane_cases_cpu.py, tests/test_plane_api_cpu.py, tests/test_gpu_plane.py): small records at the seams of
ltm_k_plane.hip -- no plane at all, the strict < of the inlier test, the tie rule, the axis constraint, chunks of 256, the count kernel's workgroup of
plane_block_points() points, hypothesis counts around a wavefront and at the limit.  Every record is given in a permuted order (the intensity carries the
row's number before the permutation).  A case is (points float32 [n, 4], params of tools/plane_numpy.py); reference(name) is its restatement, computed once."""
import functools
import math

import numpy as np

from tools import plane_numpy as pref

BLOCK_POINTS = 2048      # ltm_plane_block_points() / LTM_PLANE_BLOCK_POINTS; tests/test_plane_api_cpu.py checks that the library says the same


def _xyzi(xyz, seed):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.concatenate([xyz, np.arange(len(xyz), dtype=np.float32)[:, None]], axis=1)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(len(p))])


def noisy_plane(n_plane, n_out, seed, shift=(0.0, 0.0, 0.0)):
    """n_plane points of z = 0.25 x + 3 with 2 cm noise over 20 m x 20 m, n_out outliers in the box around it"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-10.0, 10.0, (n_plane, 2))
    pl = np.column_stack([xy, 0.25 * xy[:, 0] + 3.0 + rng.normal(0.0, 0.02, n_plane)])
    out = np.column_stack([rng.uniform(-10.0, 10.0, (n_out, 2)), rng.uniform(-4.0, 10.0, n_out)])
    return np.concatenate([pl, out]) + np.asarray(shift)[None, :]


def wall_and_ground(seed=31):
    """the scene of the issue at 4000 points: 1600 ground points (z = -1.9, 2 cm), a 2000-point wall (x = 8, 2 cm), 400 clutter points"""
    rng = np.random.default_rng(seed)
    ground = np.column_stack([rng.uniform(-15.0, 15.0, (1600, 2)), -1.9 + rng.normal(0.0, 0.02, 1600)])
    wall = np.column_stack([8.0 + rng.normal(0.0, 0.02, 2000), rng.uniform(-12.0, 12.0, 2000), rng.uniform(-1.9, 6.0, 2000)])
    clutter = np.column_stack([rng.uniform(-15.0, 15.0, (400, 2)), rng.uniform(-1.9, 6.0, 400)])
    return np.concatenate([ground, wall, clutter])


def _lattice(nx, ny, z):
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    return np.column_stack([gx.ravel(), gy.ravel(), np.full(gx.size, float(z))])


def _lattice_boundary():
    """the integer lattice of z = 0, one point at z = 0.5 and one a float32 step below, thr = 0.5; the seed is the first under which no hypothesis draws
    one of the two, so that every valid hypothesis has N = (0, 0, +-k) with an integer k and s s = 0.25 k k sits exactly on T for the first point"""
    below = np.nextafter(np.float32(0.5), np.float32(0.0))
    pts = _xyzi(np.concatenate([_lattice(20, 20, 0.0), [[3.0, 4.0, 0.5]], [[11.0, 7.0, float(below)]]]), 17)
    special = set(np.flatnonzero(pts[:, 2] != 0.0).tolist())
    for seed in range(1000):
        p = pref.params(0.5, 64, seed=seed, refine=False)
        h = pref.hypotheses(pts, p)
        if not (set(h["idx"].ravel().tolist()) & special) and h["valid"].sum() >= 32:
            return pts, p
    raise AssertionError("no seed keeps the hypotheses on the lattice")


def _cases():
    nan, inf = float("nan"), float("inf")
    c = {}
    P = pref.params
    c["empty"] = (np.zeros((0, 4), np.float32), P(0.1))
    c["one_point"] = (_xyzi([[1.0, 2.0, 3.0]], 1), P(0.1))
    c["two_points"] = (_xyzi([[1.0, 2.0, 3.0], [2.0, 0.0, 1.0]], 2), P(0.1))
    c["three_points"] = (_xyzi([[1.0, 2.0, 3.0], [2.0, 0.0, 1.0], [-1.0, 1.0, 0.5]], 3), P(0.1))
    c["all_nonfinite"] = (_xyzi([[nan, 0.0, 0.0], [0.0, inf, 1.0], [1.0, 2.0, -inf], [nan, nan, nan], [inf, 1.0, 1.0]] * 20, 4), P(0.1))
    mixed = noisy_plane(1700, 300, 5)
    bad = np.random.default_rng(6).choice(len(mixed), 120, replace=False)
    for k, i in enumerate(bad):
        mixed[i, k % 3] = (nan, inf, -inf)[(k // 3) % 3]
    c["nonfinite_mixed"] = (_xyzi(mixed, 7), P(0.05))
    c["coincident"] = (_xyzi(np.tile([[1.5, -2.25, 0.75]], (500, 1)), 8), P(0.1))
    t = np.arange(500, dtype=np.float64) - 250.0
    c["collinear"] = (_xyzi(np.column_stack([0.25 * t, 0.5 * t, -0.25 * t]) + np.array([1.0, 2.0, 3.0]), 9), P(0.1))
    c["lattice_boundary"] = _lattice_boundary()
    noise = noisy_plane(1000, 200, 10)
    c["plane_noise"] = (_xyzi(noise, 11), P(0.05))
    for it in (1, 63, 64, 65, 4096):
        c[f"plane_noise_it{it}"] = (c["plane_noise"][0], P(0.05, it))
    c["plane_noise_unrefined"] = (c["plane_noise"][0], P(0.05, refine=False))
    c["plane_noise_seed7"] = (c["plane_noise"][0], P(0.05, seed=7))
    c["plane_noise_seed7_unrefined"] = (c["plane_noise"][0], P(0.05, seed=7, refine=False))
    wg = _xyzi(wall_and_ground(), 12)
    c["wall_and_ground"] = (wg, P(0.1))
    c["wall_and_ground_axis"] = (wg, P(0.1, axis=(0.0, 0.0, 1.0), eps_angle=math.radians(10.0)))
    c["equal_support"] = (_xyzi(np.concatenate([_lattice(15, 15, 0.0), _lattice(15, 15, 10.0)]), 13), P(0.25))
    c["far_scene"] = (_xyzi(noisy_plane(1000, 200, 10, shift=(3000.0, -2000.0, 100.0)), 11), P(0.05))
    for n in (255, 256, 257, 1023, 1024, 1025, BLOCK_POINTS - 1, BLOCK_POINTS, BLOCK_POINTS + 1):
        c[f"size_{n}"] = (_xyzi(noisy_plane(n - n // 8, n // 8, 100 + n), 200 + n), P(0.05, 96, seed=n))
    return c


CASES = _cases()
SMALL = [name for name, (pts, _) in CASES.items() if len(pts) <= 2000]


@functools.lru_cache(maxsize=None)
def reference(name):
    pts, p = CASES[name]
    r = pref.segment(pts, p)
    for a in list(r.values()) + list(r["hyps"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r
