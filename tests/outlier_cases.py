"""Fixtures of the outlier-filter tests (tests/test_outlier_cases_cpu.py, tests/test_outlier_api_cpu.py, tests/test_gpu_outlier.py): small clouds at the seams
of ltm_k_outlier.hip -- nothing to filter at all, fewer points than the neighbourhood, every list form (4 / 8 / 16 registers, LDS), the variance clamp, the
chunk and group boundaries of the record sums, the strict < of the radius relation, counts beyond one leaf.  Every cloud is given in a permuted order (the
intensity carries the row's number before the permutation).  SOR[name] = (points float32 [n, 4], mean_k, stddev_mul); ROR[name] = (points, radius,
min_neighbors); reference(kind, name) is the case's restatement (tools/outlier_numpy.py), computed once.  SCENES names the cases that are scenes a user would
filter: there the filter must remove something and keep most."""
import functools

import numpy as np

from tools import outlier_numpy as oref


def _xyzi(xyz, seed):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.concatenate([xyz, np.arange(len(xyz), dtype=np.float32)[:, None]], axis=1)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(len(p))])


def noisy_plane(n_plane=600, n_out=30, seed=5, shift=(0.0, 0.0, 0.0)):
    """n_plane points of z = 0.1 x + 1 with 2 cm noise over 10 m x 10 m, n_out sparse outliers 0.5 .. 6 m above it"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-5.0, 5.0, (n_plane, 2))
    pl = np.column_stack([xy, 0.1 * xy[:, 0] + 1.0 + rng.normal(0.0, 0.02, n_plane)])
    oxy = rng.uniform(-5.0, 5.0, (n_out, 2))
    out = np.column_stack([oxy, 0.1 * oxy[:, 0] + 1.0 + rng.uniform(0.5, 6.0, n_out)])
    return np.concatenate([pl, out]) + np.asarray(shift)[None, :]


def blob(n, seed, side=4.0):
    """n points uniform in a cube"""
    return np.random.default_rng(seed).uniform(0.0, side, (n, 3))


def clamp_pairs():
    """50 pairs, pair i at (10 i, 0, 0) and (10 i, 0.7f, 0): with mean_k = 1 all 100 distances are the same float and the variance's rounding residue is
    negative"""
    i = np.arange(50, dtype=np.float64)
    a = np.column_stack([10.0 * i, np.zeros(50), np.zeros(50)])
    b = np.column_stack([10.0 * i, np.full(50, float(np.float32(0.7))), np.zeros(50)])
    return np.concatenate([a, b])


def lattice(n=6):
    g = np.arange(n, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def _with_non_finite(xyz, seed):
    """every 7th row loses a coordinate to NaN, +inf or -inf in turn"""
    xyz = np.array(xyz, np.float64)
    bad = [float("nan"), float("inf"), float("-inf")]
    for k, row in enumerate(range(3, len(xyz), 7)):
        xyz[row, (k + seed) % 3] = bad[k % 3]
    return xyz


FAR = (3000.0, -2000.0, 100.0)
MEAN_KS = (1, 3, 4, 7, 8, 15, 16, 50, 63)      # 4 / 8 / 16 register slots full, the first LDS size, PCL's tutorial setting, the limit


def _sor_cases():
    nan = float("nan")
    c = {}
    c["empty"] = (np.zeros((0, 4), np.float32), 8, 1.0)
    c["one_point"] = (_xyzi([[1.0, 2.0, 3.0]], 1), 8, 1.0)
    c["two_points"] = (_xyzi([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0]], 2), 8, 1.0)
    c["two_points_k1"] = (_xyzi([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0]], 2), 1, -0.5)
    c["all_non_finite"] = (_xyzi([[nan, 0.0, 0.0], [0.0, float("inf"), 0.0], [0.0, 0.0, float("-inf")], [nan, nan, nan]], 3), 4, 1.0)
    c["non_finite_mixed"] = (_xyzi(_with_non_finite(noisy_plane(300, 15, 6), 0), 4), 8, 1.0)
    for mk in (8, 20):      # register and LDS lists with fewer points than slots, exactly as many, one more
        for extra in (0, 1, 2):
            c[f"k{mk}_n{mk + extra}"] = (_xyzi(blob(mk + extra, 10 + mk + extra), 5), mk, 1.0)
    for mk in MEAN_KS:
        c[f"blob_k{mk}"] = (_xyzi(blob(300, 20), 6), mk, 1.0)
    c["coincident_500"] = (_xyzi(np.tile([[2.0, -1.0, 0.5]], (500, 1)), 7), 8, 1.0)
    c["clamp"] = (_xyzi(clamp_pairs(), 8), 1, 1.0)
    c["plane"] = (_xyzi(noisy_plane(), 9), 8, 1.0)
    c["plane_k50"] = (_xyzi(noisy_plane(), 9), 50, 1.0)
    c["plane_negative_mul"] = (_xyzi(noisy_plane(), 9), 8, -0.25)      # a threshold below the mean, as PCL allows: no scene, most points go
    c["plane_far"] = (_xyzi(noisy_plane(shift=FAR), 9), 8, 1.0)
    for n in (255, 256, 257, 16383, 16384, 16385):      # one chunk short / full / one over; one group of 64 chunks short / full / one over
        c[f"n{n}"] = (_xyzi(blob(n, 30 + n % 7, side=4.0 if n < 1000 else 16.0), 10), 4, 1.0)
    c["n16385_k20"] = (_xyzi(blob(16385, 33, side=16.0), 11), 20, 2.0)
    return c


def _ror_cases():
    nan = float("nan")
    c = {}
    c["empty"] = (np.zeros((0, 4), np.float32), 0.5, 2)
    c["one_point"] = (_xyzi([[1.0, 2.0, 3.0]], 1), 0.5, 1)
    c["one_point_needs_two"] = (_xyzi([[1.0, 2.0, 3.0]], 1), 0.5, 2)
    c["two_points"] = (_xyzi([[1.0, 2.0, 3.0], [1.25, 2.0, 3.0]], 2), 0.5, 2)
    c["all_non_finite"] = (_xyzi([[nan, 0.0, 0.0], [0.0, float("inf"), 0.0], [0.0, 0.0, float("-inf")]], 3), 0.5, 1)
    c["non_finite_mixed"] = (_xyzi(_with_non_finite(noisy_plane(300, 15, 6), 1), 4), 0.8, 3)
    c["coincident_500"] = (_xyzi(np.tile([[2.0, -1.0, 0.5]], (500, 1)), 7), 0.01, 500)
    # the integer lattice: at radius 1 the six neighbours at d2 == r2 are out (strict <), at the next float above they are in
    c["lattice_r1"] = (_xyzi(lattice(), 12), 1.0, 7)
    c["lattice_r1_next"] = (_xyzi(lattice(), 12), float(np.nextafter(np.float32(1.0), np.float32(2.0))), 7)
    c["plane_min1"] = (_xyzi(noisy_plane(), 9), 0.4, 1)           # every finite point has itself
    c["plane_min2"] = (_xyzi(noisy_plane(), 9), 0.4, 2)
    c["plane_min33"] = (_xyzi(noisy_plane(), 9), 2.0, 33)         # beyond one leaf of 32 points
    c["plane_min_over_n"] = (_xyzi(noisy_plane(), 9), 2.0, 631)   # more than there are points: all removed
    c["plane_far_min2"] = (_xyzi(noisy_plane(shift=FAR), 9), 0.4, 2)
    for n in (255, 256, 257):
        c[f"n{n}"] = (_xyzi(blob(n, 30 + n % 7), 10), 0.6, 4)
    c["n16385"] = (_xyzi(blob(16385, 33, side=16.0), 11), 0.7, 5)
    return c


SOR = _sor_cases()
ROR = _ror_cases()
SCENES = (("sor", "plane"), ("sor", "plane_k50"), ("sor", "plane_far"), ("sor", "non_finite_mixed"),
          ("ror", "plane_min2"), ("ror", "plane_min33"), ("ror", "plane_far_min2"), ("ror", "non_finite_mixed"))
ALL = [("sor", n) for n in SOR] + [("ror", n) for n in ROR]


def case(kind, name):
    return (SOR if kind == "sor" else ROR)[name]


@functools.lru_cache(maxsize=None)
def reference(kind, name):
    pts, a, b = case(kind, name)
    return oref.statistical(pts, a, b) if kind == "sor" else oref.radius(pts, a, b)
