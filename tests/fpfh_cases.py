"""Fixtures of the FPFH tests (tests/test_fpfh_cases_cpu.py, tests/test_gpu_fpfh.py): small clouds at the seams of ltm_k_fpfh.hip -- nothing to describe at
all, fewer points than the neighbourhood, every list form (4 / 8 / 16 registers, LDS) full and one past it, pairs that are skipped (coincident points,
duplicates, normals along the line of sight), exact geometry (a lattice plane, a sphere seen from its centre, two planes meeting at an edge), coordinates far
from the origin, one workgroup short / full / one over.  Every cloud is given in a permuted order (the intensity carries the row's number before the
permutation).  CASES[name] = dict(points float32 [n, 4], k, normal: None (the normals are estimated at NORMALS_K, viewpoint at the origin) or one (nx, ny, nz)
that every point gets)."""
import numpy as np

from outlier_cases import FAR, _with_non_finite, _xyzi, blob, noisy_plane

NORMALS_K = 10
KS = (2, 3, 4, 5, 8, 9, 16, 17, 33, 64)      # 4 / 8 / 16 register slots full and one past each, two LDS sizes, the limits


def lattice_plane(n=12):
    """n x n points of z = 0 at integer x, y"""
    g = np.arange(n, dtype=np.float64)
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.column_stack([x.ravel(), y.ravel(), np.zeros(n * n)])


def lattice_interior(xyz, margin):
    """rows of a lattice_plane at least `margin` from its border"""
    n = xyz[:, :2].max() + 1
    return ((xyz[:, :2] >= margin) & (xyz[:, :2] <= n - 1 - margin)).all(axis=1)


def sphere_shell(n=600, radius=5.0, seed=41):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return radius * v / np.sqrt((v * v).sum(axis=1))[:, None]


def edge_scene(n=21, step=0.1):
    """two planes meeting at the edge x = 0, z = 0: z = 0 for x <= 0 and x = 0 for z >= 0, n x n points each with spacing `step` (the edge's points once per
    plane, a tenth of a step apart so that none coincide); returns (xyz, hand normals towards +z / -x, distance from the edge)"""
    g = np.arange(n, dtype=np.float64) * step
    a, y = np.meshgrid(g, g, indexing="ij")
    a, y = a.ravel(), y.ravel()
    floor = np.column_stack([-a - 0.1 * step, y, np.zeros(len(a))])
    wall = np.column_stack([np.zeros(len(a)), y, a + 0.1 * step])
    normals = np.concatenate([np.tile([[0.0, 0.0, 1.0]], (len(a), 1)), np.tile([[-1.0, 0.0, 0.0]], (len(a), 1))])
    return np.concatenate([floor, wall]), normals, np.concatenate([a, a])


def duplicated_scene(seed=17):
    """a noisy plane of 200 points of which 40 are there twice"""
    xyz = noisy_plane(200, 0, seed)
    return np.concatenate([xyz, xyz[np.random.default_rng(seed).choice(200, 40, replace=False)]])


def line(n=40):
    return np.column_stack([0.25 * np.arange(n), np.full(n, 1.0), np.full(n, -2.0)])


def _cases():
    nan, inf = float("nan"), float("inf")
    c = {}

    def add(name, xyz, k, seed, normal=None):
        pts = np.zeros((0, 4), np.float32) if len(xyz) == 0 else _xyzi(xyz, seed)
        c[name] = dict(points=pts, k=k, normal=normal)

    add("empty", [], 8, 0)
    add("one_point", [[1.0, 2.0, 3.0]], 8, 1)
    add("two_points", [[1.0, 2.0, 3.0], [1.5, 2.0, 3.0]], 8, 2)
    add("two_points_hand_normal", [[1.0, 2.0, 3.0], [1.5, 2.25, 3.0]], 8, 2, normal=(0.0, 0.0, 1.0))
    add("two_finite_among_non_finite", [[nan, 0.0, 0.0], [1.0, 2.0, 3.0], [0.0, inf, 0.0], [1.5, 2.0, 3.5], [0.0, 0.0, -inf]], 8, 3, normal=(0.0, 0.6, 0.8))
    add("all_non_finite", [[nan, 0.0, 0.0], [0.0, inf, 0.0], [0.0, 0.0, -inf], [nan, nan, nan]], 4, 3)
    add("non_finite_mixed", _with_non_finite(noisy_plane(285, 15, 6), 0), 10, 4)
    for k in (8, 20):      # register and LDS lists with fewer points than slots, exactly as many, one more
        for n in (k - 1, k, k + 1):
            add(f"k{k}_n{n}", blob(n, 10 + k + n), k, 5)
    for k in KS:
        add(f"blob_k{k}", blob(300, 20), k, 6)
    add("coincident_500", np.tile([[2.0, -1.0, 0.5]], (500, 1)), 8, 7, normal=(0.0, 0.0, 1.0))
    add("duplicates", duplicated_scene(), 10, 8)
    add("line_normals_along", line(), 6, 9, normal=(1.0, 0.0, 0.0))
    add("lattice_plane", lattice_plane(), 9, 10)
    add("lattice_plane_hand_normal", lattice_plane(), 9, 10, normal=(0.0, 0.0, 1.0))
    add("sphere_shell", sphere_shell(), 10, 11)
    add("edge", edge_scene()[0], 12, 12)
    add("plane", noisy_plane(), 10, 9)
    add("plane_k32", noisy_plane(), 32, 9)
    add("plane_far", noisy_plane(shift=FAR), 10, 9)
    for n in (255, 256, 257):
        add(f"n{n}", blob(n, 30 + n % 7), 10, 10)
    return c


CASES = _cases()
ALL = list(CASES)
BATCH = ("empty", "one_point", "edge", "blob_k8")      # one call over all four (each index at its own normals, one k)
