"""Fixtures of the ICP tests (tests/test_icp_api_cpu.py checks them on the CPU, tests/test_gpu_icp.py runs them on the device) and the bounds both use.
Every cloud keeps |coordinate| < 16 m (EXTENT), which the derivation of tol_T rests on.  Everything is seeded; the restatement's results are computed
once per process and shared."""
import functools

import numpy as np

from tools import icp_numpy as ref

EXTENT = 16.0


def tol_T(n_source):
    """Largest difference allowed on an entry of T between the device and the restatement.  The two differ only in summation order and SVD route, about
    1e-14 here -- unless such a difference moves one transformed coordinate across a float rounding boundary: one query then moves by one float ulp
    (at most 2^-23 * EXTENT for |coordinate| < EXTENT) and the estimate by about ulp / N.  With N >= 64 source points and a factor 8 for lever arm and
    conditioning this is 2^-23 * 16 / 8 ~ 2.4e-7; the fixtures with fewer points get the same bound scaled by 64 / N."""
    return 2.0 ** -23 * EXTENT * 8.0 / min(max(int(n_source), 1), 64)


def tol_rel(n_source):
    """relative bound on fitness, last_mse and the trace MSEs: a displacement of tol_T against distances of the order of the extent, d2 twice that, and 2
    for the mean's own order"""
    return 4.0 * tol_T(n_source) / EXTENT


def rigid(yaw_deg, t, pitch_deg=0.0):
    a, b = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg)
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[np.cos(b), 0.0, np.sin(b)], [0.0, 1.0, 0.0], [-np.sin(b), 0.0, np.cos(b)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry
    T[:3, 3] = t
    return T


def apply(T, pts):
    return (pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def scene(rng, n):
    """n points on a floor, two walls and a box, 20 m across: every direction is constrained"""
    kind = rng.integers(0, 4, n)
    u, v = rng.uniform(-10.0, 10.0, n), rng.uniform(-10.0, 10.0, n)
    h = rng.uniform(0.0, 3.0, n)
    p = np.empty((n, 3))
    p[kind == 0] = np.stack([u, v, np.zeros(n)], 1)[kind == 0]                       # floor z = 0
    p[kind == 1] = np.stack([u, np.full(n, 10.0), h], 1)[kind == 1]                  # wall y = 10
    p[kind == 2] = np.stack([np.full(n, -10.0), v, h], 1)[kind == 2]                 # wall x = -10
    face = rng.integers(0, 3, n)
    bx = np.stack([np.where(face == 0, 4.0, 2.0 + 2.0 * (u + 10.0) / 20.0), np.where(face == 1, -3.0, -5.0 + 2.0 * (v + 10.0) / 20.0),
                   np.where(face == 2, 1.5, 1.5 * h / 3.0)], 1)                      # a 2 x 2 x 1.5 m box: three of its faces
    p[kind == 3] = bx[kind == 3]
    return p.astype(np.float32)


def scene_pair(seed, n_target, n_source, yaw_deg, t, noise=0.01):
    """target: a scene; source: n_source other points of the same scene with 1 cm of noise, moved by the INVERSE of the ground truth (yaw, t)"""
    rng = np.random.default_rng(seed)
    target = scene(rng, n_target)
    src = scene(rng, n_source).astype(np.float64) + rng.normal(0.0, noise, (n_source, 3))
    source = apply(np.linalg.inv(rigid(yaw_deg, t)), src)
    assert np.abs(target).max() < EXTENT and np.abs(source).max() < EXTENT
    return target, source


# the three scene fixtures (target / source points, ground truth 3-7 degrees of yaw and at most 0.6 m)
SCENES = {"scene_3000_700": (11, 3000, 700, 5.0, (0.4, -0.3, 0.1)),
          "scene_2000_65": (12, 2000, 65, 3.0, (-0.2, 0.5, 0.05)),
          "scene_4000_1000": (13, 4000, 1000, 7.0, (0.3, 0.3, -0.2))}


def outlier_pair():
    """640 source points: 600 inliers (target points with 1 cm of noise, 1.5 degrees and 0.15 m off: always within 1 m of the target) and 40 outliers
    9 m and more above everything (never within 1 m, always within 150 m).  The scene is shrunk to 8 m across so that the outliers at z = 10 .. 15 m stay
    inside |coordinate| < 16."""
    rng = np.random.default_rng(21)
    target = (scene(rng, 2000) * np.float32(0.4)).astype(np.float32)
    pick = rng.choice(len(target), 600, replace=False)
    inl = target[pick].astype(np.float64) + rng.normal(0.0, 0.01, (600, 3))
    out = np.stack([rng.uniform(-4.0, 4.0, 40), rng.uniform(-4.0, 4.0, 40), rng.uniform(10.0, 15.0, 40)], 1)
    src = np.concatenate([inl, out])[rng.permutation(640)]
    source = apply(np.linalg.inv(rigid(1.5, (0.1, -0.1, 0.05))), src)
    assert np.abs(target).max() < EXTENT and np.abs(source).max() < EXTENT
    return target, source


def edge_pairs():
    """tree and block edges: target sizes 4, 31, 32, 33, 1025 (random, not coplanar), source sizes 3, 63, 64, 65, 255, 256, 257 and one source with a few
    NaN / inf points.  A source point is a target point (taken round robin, distinct while they last) with 1 cm of noise, the whole moved by a small
    transform, so the correspondences span three dimensions (a plane for the three-point source)."""
    rng = np.random.default_rng(31)
    out = []
    for k, (nt, ns, bad) in enumerate(((4, 3, 0), (31, 63, 0), (32, 64, 0), (33, 65, 0), (1025, 255, 0), (1025, 256, 0), (1025, 257, 0), (33, 257, 5))):
        target = rng.uniform(-8.0, 8.0, (nt, 3)).astype(np.float32)
        src = target[np.arange(ns) % nt].astype(np.float64) + rng.normal(0.0, 0.01, (ns, 3))
        source = apply(np.linalg.inv(rigid(2.0 + 0.3 * k, (0.05, -0.04, 0.03), pitch_deg=1.0)), src)
        if bad:
            source = np.concatenate([source, source[:bad]])
            at = rng.choice(len(source), bad, replace=False)
            source[at, rng.integers(0, 3, bad)] = np.array([np.nan, np.inf, -np.inf, np.nan, np.inf], np.float32)[:bad]
        assert np.abs(target).max() < EXTENT and np.nanmax(np.abs(np.where(np.isfinite(source), source, 0.0))) < EXTENT
        out.append((target, source))
    return out


def lattice_pair(offset=(0.0, 0.0, 0.0)):
    """the known answer: the 6 x 5 x 4 unit lattice and every third point of it shifted by (-0.25, 0, 0); both moved by `offset`"""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    target = g + np.asarray(offset, np.float32)
    source = target[::3] + np.float32((-0.25, 0.0, 0.0))
    return target, source


FAR = (1000.125, -2000.5, 0.0)


def check_known_answer(r, bound):
    """r: anything with T, iterations, state, n_corr, fitness by name (the restatement's dict or a device record)"""
    want = np.eye(4)
    want[0, 3] = 0.25
    assert int(r["iterations"]) == 2 and int(r["state"]) == 2 and int(r["n_corr"]) == 40, (r["iterations"], r["state"], r["n_corr"])
    err = np.abs(np.asarray(r["T"]) - want).max()
    assert err <= bound, err
    assert float(r["fitness"]) < 1e-24, r["fitness"]


@functools.lru_cache(maxsize=None)
def scene_fixture(name):
    """(target, source, the restatement's result) of a scene fixture"""
    target, source = scene_pair(*SCENES[name])
    return target, source, ref.align(target, source)


@functools.lru_cache(maxsize=None)
def outlier_fixture(max_corr_dist):
    target, source = outlier_pair()
    return target, source, ref.align(target, source, max_corr_dist=max_corr_dist)


@functools.lru_cache(maxsize=None)
def edge_fixtures():
    return tuple((t, s, ref.align(t, s)) for t, s in edge_pairs())


# Started again from its own answer, the restatement has nothing left to do on these (at most 2 iterations).  scene_3000_700 is not among them: a stop by
# the transform test (a step under 1 mm) is not a fixed point, its next step regroups a few correspondences and takes three more iterations to settle;
# there the device only has to do what the restatement does.
RESTART_QUIET = ("scene_2000_65", "scene_4000_1000")


@functools.lru_cache(maxsize=None)
def restart_fixture(name):
    """the restatement's result on a scene fixture when it starts from its own final transform"""
    target, source, first = scene_fixture(name)
    return ref.align(target, source, init=first["T"])
