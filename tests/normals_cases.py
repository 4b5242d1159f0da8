"""Fixtures of the normals and point-to-plane ICP tests (tests/test_normals_cases_cpu.py and tests/test_icp_plane_api_cpu.py check them on the CPU,
tests/test_gpu_normals.py and tests/test_gpu_icp_plane.py run them on the device).  The clouds are those of tests/icp_fixtures.py (|coordinate| < 16 m)
plus a sphere; everything is seeded, and the restatements' results (tools/normals_numpy.py, tools/icp_plane_numpy.py) are computed once per process and
shared, read-only."""
import functools

import numpy as np

import icp_fixtures as fx
from tools import icp_plane_numpy as plane_ref
from tools import normals_numpy as nref

WELL_POSED_GAP = 1e-3      # (l1 - l0) / l2 of the restatement: below it the direction is left out of the comparison
MAX_ILL_POSED = 0.02       # share of such points a normals fixture may have
ICP_NORMAL_K = 10          # neighbours of the normals the ICP fixtures use
SCENE_VIEWPOINT = (1.0, -2.0, 1.7)


def sphere(n=1000, radius=5.0, seed=51):
    """n points on a sphere.  Of uniformly random points about 6 % have their two nearest neighbours nearly in line with themselves, which leaves the
    normal at k = 3 undetermined; such points (gap below 4 WELL_POSED_GAP in the restatement at k = 3) are drawn again until none is left, so the fixture
    meets the condition at k = 3 with a margin and the larger neighbourhoods are well-posed anyway."""
    rng = np.random.default_rng(seed)

    def draw(m):
        v = rng.normal(size=(m, 3))
        return (radius * v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)

    pts = draw(n)
    for _ in range(50):
        bad = np.flatnonzero(nref.estimate(pts, 3)["gap"] < 4.0 * WELL_POSED_GAP)
        if not len(bad):
            return pts
        pts[bad] = draw(len(bad))
    raise AssertionError("the sphere fixture did not settle")


# name -> (cloud, k, viewpoint): the scene targets at k = 10 and 20, the sphere on both sides of the register / LDS split
@functools.lru_cache(maxsize=None)
def _sphere():
    return sphere()


@functools.lru_cache(maxsize=None)
def normals_fixture(name):
    """(cloud, k, viewpoint, the restatement's result)"""
    if name.startswith("sphere_k"):
        cloud, k, vp = _sphere(), int(name[len("sphere_k"):]), (0.0, 0.0, 0.0)
    else:
        scene, k = name.rsplit("_k", 1)
        cloud, k, vp = fx.scene_pair(*fx.SCENES[scene])[0], int(k), SCENE_VIEWPOINT
    r = nref.estimate(cloud, k, vp)
    for a in r.values():
        a.setflags(write=False)
    return cloud, k, vp, r


NORMALS_FIXTURES = tuple(f"{s}_k{k}" for s in fx.SCENES for k in (10, 20)) + tuple(f"sphere_k{k}" for k in (3, 16, 17, 64))


def well_posed(r):
    """mask of the points whose direction is compared"""
    return np.isfinite(r["gap"]) & (r["gap"] >= WELL_POSED_GAP)


# the comparison of tests/test_gpu_normals.py (its header derives the bounds), shared by every test that holds device normals against the restatement
ULP = 2.0 ** -23


def compare(got, r, what, reach=None):
    """device normals (n, 4) against a restatement result on the well-posed points; curvature on every point.  reach: |viewpoint - point| per point (the
    sum of the three magnitudes) for clouds far beyond the fixtures' 16 m; the flip's dot product carries the direction's own error of about 1e-12 times
    that length, so the zone in which either sign is right grows with it beyond 10^6 m and is the fixtures' 1e-6 below"""
    want = r["normals"]
    assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all(), what
    ok = well_posed(r)
    # where the flip's dot product is within 1e-6 of zero either side is right: those points are compared up to the sign
    sure = ok & (np.abs(r["view_dot"]) > (1e-6 if reach is None else np.maximum(1e-6, 1e-12 * np.asarray(reach, np.float64))))
    g, w = got[:, :3].astype(np.float64), want[:, :3].astype(np.float64)
    same, flipped = np.abs(g - w).max(axis=1), np.abs(g + w).max(axis=1)
    d = np.where(sure, same, np.minimum(same, flipped))[ok].max() if ok.any() else 0.0
    fin = np.isfinite(want[:, 3])
    dc = np.abs(got[fin, 3].astype(np.float64) - want[fin, 3].astype(np.float64))
    excess = (dc - (1e-12 + ULP * want[fin, 3].astype(np.float64))).max() if fin.any() else -1.0
    same_side = ((g * w).sum(axis=1) > 0.0)[sure]
    print(f"{what}: {int(ok.sum())} of {len(want)} points compared, max |component difference| {d:.3e} (bound {ULP:.3e}), "
          f"max curvature difference {dc.max() if fin.any() else 0.0:.3e}")
    assert d <= ULP, (what, d)
    assert excess <= 0.0, (what, excess)
    assert same_side.all(), what
    unit = np.abs(np.linalg.norm(got[fin, :3].astype(np.float64), axis=1) - 1.0)
    assert (unit < 1e-6).all(), what
    return d


@functools.lru_cache(maxsize=None)
def target_normals(kind, key=None):
    """the restatement's float normals (k = ICP_NORMAL_K, viewpoint_of(kind)) of an ICP fixture's target"""
    n = nref.estimate(_icp_clouds(kind, key)[0], ICP_NORMAL_K, viewpoint_of(kind))["normals"]
    n.setflags(write=False)
    return n


def viewpoint_of(kind):
    """the viewpoint of an ICP fixture's normals: the origin, moved along with the clouds"""
    return fx.FAR if kind == "far" else (0.0, 0.0, 0.0)


def _icp_clouds(kind, key):
    if kind == "scene":
        return fx.scene_pair(*fx.SCENES[key])
    if kind == "outlier":
        return fx.outlier_pair()
    if kind == "edge":
        return fx.edge_pairs()[key]
    if kind == "far":      # a scene pair FAR from the origin: both clouds moved by fx.FAR, in float
        t, s = fx.scene_pair(*fx.SCENES[key])
        return (t + np.float32(fx.FAR)).astype(np.float32), (s + np.float32(fx.FAR)).astype(np.float32)
    if kind == "lattice":
        return fx.lattice_pair(key) if key else fx.lattice_pair()
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def plane_fixture(kind, key=None, max_corr_dist=150.0):
    """(target, source, target normals, the plane restatement's result) of an ICP fixture"""
    t, s = _icp_clouds(kind, key)
    n = target_normals(kind, key)
    return t, s, n, plane_ref.align(t, n, s, max_corr_dist=max_corr_dist)


N_EDGE = 8      # len(fx.edge_pairs())
FAR_SCENE = "scene_3000_700"
FAR_SCALE = 1000.0      # the bounds of the far fixture: those of the near one times what tests/test_gpu_icp.py allows its far known answer (1e-9 against 1e-12)


def plane_z0(n=400, seed=61):
    """a single exact plane z = 0 and a source on it, moved a little inside the plane: three unknowns are not determined"""
    rng = np.random.default_rng(seed)
    t = np.concatenate([rng.uniform(-8.0, 8.0, (n, 2)), np.zeros((n, 1))], axis=1).astype(np.float32)
    s = (t[::3] + np.float32((0.05, -0.03, 0.0))).astype(np.float32)
    return t, s
