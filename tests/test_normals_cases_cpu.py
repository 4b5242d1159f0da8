"""CPU checks of the normals fixtures and of their restatement (tools/normals_numpy.py), no device needed: known answers, and the condition the GPU
comparison rests on -- at most 2 % of the points of a fixture have a direction that is not well-posed ((l1 - l0) / l2 below 1e-3), and the scene targets
have none."""
import numpy as np
import pytest

import icp_fixtures as fx
import normals_cases as nc
from tools import normals_numpy as nref


@pytest.mark.parametrize("name", nc.NORMALS_FIXTURES)
def test_fixture_is_well_posed(name):
    cloud, k, vp, r = nc.normals_fixture(name)
    ill = ~nc.well_posed(r)
    share = float(ill.mean())
    print(f"{name}: {int(ill.sum())} of {len(cloud)} points below the gap {nc.WELL_POSED_GAP:g}, smallest gap {np.nanmin(r['gap']):.3e}")
    assert share <= nc.MAX_ILL_POSED, (name, share)
    if not name.startswith("sphere"):
        assert not ill.any(), (name, int(ill.sum()))
    n = r["normals"]
    assert np.isfinite(n).all() and np.abs(np.linalg.norm(n[:, :3].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert (n[:, 3] >= 0.0).all() and (n[:, 3] <= 1.0 / 3.0 + 1e-6).all()
    # every normal looks towards the viewpoint
    assert (((np.asarray(vp) - cloud.astype(np.float64)) * r["normals64"][:, :3]).sum(axis=1) >= -1e-12).all()


def test_scene_fixtures_are_the_icp_targets():
    for scene in fx.SCENES:
        assert (nc.normals_fixture(scene + "_k10")[0] == fx.scene_fixture(scene)[0]).all()


def test_known_answers():
    # an exact plane: the normal is the plane's, towards the viewpoint, curvature 0
    t, _ = nc.plane_z0()
    for vp, nz in (((0.0, 0.0, 3.0), 1.0), ((0.0, 0.0, -3.0), -1.0)):
        r = nref.estimate(t, 10, vp)
        assert (r["normals"] == np.float32((0.0, 0.0, nz, 0.0))).all()
    # the sphere: radial, towards the centre, to the accuracy the neighbourhood's size allows
    cloud, k, vp, r = nc.normals_fixture("sphere_k16")
    radial = -cloud.astype(np.float64) / np.linalg.norm(cloud.astype(np.float64), axis=1)[:, None]
    assert ((r["normals64"][:, :3] * radial).sum(axis=1) > 0.98).all()
    # the neighbourhood holds the point itself first, and ties go to the smaller index
    assert (r["neighbours"][:, 0] == np.arange(len(cloud))).all()
    dup = np.float32([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0]])
    assert nref.neighbours(dup, 3).tolist()[0] == [0, 1, 2]


def test_edge_cases():
    rng = np.random.default_rng(5)
    # fewer than three finite points: NaN; non-finite points: NaN at their positions and nobody's neighbour
    for n in (0, 1, 2):
        r = nref.estimate(rng.uniform(-1, 1, (n, 3)), 10)
        assert r["normals"].shape == (n, 4) and np.isnan(r["normals"]).all()
    c = rng.uniform(-1, 1, (20, 3)).astype(np.float32)
    c[3, 1], c[11, 0] = np.nan, np.inf
    r = nref.estimate(c, 5)
    bad = np.zeros(20, bool)
    bad[[3, 11]] = True
    assert np.isnan(r["normals"][bad]).all() and np.isfinite(r["normals"][~bad]).all()
    assert not np.isin(r["neighbours"][~bad], (3, 11)).any()
    # k larger than the cloud: every point is every point's neighbour, one covariance up to the shift, one direction
    r = nref.estimate(c[~bad][:6], 64)
    assert r["neighbours"].shape == (6, 6) and np.abs(np.abs(r["normals64"][:, :3] @ r["normals64"][0, :3]) - 1.0).max() < 1e-9
    # coincident points: zero covariance, curvature 0, a finite unit normal
    r = nref.estimate(np.ones((5, 3), np.float32), 4)
    assert (r["normals"][:, 3] == 0).all() and np.abs(np.linalg.norm(r["normals"][:, :3], axis=1) - 1.0).max() < 1e-6
    for k in (2, 65):
        with pytest.raises(ValueError):
            nref.estimate(c, k)
