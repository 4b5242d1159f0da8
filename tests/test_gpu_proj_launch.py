"""The projection kernels take their launch constants (ProjLaunch) from the host instead of recomputing them in every thread, and the workgroup ->
(tile, keyframe) mapping from shifts and a multiply-high.  Nothing a caller can see may change: mode-0 labels of the culled vote kernel against the
exact-image kernel (LTM_VOTE_CULL=0), reprojection scan sets of the pre-filtered arg-min kernel against the plain LDS one (LTM_MAP_KERNEL=1), both
against the CPU oracle, bitwise -- on maps around the 4096-point tile and the 8-tile group boundaries, keyframe counts around the 8-keyframe group,
fields of view with and without the steep-elevation clamp, and a base->lidar extrinsic with a lever arm."""
import os

import numpy as np
import pytest

from conftest import assert_clouds_equal

pytestmark = pytest.mark.gpu

HFOV = 360.0
MAP_SIZES = (1, 4095, 4096, 4097, 8 * 4096, 8 * 4096 + 1, 9 * 4096 - 1)
KEYFRAMES = (1, 7, 8, 9)
ALPHAS = (2.5, float(np.float32(0.95 * 2.5)), 1.5, 3.0)


def _lever():
    c, s = np.cos(0.4), np.sin(0.4)
    T = np.eye(4)
    T[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[np.cos(0.03), 0, np.sin(0.03)], [0, 1, 0], [-np.sin(0.03), 0, np.cos(0.03)]])
    T[:3, 3] = (0.9, -0.3, 1.7)
    return T


CONFIGS = {"vfov50": (50.0, None), "vfov90_no_steep_clamp": (90.0, None), "vfov50_lever_arm": (50.0, _lever())}


def _context(ltm, vfov, l2b, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ltm.Context(vfov=vfov, hfov=HFOV, lidar2base=l2b, device=0)      # the switches are read when the context is created
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def session9():
    from tools import synth
    return synth.to_numpy(synth.make_session(1, 9, "small"))


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def rig(request, ltm, orc, session9):
    """three contexts of one configuration (default, exact vote, plain LDS image kernel) and a pool of map points: the session's own map, then scattered points"""
    vfov, l2b = CONFIGS[request.param]
    L2B = np.eye(4) if l2b is None else l2b
    ctxs = {"default": _context(ltm, vfov, l2b, {}), "vote_exact": _context(ltm, vfov, l2b, {"LTM_VOTE_CULL": "0"}),
            "image_lds": _context(ltm, vfov, l2b, {"LTM_MAP_KERNEL": "1"})}
    S = session9
    cmap = orc.voxel_centroid(orc.merge_to_global(S["scans"], S["offsets"], S["poses"], L2B), 0.05)
    rng = np.random.default_rng(11)
    extra = rng.normal(0, 25.0, size=(max(MAP_SIZES), 4)).astype(np.float32)
    extra[:, 2] = rng.normal(0, 4.0, size=len(extra))
    pool = np.concatenate([cmap, extra])[: max(MAP_SIZES)].copy()
    pool[0] = cmap[len(cmap) // 2]      # point 0 in a populated place
    yield {"vfov": vfov, "b2l": ltm.inverse4x4(L2B) if l2b is not None else np.eye(4), "l2b": l2b, "ctxs": ctxs, "pool": pool, "S": S}
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("nb", KEYFRAMES)
def test_labels_and_scan_sets_are_unchanged(rig, orc, nb):
    S, vfov, b2l = rig["S"], rig["vfov"], rig["b2l"]
    off = S["offsets"][: nb + 1]
    scans = S["scans"][: int(off[-1])]
    poses, inv = S["poses"][:nb], S["inv"][:nb]
    flagged = 0
    for i, M in enumerate(MAP_SIZES):
        alpha = ALPHAS[(i + nb) % len(ALPHAS)]
        cmap = rig["pool"][:M]
        labels, rep = {}, {}
        for name, ctx in rig["ctxs"].items():
            g_map, g_scans, g_poses = ctx.upload(cmap), ctx.upload_scans(scans, off), ctx.poses(poses, inv)
            if name != "image_lds":
                _, _, labels[name] = ctx.visibility_partition(g_map, g_scans, g_poses, alpha, 0.1, 0, want_labels=True)
            if name != "vote_exact":
                rep[name] = ctx.reproject(g_map, g_poses, alpha).download()
        want = orc.vote_labels(cmap, scans, off, inv, b2l, vfov, HFOV, alpha, 0.1, 0)
        what = f"M {M} nb {nb} alpha {alpha}"
        assert (labels["default"] == labels["vote_exact"]).all(), f"{what}: culled vote differs from the exact-image vote"
        assert (labels["default"] == want).all(), f"{what}: {(labels['default'] != want).sum()} labels differ from the oracle"
        flagged += int(want.sum())
        o_pts, o_off = orc.reproject(cmap, inv, b2l, vfov, HFOV, alpha)
        for name in ("default", "image_lds"):
            assert (rep[name][1] == o_off).all(), f"{what}: {name} offsets differ from the oracle"
            assert_clouds_equal(rep[name][0], o_pts, f"{what}: {name} scan set")
    assert flagged > 0, "degenerate test: nothing flagged at any size"
    checked, failed = rig["ctxs"]["default"].cull_validation()
    assert checked >= 1 and failed == 0, "the bounded-error projection must validate with the constants the hot kernels use"


def test_device_evaluation_of_the_old_expressions_gives_the_host_constants(rig, ltm):
    """one device thread evaluates what every thread of the kernels used to evaluate; the host structure must hold the same bits"""
    vfov, l2b = rig["vfov"], rig["l2b"]
    b2l = None if l2b is None else rig["b2l"]
    for alpha in ALPHAS + (2.0, 1.0):
        for M in (1, 9 * 4096 - 1, 11000 * 4096):
            hf, hu, _, _ = ltm.proj_launch(vfov, HFOV, alpha, b2l, map_points=M, n_keyframes=9)
            df, du, _, _ = ltm.proj_launch(vfov, HFOV, alpha, b2l, map_points=M, n_keyframes=9, on_device=True)
            for k in hf:
                assert np.float32(hf[k]).view(np.uint32) == np.float32(df[k]).view(np.uint32), f"{k} at alpha {alpha}: host {hf[k]!r} device {df[k]!r}"
            assert hu == du
