"""One workgroup of the range-culled vote kernel takes a run of T consecutive map tiles for one keyframe (LTM_VOTE_TILE_RUN): the pixel table, the pose
and the deferred uncertain-pixel survivors live across the tiles of the run.  Only the grouping of work changes: mode-0 labels must be the same bits
for T = 1, 2, 4, 8, for the exact-image kernel (LTM_VOTE_CULL=0) and for the CPU oracle -- on maps around the tile and run boundaries, keyframe counts
around the 8-keyframe group, with and without the steep-elevation clamp, with a lever-arm extrinsic, and on maps built to take the rare paths inside a
run: a tile out of reach, a tile that overflows the survivor queue, more uncertain-pixel survivors than their queue holds, duplicates across tiles."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HFOV = 360.0
TILE = 4096
RUN_LENGTHS = (1, 2, 4, 8)
MAP_SIZES = (4095, 4096, 4097, 2 * 4096 + 1, 8 * 4096, 32 * 4096 + 1, 33 * 4096 - 1)
KEYFRAMES = (1, 8, 9)
ALPHAS = (2.5, float(np.float32(0.95 * 2.5)), 1.5)
UQUEUE = 2048          # kCullQueue: capacity of the survivor queue of a tile and of the deferred uncertain-pixel queue of a run


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
    """one context per run length and one with the exact-image vote, of one configuration, and a pool of map points: the session's own map, then scattered points"""
    vfov, l2b = CONFIGS[request.param]
    L2B = np.eye(4) if l2b is None else l2b
    ctxs = {f"run{T}": _context(ltm, vfov, l2b, {"LTM_VOTE_TILE_RUN": str(T)}) for T in RUN_LENGTHS}
    ctxs["vote_exact"] = _context(ltm, vfov, l2b, {"LTM_VOTE_CULL": "0"})
    S = session9
    cmap = orc.voxel_centroid(orc.merge_to_global(S["scans"], S["offsets"], S["poses"], L2B), 0.05)
    rng = np.random.default_rng(11)
    extra = rng.normal(0, 25.0, size=(max(MAP_SIZES), 4)).astype(np.float32)
    extra[:, 2] = rng.normal(0, 4.0, size=len(extra))
    pool = np.concatenate([cmap, extra])[: max(MAP_SIZES)].copy()
    pool[0] = cmap[len(cmap) // 2]      # point 0 in a populated place
    yield {"vfov": vfov, "b2l": ltm.inverse4x4(L2B) if l2b is not None else np.eye(4), "L2B": L2B, "ctxs": ctxs, "pool": pool, "S": S}
    for c in ctxs.values():
        c.close()


def _labels_everywhere(rig, orc, cmap, scans, off, poses, inv, alpha, what):
    """the labels of every context, asserted equal to each other and to the oracle; returns the oracle's"""
    labels = {}
    for name, ctx in rig["ctxs"].items():
        g_map, g_scans, g_poses = ctx.upload(cmap), ctx.upload_scans(scans, off), ctx.poses(poses, inv)
        _, _, labels[name] = ctx.visibility_partition(g_map, g_scans, g_poses, alpha, 0.1, 0, want_labels=True)
    want = orc.vote_labels(cmap, scans, off, inv, rig["b2l"], rig["vfov"], HFOV, alpha, 0.1, 0)
    for name, got in labels.items():
        assert (got == want).all(), f"{what}: {name}: {(got != want).sum()} labels differ from the oracle"
    for T in RUN_LENGTHS:
        assert (labels[f"run{T}"] == labels["vote_exact"]).all(), f"{what}: run length {T} differs from the exact-image vote"
    return want


def _no_shape_failed(rig):
    for name, ctx in rig["ctxs"].items():
        checked, failed = ctx.cull_validation()
        assert failed == 0 and (checked >= 1 or name == "vote_exact"), f"{name}: the bounded-error projection must validate ({checked} checked, {failed} failed)"


def _session_part(S, nb):
    off = S["offsets"][: nb + 1]
    return S["scans"][: int(off[-1])], off, S["poses"][:nb], S["inv"][:nb]


@pytest.mark.parametrize("nb", KEYFRAMES)
def test_labels_do_not_depend_on_the_run_length(rig, orc, nb):
    scans, off, poses, inv = _session_part(rig["S"], nb)
    flagged = 0
    for i, M in enumerate(MAP_SIZES):
        alpha = ALPHAS[(i + nb) % len(ALPHAS)]
        flagged += int(_labels_everywhere(rig, orc, rig["pool"][:M], scans, off, poses, inv, alpha, f"M {M} nb {nb} alpha {alpha}").sum())
    assert flagged > 0, "degenerate test: nothing flagged at any size"
    _no_shape_failed(rig)


def _to_global(orc, local, pose, L2B):
    """sensor-frame points of one keyframe in the map frame, by the arithmetic the map itself was merged with"""
    p = np.zeros((len(local), 4), dtype=np.float32)
    p[:, :3] = local
    return orc.merge_to_global(p, np.array([0, len(p)], dtype=np.uint64), pose.reshape(1, 16), L2B)


def _in_front_of_returns(orc, rig, kf, n, metres):
    """n points `metres` in front of scan returns of keyframe kf, on the same rays: every one can be flagged, so every one survives the range cull"""
    S = rig["S"]
    loc = S["scans"][int(S["offsets"][kf]):int(S["offsets"][kf + 1]), :3].astype(np.float64)
    r = np.linalg.norm(loc, axis=1)
    loc, r = loc[r > 4.0 * metres], r[r > 4.0 * metres]
    assert len(loc) >= n
    pick = np.linspace(0, len(loc) - 1, n).astype(np.int64)
    return _to_global(orc, (loc[pick] * ((r[pick] - metres) / r[pick])[:, None]).astype(np.float32), S["poses"][kf], rig["L2B"])


def _uncertain_count(rig, pts, kf, alpha):
    """how many of `pts` (map frame) lie within the kernel's distrust band of a pixel-rounding boundary of keyframe kf's image (double arithmetic: an estimate)"""
    vfov = rig["vfov"]
    rows, cols = int(round(vfov * alpha)), int(round(HFOV * alpha))
    T = rig["b2l"] @ rig["S"]["inv"][kf].reshape(4, 4)
    p = pts[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    az, el = np.degrees(np.arctan2(p[:, 1], p[:, 0])), np.degrees(np.arctan2(p[:, 2], np.hypot(p[:, 0], p[:, 1])))
    colf, rowf = cols * (az + HFOV / 2) / HFOV, rows * (1.0 - (el + vfov / 2) / vfov)
    eps = 1.0e-3        # the floor of Geom::cull_eps_px; the band is never narrower
    near = lambda v: np.abs((v + 0.5) - np.round(v + 0.5)) < 0.5 * eps
    return int((near(colf) | near(rowf)).sum())


def test_rare_paths_inside_a_run(rig, orc):
    from tools.eps_sweep import boundary_points
    S, vfov, pool = rig["S"], rig["vfov"], rig["pool"]
    nb, alpha = 9, 2.5
    scans, off, poses, inv = _session_part(S, nb)
    rng = np.random.default_rng(23)
    maps = {}
    # 1. tiles 1 and 5 of nine wholly out of reach (5 km away): the second tile of a run of 2, a middle tile of the runs of 4 and 8
    m = pool[:9 * TILE].copy()
    for k in (1, 5):
        m[k * TILE:(k + 1) * TILE, :3] = (np.array([5000.0, 300.0, 20.0]) + rng.normal(0, 15.0, (TILE, 3))).astype(np.float32)
    maps["tile_out_of_reach"] = m
    # 2. tiles 1 and 5 overflow the survivor queue of keyframes 0 and 4: all of their points sit 1 m in front of that keyframe's scan returns
    m = pool[:9 * TILE].copy()
    m[1 * TILE:2 * TILE] = _in_front_of_returns(orc, rig, 0, TILE, 1.0)
    m[5 * TILE:6 * TILE] = _in_front_of_returns(orc, rig, 4, TILE, 1.0)
    maps["queue_overflow"] = m
    # 3. 1100 points on pixel boundaries of keyframe 2 in each of eight tiles: no tile overflows its survivor queue by them, every run of two or more
    #    tiles collects more than the deferred queue holds and has to serve the waiting ones early
    m = pool[:8 * TILE + 7].copy()
    n_edge = 1100
    edge = _to_global(orc, boundary_points(rng, 8 * n_edge, alpha, vfov, HFOV, 1.0e-6, 4.0, 30.0), S["poses"][2], rig["L2B"])
    for k in range(8):
        m[k * TILE + 5:k * TILE + 5 + n_edge] = edge[k * n_edge:(k + 1) * n_edge]
        assert _uncertain_count(rig, m[k * TILE:(k + 1) * TILE], 2, alpha) <= UQUEUE - 400, "a tile must not overflow its own queue by the edge points alone"
    for T in (2, 4, 8):
        assert _uncertain_count(rig, m[:T * TILE], 2, alpha) > UQUEUE, f"the first run of {T} tiles must exceed the deferred queue"
    maps["uncertain_overflow"] = m
    # 4. the same coordinates under different indices in different tiles of one run: the lowest index must win the pixel.  The first 600 are points
    #    that keyframe 0 flags (1 m in front of its returns), few enough to stay in the survivor queue
    m = pool[:4 * TILE + 3].copy()
    n_dup = 600
    m[:n_dup] = _in_front_of_returns(orc, rig, 0, n_dup, 1.0)
    m[1 * TILE:2 * TILE] = m[0:TILE]
    m[3 * TILE + 100:4 * TILE] = m[100:TILE]
    m[4 * TILE:] = m[:3]
    maps["duplicates"] = m
    for name, cmap in maps.items():
        want = _labels_everywhere(rig, orc, cmap, scans, off, poses, inv, alpha, name)
        assert want.sum() > 0, f"degenerate case: nothing flagged in {name}"
        if name == "duplicates":      # of equal points only the first can have won a pixel
            assert want[:n_dup].sum() > 0 and want[TILE:2 * TILE].sum() == 0 and want[3 * TILE + 100:].sum() == 0, "a copy never wins against its original"
    _no_shape_failed(rig)


def test_a_lane_votes_like_its_parent(rig):
    """a lane inherits the run length of the context it was made from"""
    ctx = rig["ctxs"]["run4"]
    lane = ctx.lane()
    scans, off, poses, inv = _session_part(rig["S"], 9)
    cmap = rig["pool"][:9 * TILE + 11]
    out = []
    for c in (ctx, lane):
        _, _, labels = c.visibility_partition(c.upload(cmap), c.upload_scans(scans, off), c.poses(poses, inv), 2.5, 0.1, 0, want_labels=True)
        out.append(labels)
    lane.close()
    assert out[0].sum() > 0 and (out[0] == out[1]).all()
