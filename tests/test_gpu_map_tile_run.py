"""One workgroup of the exact-image kernel takes a run of T consecutive map tiles for one keyframe (LTM_MAP_TILE_RUN): pose, pixel table, the table of range
bounds and the flush live across the tiles of the run, every wave keeps its survivors in a segment of its own (376 words) and gives them their exact range
when a group of 4 x 64 points does not fit any more, and the uncertain-pixel survivors of the run wait in a queue of 256.  None of this may show: the
reprojected scans (points and offsets) and the mode-1 labels must be the same bits for T = 1, 2, 4, 8, 16, for the two A/B forms (tables reset per tile, a
barrier between the two halves of the pre-filter), for the list-driven launch (which keeps the one-tile kernel), for k_map_rimg_lds (LTM_MAP_KERNEL=1, not
touched by any of this) and for the CPU oracle -- on maps of 2 to 9 tiles built to take each path."""
import numpy as np
import pytest

from test_gpu_vote_tile_run import CONFIGS, HFOV, TILE, _context, _session_part, _to_global, _uncertain_count
from test_gpu_vote_wave_queue import _shape, _wave_slice

pytestmark = pytest.mark.gpu

RUN_LENGTHS = (1, 2, 4, 8)
MAX_TILES = 10
SEGMENT = 376                      # queue words of one wave
UQUEUE = 256                       # uncertain-pixel survivors of a run that can wait for the run's end
NPX_LIMIT = (1 << 18) - 1          # the queue word of the vote kernel: 18 bits of linear pixel index, all ones = pixel not certain
NB = 9


@pytest.fixture(scope="module")
def session9():
    from tools import synth
    return synth.to_numpy(synth.make_session(1, NB, "small"))


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def rig(request, ltm, orc, session9):
    vfov, l2b = CONFIGS[request.param]
    L2B = np.eye(4) if l2b is None else l2b
    plain = {"LTM_OCCLUSION_MIN_PAIRS": str(1 << 40)}
    ctxs = {"lds": _context(ltm, vfov, l2b, dict(plain, LTM_MAP_KERNEL="1"))}
    for T in RUN_LENGTHS:
        ctxs[f"run{T}"] = _context(ltm, vfov, l2b, dict(plain, LTM_MAP_TILE_RUN=str(T)))
    ctxs["run16"] = _context(ltm, vfov, l2b, dict(plain, LTM_MAP_TILE_RUN="16"))
    ctxs["run_by_launch"] = _context(ltm, vfov, l2b, plain)              # no run length given: chosen per launch, one tile per workgroup on maps this small
    ctxs["run4_reset_per_tile"] = _context(ltm, vfov, l2b, dict(plain, LTM_MAP_TILE_RUN="4", LTM_MAP_TILE_PERSIST="0"))
    ctxs["run4_barrier"] = _context(ltm, vfov, l2b, dict(plain, LTM_MAP_TILE_RUN="4", LTM_MAP_TILE_BARRIER="1"))
    ctxs["run1_barrier"] = _context(ltm, vfov, l2b, dict(plain, LTM_MAP_TILE_RUN="1", LTM_MAP_TILE_BARRIER="1"))
    # diagnostics: ltm_debug_cull_stats reports the exact-image kernels' sampled {survivors, points} (every 64th workgroup; one device-wide counter)
    ctxs["stats_run1"] = _context(ltm, vfov, l2b, dict(plain, LTM_MAP_TILE_RUN="1", LTM_STATS_BLOCKMIN="1"))
    ctxs["stats_run4"] = _context(ltm, vfov, l2b, dict(plain, LTM_MAP_TILE_RUN="4", LTM_STATS_BLOCKMIN="1"))
    # the list-driven launch for every image: all pairs in the first shell (nothing hidden), and a first shell of 2 m (later shells behind the cull)
    ctxs["list"] = _context(ltm, vfov, l2b, {"LTM_OCCLUSION": "1", "LTM_OCCLUSION_MIN_PAIRS": "1", "LTM_OCCLUSION_RNEAR": "10000"})
    ctxs["list_shells"] = _context(ltm, vfov, l2b, {"LTM_OCCLUSION": "1", "LTM_OCCLUSION_MIN_PAIRS": "1", "LTM_OCCLUSION_RNEAR": "2", "LTM_OCCLUSION_STATS": "1"})
    S = session9
    cmap = orc.voxel_centroid(orc.merge_to_global(S["scans"], S["offsets"], S["poses"], L2B), 0.05)
    rng = np.random.default_rng(17)
    n = MAX_TILES * TILE
    extra = rng.normal(0, 25.0, size=(n, 4)).astype(np.float32)
    extra[:, 2] = rng.normal(0, 4.0, size=n)
    pool = np.concatenate([cmap, extra])[:n].copy()
    yield {"vfov": vfov, "b2l": ltm.inverse4x4(L2B) if l2b is not None else np.eye(4), "L2B": L2B, "ctxs": ctxs, "pool": pool, "S": S}
    for c in ctxs.values():
        c.close()


def _no_shape_failed(rig):
    """every context that runs the pre-filter validated the bounded-error projection for its image shapes, and none fell back to the exact kernels"""
    for name, ctx in rig["ctxs"].items():
        checked, failed = ctx.cull_validation()
        assert failed == 0 and (checked >= 1 or name == "lds"), f"{name}: the bounded-error projection must validate ({checked} checked, {failed} failed)"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _images_everywhere(rig, orc, cmap, alpha, what, nb=NB, kb=1):
    """reprojection of keyframes [kb, nb) and mode-1 labels against keyframes [0, nb) in every context, asserted equal to k_map_rimg_lds's and to the
    oracle's bit for bit; returns the oracle's (points, offsets, labels)"""
    assert 2 * TILE <= len(cmap) <= MAX_TILES * TILE and 0 < kb < nb
    scans, off, poses, inv = _session_part(rig["S"], nb)
    got = {}
    for name, ctx in rig["ctxs"].items():
        g_map, g_scans, g_poses = ctx.upload(cmap), ctx.upload_scans(scans, off), ctx.poses(poses, inv)
        pts, offs = ctx.reproject(g_map, g_poses, alpha, kb, nb).download()
        _, _, labels = ctx.visibility_partition(g_map, g_scans, g_poses, alpha, 0.1, 1, want_labels=True)
        got[name] = (pts, np.asarray(offs, dtype=np.uint64), labels)
    o_pts, o_off = orc.reproject(cmap, inv, rig["b2l"], rig["vfov"], HFOV, alpha, kb, nb)
    o_lab = orc.vote_labels(cmap, scans, off, inv, rig["b2l"], rig["vfov"], HFOV, alpha, 0.1, 1)
    for ref_name, (r_pts, r_off, r_lab) in (("oracle", (o_pts, np.asarray(o_off, dtype=np.uint64), o_lab)), ("lds", got["lds"])):
        for name, (pts, offs, labels) in got.items():
            assert (offs == r_off).all(), f"{what}: {name}: offsets differ from {ref_name}"
            assert pts.shape == r_pts.shape and (_bits(pts) == _bits(r_pts)).all(), f"{what}: {name}: reprojected points differ from {ref_name}"
            assert (labels == r_lab).all(), f"{what}: {name}: {(labels != r_lab).sum()} mode-1 labels differ from {ref_name}"
    assert len(o_pts) > 0, f"degenerate case: {what}: empty reprojection"
    return o_pts, o_off, o_lab


def _on_rays(orc, rig, kf, n, metres):
    """n points on rays of scan returns of keyframe kf, `metres` nearer to the sensor than the return (farther if negative), in the map frame.  The rays do
    not depend on `metres`: point i of one call shares its ray, hence its pixel, with point i of another."""
    S = rig["S"]
    loc = S["scans"][int(S["offsets"][kf]):int(S["offsets"][kf + 1]), :3].astype(np.float64)
    r = np.linalg.norm(loc, axis=1)
    loc, r = loc[r > 6.0], r[r > 6.0]
    assert len(loc) >= n
    pick = np.linspace(0, len(loc) - 1, n).astype(np.int64)
    return _to_global(orc, (loc[pick] * ((r[pick] - metres) / r[pick])[:, None]).astype(np.float32), S["poses"][kf], rig["L2B"])


@pytest.mark.parametrize("nb,kb", [(3, 1), (9, 2)])
def test_images_do_not_depend_on_the_run_length(rig, orc, nb, kb):
    """tile counts around the run lengths; the partial last tile inside a run (3 tiles + 5 points with T = 4) and alone in one (4 tiles + 7 with T = 2 and 4,
    8 tiles + 100 with T = 8); 50 x 360 images (alpha 1), the shipped 125 x 900 and 150 x 1080"""
    sizes = (2 * TILE, 2 * TILE + 1, 3 * TILE + 5, 4 * TILE + 7, 7 * TILE + 3, 8 * TILE + 100)
    alphas = (1.0, 2.5, 3.0)
    for i, M in enumerate(sizes):
        alpha = alphas[(i + nb) % len(alphas)]
        _images_everywhere(rig, orc, rig["pool"][:M], alpha, f"M {M} nb {nb} kb {kb} alpha {alpha}", nb, kb)
    _no_shape_failed(rig)


def test_lowest_index_wins_between_tiles_waves_and_drains(rig, orc):
    m = rig["pool"][:4 * TILE + 3].copy()
    orig = _wave_slice(0, 0, range(8))                   # 512 points of wave 0 of tile 0, each the nearest of its pixel for keyframe 2: more than a segment holds
    m[orig, :3] = _on_rays(orc, rig, 2, len(orig), 1.5)[:, :3]
    copies = {"same wave, behind a drain": _wave_slice(0, 0, range(8, 16)), "another wave of the tile": _wave_slice(0, 3, range(8)),
              "the next tile of the run": _wave_slice(1, 1, range(8)), "the fourth tile": np.arange(3 * TILE + 7, 3 * TILE + 7 + len(orig)),
              "the partial tile": np.arange(4 * TILE, 4 * TILE + 3)}
    for idx in copies.values():
        m[idx, :3] = m[orig[:len(idx)], :3]              # the same coordinates under a fourth channel of their own: the winner shows in the output
    assert len(orig) > SEGMENT
    _, _, labels = _images_everywhere(rig, orc, m, 2.5, "bit-equal points")
    assert labels[orig].sum() > 0, "some originals are flagged"
    for name, idx in copies.items():
        assert labels[idx].sum() == 0, f"{name}: a copy never wins against its original"


def test_one_wave_drains_again_and_again(rig, orc):
    """tile 1: all 1024 points of wave 2 are the nearest of their pixels, more than twice what its segment holds: that wave drains inside the tile, more
    than once, while the other waves, which see the pool's points, do not"""
    m = rig["pool"][:5 * TILE + 5].copy()
    idx = _wave_slice(1, 2)
    m[idx, :3] = _on_rays(orc, rig, 3, len(idx), 2.0)[:, :3]
    assert len(idx) > 2 * SEGMENT
    _, _, labels = _images_everywhere(rig, orc, m, 2.5, "one wave drains")
    assert labels[idx].sum() > 0
    _no_shape_failed(rig)


def test_far_tile_behind_a_near_one_in_the_same_pixels(rig, orc):
    """tiles 0 / 1 (one run for T >= 2): near points, then farther points on the same rays -- the bounds of tile 0 are still in the table when tile 1 is
    tested; tiles 2 / 3: the far ones first.  Keyframe 2's image holds the near ones either way."""
    m = rig["pool"][:6 * TILE + 9].copy()
    near, far = _on_rays(orc, rig, 2, TILE, 2.0)[:, :3], _on_rays(orc, rig, 2, TILE, -3.0)[:, :3]
    m[0:TILE, :3], m[TILE:2 * TILE, :3] = near, far
    m[2 * TILE:3 * TILE, :3], m[3 * TILE:4 * TILE, :3] = far + np.float32(1.0e-3), near + np.float32(1.0e-3)
    _, _, labels = _images_everywhere(rig, orc, m, 2.5, "far behind near")
    assert labels[:4 * TILE].sum() > 0, "degenerate case: none of the placed points is flagged"


def test_uncertain_queue_past_its_capacity_inside_a_run(rig, orc):
    from tools.eps_sweep import boundary_points
    rng = np.random.default_rng(37)
    alpha = 2.5
    m = rig["pool"][:8 * TILE + 7].copy()
    n_edge = 170
    edge = _to_global(orc, boundary_points(rng, 8 * n_edge, alpha, rig["vfov"], HFOV, 1.0e-6, 4.0, 30.0), rig["S"]["poses"][2], rig["L2B"])
    for k in range(8):
        m[k * TILE + 5:k * TILE + 5 + n_edge] = edge[k * n_edge:(k + 1) * n_edge]
    assert _uncertain_count(rig, m[:TILE], 2, alpha) < UQUEUE, "one tile alone stays inside the queue"
    for T in (2, 4, 8):
        assert _uncertain_count(rig, m[:T * TILE], 2, alpha) > UQUEUE, f"the first run of {T} tiles exceeds it"
    _images_everywhere(rig, orc, m, alpha, "uncertain queue past capacity in a run")
    m2 = rig["pool"][:3 * TILE + 9].copy()               # and inside one tile, with drains of the certain survivors around it
    m2[TILE + 5:TILE + 5 + 3000] = _to_global(orc, boundary_points(rng, 3000, alpha, rig["vfov"], HFOV, 1.0e-6, 4.0, 30.0), rig["S"]["poses"][2], rig["L2B"])
    assert _uncertain_count(rig, m2[TILE:2 * TILE], 2, alpha) > UQUEUE
    _images_everywhere(rig, orc, m2, alpha, "uncertain queue past capacity in a tile")
    _no_shape_failed(rig)


def test_either_side_of_the_pixel_field_limit_and_an_unpackable_shape(rig, orc):
    """the run kernel's queue word is the vote kernel's: fast path iff rows * cols <= 2^18 - 1 (test_gpu_vote_wave_queue derives the shapes); alpha 6 gives
    300 x 2160 / 540 x 2160, which neither that word nor the one-tile kernel's 9 + 11 bits of row and column hold: every tile takes the exact path"""
    vfov = rig["vfov"]
    c_fit, c_over = {50.0: (1372, 1373), 90.0: (1023, 1024)}[vfov]
    (a_fit, r_fit), (a_over, r_over) = _shape(vfov, c_fit), _shape(vfov, c_over)
    assert r_fit * c_fit <= NPX_LIMIT < r_over * c_over
    m = rig["pool"][:3 * TILE + 3].copy()
    idx = _wave_slice(1, 1)
    m[idx, :3] = _on_rays(orc, rig, 2, len(idx), 2.0)[:, :3]
    for alpha in (a_fit, a_over, 6.0):
        _images_everywhere(rig, orc, m, alpha, f"alpha {alpha}", nb=4, kb=1)
    _no_shape_failed(rig)


def _survivors(ctx, rig, cmap, alpha):
    """sampled {survivors, points} of one reprojection of all nine keyframes"""
    scans, off, poses, inv = _session_part(rig["S"], NB)
    g_map, g_poses = ctx.upload(cmap), ctx.poses(poses, inv)
    ctx.cull_stats()
    ctx.reproject(g_map, g_poses, alpha, 0, NB).download()
    return ctx.cull_stats()


def test_the_pre_filter_and_the_run_length_are_really_taken(rig):
    """The exact path gives the same bits, so the other tests would pass with the pre-filter off or the run length ignored.  The sampled counters tell:
    of a map of 8 tiles + 7 points and 9 keyframes the workgroups 0, 64, ... are sampled -- with T = 1 (run 0 | run 8, the partial tile) x (keyframe 0 | 8),
    i.e. 2 full tiles; with T = 4 run 0 of three x (keyframe 0 | 8), i.e. 2 x 4 full tiles.  Survivors are fewer than the points on the fast path (how many fewer depends on how many points share a pixel: no bound is set) and
    every point on the exact path (300 x 2160 / 540 x 2160 at alpha 6 fit neither queue word); the first shape past the run kernel's pixel field
    still fits the one-tile kernel's record and keeps the pre-filter there."""
    vfov = rig["vfov"]
    m = rig["pool"][:8 * TILE + 7]
    surv1, pts1 = _survivors(rig["ctxs"]["stats_run1"], rig, m, 2.5)
    surv4, pts4 = _survivors(rig["ctxs"]["stats_run4"], rig, m, 2.5)
    assert pts1 == 2 * TILE and pts4 == 8 * TILE, "the run length decides which workgroups are sampled and how many tiles each one has"
    assert 0 < surv1 < pts1 and 0 < surv4 < pts4, "fast path: the pre-filter drops points (on the exact path every point counts as a survivor)"
    c_fit, c_over = {50.0: (1372, 1373), 90.0: (1023, 1024)}[vfov]
    for T, ctx in ((1, rig["ctxs"]["stats_run1"]), (4, rig["ctxs"]["stats_run4"])):
        s_fit, p_fit = _survivors(ctx, rig, m, _shape(vfov, c_fit)[0])
        assert p_fit == (2 if T == 1 else 8) * TILE and 0 < s_fit < p_fit, f"T {T}: the largest shape of the pixel field is on the fast path"
        s_over, p_over = _survivors(ctx, rig, m, _shape(vfov, c_over)[0])
        assert p_over == 2 * TILE and 0 < s_over < p_over, f"T {T}: the next shape keeps its pre-filter in the one-tile kernel (one tile per workgroup)"
        s_big, p_big = _survivors(ctx, rig, m, 6.0)
        assert p_big == (2 if T == 1 else 8) * TILE and s_big == p_big, f"T {T}: an image that fits no queue word takes the exact path, every point a survivor"


def test_the_list_driven_launch_is_taken_with_later_shells(rig, orc):
    _images_everywhere(rig, orc, rig["pool"][:5 * TILE + 1], 2.5, "list-driven launch")
    pairs, near, far_live = rig["ctxs"]["list_shells"].occlusion_stats()
    assert pairs > 0 and near < pairs, "with a first shell of 2 m most pairs wait for a later shell, where the cull and its quarter masks apply"
