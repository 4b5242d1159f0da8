"""The range-culled vote kernel keeps its survivors in four wave-private queue segments of 512 words: a wave walks its quarter of every tile of the run
(the points with (tile-local index % 256) // 64 == wave) as one stream, and gives its survivors their exact range whenever another group of 4 x 64
points could overflow its segment (more than 256 entries) and once behind the run.  A queue word carries tile in run (4 bits), group (4), lane (6) and
the pixel as a linear index (18 bits, all ones = pixel not certain); uncertain survivors go to a queue of 2048 shared by the workgroup, and a ticket
past its capacity is served on the spot.  None of this may show in the result: mode-0 labels must be the same bits for run lengths 1, 4 and 16, for the
exact-image kernel (LTM_VOTE_CULL=0) and for the CPU oracle, on maps of at most 17 tiles built to take each of these paths."""
import numpy as np
import pytest

from test_gpu_vote_tile_run import CONFIGS, HFOV, TILE, UQUEUE, _context, _in_front_of_returns, _no_shape_failed, _session_part, _to_global, _uncertain_count

pytestmark = pytest.mark.gpu

RUN_LENGTHS = (1, 4, 16)
MAX_TILES = 17
SEGMENT = 512                      # queue words of one wave
DRAIN_AT = SEGMENT - 4 * 64        # a wave drains in front of a group when it holds more than this
NPX_LIMIT = (1 << 18) - 1          # largest rows * cols whose pixel indices all stay below the all-ones value of the 18-bit field
NB, ALPHA = 9, 2.5


@pytest.fixture(scope="module")
def session9():
    from tools import synth
    return synth.to_numpy(synth.make_session(1, 9, "small"))


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def rig(request, ltm, orc, session9):
    """as the rig of test_gpu_vote_tile_run: one context per run length and one with the exact-image vote, and a pool of map points"""
    vfov, l2b = CONFIGS[request.param]
    L2B = np.eye(4) if l2b is None else l2b
    ctxs = {f"run{T}": _context(ltm, vfov, l2b, {"LTM_VOTE_TILE_RUN": str(T)}) for T in RUN_LENGTHS}
    ctxs["vote_exact"] = _context(ltm, vfov, l2b, {"LTM_VOTE_CULL": "0"})
    S = session9
    cmap = orc.voxel_centroid(orc.merge_to_global(S["scans"], S["offsets"], S["poses"], L2B), 0.05)
    rng = np.random.default_rng(11)
    n = MAX_TILES * TILE
    extra = rng.normal(0, 25.0, size=(n, 4)).astype(np.float32)
    extra[:, 2] = rng.normal(0, 4.0, size=n)
    pool = np.concatenate([cmap, extra])[:n].copy()
    yield {"vfov": vfov, "b2l": ltm.inverse4x4(L2B) if l2b is not None else np.eye(4), "L2B": L2B, "ctxs": ctxs, "pool": pool, "S": S}
    for c in ctxs.values():
        c.close()


def _labels(rig, orc, cmap, alpha, what):
    """the labels of every context, asserted equal to the exact-image vote's and to the oracle's; returns the oracle's"""
    scans, off, poses, inv = _session_part(rig["S"], NB)
    assert len(cmap) <= MAX_TILES * TILE
    labels = {}
    for name, ctx in rig["ctxs"].items():
        g_map, g_scans, g_poses = ctx.upload(cmap), ctx.upload_scans(scans, off), ctx.poses(poses, inv)
        _, _, labels[name] = ctx.visibility_partition(g_map, g_scans, g_poses, alpha, 0.1, 0, want_labels=True)
    want = orc.vote_labels(cmap, scans, off, inv, rig["b2l"], rig["vfov"], HFOV, alpha, 0.1, 0)
    for name, got in labels.items():
        assert (got == want).all(), f"{what}: {name}: {(got != want).sum()} labels differ from the oracle"
    for T in RUN_LENGTHS:
        assert (labels[f"run{T}"] == labels["vote_exact"]).all(), f"{what}: run length {T} differs from the exact-image vote"
    assert want.sum() > 0, f"degenerate case: nothing flagged in {what}"
    return want


def _wave_slice(tile, wave, groups=range(16)):
    """map indices of the points of `tile` that wave `wave` walks, in the order it walks them: group by group, 64 consecutive points each"""
    return np.concatenate([tile * TILE + g * 256 + wave * 64 + np.arange(64) for g in groups])


def test_one_wave_drains_and_the_others_do_not(rig, orc):
    m = rig["pool"][:5 * TILE + 5].copy()
    idx = _wave_slice(1, 2)
    assert (((idx - TILE) % 256) // 64 == 2).all()
    m[idx] = _in_front_of_returns(orc, rig, 0, len(idx), 1.0)
    assert len(idx) == 1024 > SEGMENT, "wave 2's slice holds more survivors than its segment: it has to drain inside the tile"
    want = _labels(rig, orc, m, ALPHA, "one wave drains")
    assert want[idx].sum() > 0, "some of the placed points are flagged"
    _no_shape_failed(rig)


def test_lowest_index_wins_across_a_drain(rig, orc):
    m = rig["pool"][:4 * TILE + 3].copy()
    orig = _wave_slice(0, 0, range(8))              # the first 512 points wave 0 sees: more than DRAIN_AT, so a drain comes before it sees the rest
    assert len(orig) == SEGMENT > DRAIN_AT
    m[orig] = _in_front_of_returns(orc, rig, 0, len(orig), 1.0)
    later = _wave_slice(0, 0, range(8, 16))         # bit-equal copies behind the drain, in the same wave's stream ...
    m[later] = m[orig]
    other = _wave_slice(0, 3, range(8))             # ... in another wave of the same tile ...
    m[other] = m[orig]
    nxt = _wave_slice(1, 0, range(8))               # ... and in the next tile of the run
    m[nxt] = m[orig]
    m[2 * TILE + 7:2 * TILE + 7 + len(orig)] = m[orig]
    want = _labels(rig, orc, m, ALPHA, "duplicates across a drain")
    assert want[orig].sum() > 0, "some originals are flagged"
    for name, copies in (("same wave", later), ("other wave", other), ("next tile", nxt), ("third tile", np.arange(2 * TILE + 7, 2 * TILE + 7 + len(orig)))):
        assert want[copies].sum() == 0, f"{name}: a copy never wins against its original"


def test_the_largest_tile_in_run_field(rig, orc):
    from tools.eps_sweep import boundary_points
    rng = np.random.default_rng(29)
    m = rig["pool"][:MAX_TILES * TILE].copy()        # run length 16: tiles 0 .. 15 are one run (tile field 0 .. 15), tile 16 starts the next
    n = 300
    for k, kf in ((0, 0), (15, 4), (16, 7)):         # (in front of another keyframe's returns in each tile: equal points would leave the win to tile 0)
        m[k * TILE + 11:k * TILE + 11 + n] = _in_front_of_returns(orc, rig, kf, n, 1.0)
        m[k * TILE + 2049:k * TILE + 2049 + n] = _to_global(orc, boundary_points(rng, n, ALPHA, rig["vfov"], HFOV, 1.0e-6, 4.0, 30.0), rig["S"]["poses"][2], rig["L2B"])
        assert _uncertain_count(rig, m[k * TILE:(k + 1) * TILE], 2, ALPHA) >= n // 2, "the tile holds points on pixel boundaries"
    want = _labels(rig, orc, m, ALPHA, "tiles 0, 15 and 16 of 17")
    for k in (0, 15, 16):
        assert want[k * TILE + 11:k * TILE + 11 + n].sum() > 0, f"tile {k}: some of the placed points are flagged"
    _no_shape_failed(rig)


def _shape(vfov, cols):
    alpha = float(np.float32(cols / HFOV))
    rows = int(np.round(np.float32(vfov) * np.float32(alpha)))
    assert int(np.round(np.float32(HFOV) * np.float32(alpha))) == cols
    return alpha, rows


def test_either_side_of_the_pixel_field_limit(rig, orc, ltm):
    """The pixel field holds 18 bits and its all-ones value means "not certain", so a shape is on the fast path when rows * cols <= 2^18 - 1 = 262143 --
    whatever the run length, the field widths do not depend on it.  rows = round(vfov alpha), cols = round(360 alpha):
      vfov 50: 262143 / 191 = 1372.5 -> 191 x 1372 = 262052 (alpha 1372 / 360) fits, 191 x 1373 = 262243 (alpha 1373 / 360) is the next shape and does not;
      vfov 90: 256 x 1023 = 261888 (alpha 1023 / 360) fits, 256 x 1024 = 262144 = 2^18 does not: its last pixel index would be the all-ones value."""
    vfov = rig["vfov"]
    c_fit, c_over = {50.0: (1372, 1373), 90.0: (1023, 1024)}[vfov]
    (a_fit, r_fit), (a_over, r_over) = _shape(vfov, c_fit), _shape(vfov, c_over)
    assert r_fit * c_fit <= NPX_LIMIT < r_over * c_over
    assert (r_fit * c_fit, r_over * c_over) == {50.0: (262052, 262243), 90.0: (261888, 262144)}[vfov]
    for alpha, rows, cols, fast in ((a_fit, r_fit, c_fit, 1), (a_over, r_over, c_over, 0)):
        u, _, _ = ltm.vote_queue_word(vfov, HFOV, alpha)
        assert (u["rows"], u["cols"], u["fast_path"]) == (rows, cols, fast)
    m = rig["pool"][:5 * TILE + 3].copy()
    idx = _wave_slice(1, 1)
    m[idx] = _in_front_of_returns(orc, rig, 0, len(idx), 1.0)
    for alpha in (a_fit, a_over):
        want = _labels(rig, orc, m, alpha, f"alpha {alpha}")
        assert want[idx].sum() > 0
    _no_shape_failed(rig)


def test_uncertain_queue_past_capacity_within_a_drain(rig, orc):
    from tools.eps_sweep import boundary_points
    rng = np.random.default_rng(31)
    m = rig["pool"][:3 * TILE + 9].copy()
    n_edge = 3000
    m[TILE + 5:TILE + 5 + n_edge] = _to_global(orc, boundary_points(rng, n_edge, ALPHA, rig["vfov"], HFOV, 1.0e-6, 4.0, 30.0), rig["S"]["poses"][2], rig["L2B"])
    m[TILE + 3200:TILE + 3600] = _in_front_of_returns(orc, rig, 2, 400, 1.0)
    assert _uncertain_count(rig, m[TILE:2 * TILE], 2, ALPHA) > UQUEUE, "one tile holds more uncertain-pixel survivors than the shared queue"
    want = _labels(rig, orc, m, ALPHA, "uncertain queue past capacity")
    assert want[TILE:2 * TILE].sum() > 0
    _no_shape_failed(rig)
