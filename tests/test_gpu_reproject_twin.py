"""ltm_reproject_twin against two plain ltm_reproject calls, bitwise: points, offsets and sizes of both scan sets.

Two grids of one octree frame that share most of their points are projected with ONE exact-image launch over the shared points; the image's point
indices are replaced through two increasing tables and the points each map has alone are added with their own indices.  The cases
are the places where that can go wrong: a point of one map that wins or loses its pixel against a shared point, an exact tie between the two with the
indices either way round, equal maps, maps that share nothing, maps whose frames differ or are missing, an empty map, a signed zero, keyframe
sub-ranges and chunked images, and the A/B switch.  Clouds of ~4000 points, 5 keyframes, images of 150 x 1080 pixels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VFOV, HFOV, ALPHA, LEAF = 50.0, 360.0, 3.0, 0.05
N_KF = 5
# every cloud of one frame holds these: the bounding box, and with it the octree frame, is theirs whatever else the cloud holds
CORNERS = np.array([[-40.0, -40.0, -8.0, 0.0], [40.0, 40.0, 8.0, 0.0]], np.float32)


def _poses():
    p = np.tile(np.eye(4).reshape(1, 16), (N_KF, 1))
    for k in range(N_KF):      # keyframe 0 sits at the origin with an identity pose: what it sees is the map's own coordinates
        p[k, 3], p[k, 7], p[k, 11] = 0.7 * k, -0.3 * k, 0.05 * k
    return p


def _shell(n, seed, el_lo=3.0, el_hi=20.0):
    """n points at 10 .. 20 m around the origin, elevations of 3 .. 20 degrees above and below the horizon (the horizon itself stays free)"""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-np.pi, np.pi, n)
    el = np.deg2rad(rng.uniform(el_lo, el_hi, n)) * rng.choice([-1.0, 1.0], n)
    r = rng.uniform(10.0, 20.0, n)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.uniform(1.0, 100.0, n)], axis=1).astype(np.float32)


@pytest.fixture(scope="module")
def U():
    return np.concatenate([CORNERS, _shell(4000, 11)])


@pytest.fixture(scope="module")
def poses(gpu_ctx):
    return gpu_ctx.poses(_poses())


def _grid(ctx, *parts):
    return ctx.voxel_centroid(ctx.upload(np.concatenate(parts)), LEAF)


def _same(a, b, what):
    (ap, ao), (bp, bo) = a.download(), b.download()
    assert ao.shape == bo.shape and (ao == bo).all(), f"{what}: keyframe offsets differ"
    assert ap.shape == bp.shape, f"{what}: sizes differ, {ap.shape[0]} vs {bp.shape[0]}"
    assert (ap.view(np.uint32) == bp.view(np.uint32)).all(), f"{what}: points differ bitwise"
    return ap, ao


def _check(ctx, A, B, poses, kb=0, ke=None, expect=None):
    """twin == two plain calls; returns the twin's counters of this call and the plain result of A"""
    ctx.reproject_twin_stats(reset=True)
    ta, tb = ctx.reproject_twin(A, B, poses, ALPHA, kb, ke)
    st = ctx.reproject_twin_stats()
    pa, pb = ctx.reproject(A, poses, ALPHA, kb, ke), ctx.reproject(B, poses, ALPHA, kb, ke)
    ra = _same(ta, pa, "map A")
    _same(tb, pb, "map B")
    assert st["calls"] == 1
    if expect == "hit":
        assert st["hits"] == 1 and st["fallbacks"] == 0 and st["plain_passes"] == 0, st
    elif expect == "fallback":
        assert st["hits"] == 0 and st["fallbacks"] == 1 and st["plain_passes"] == 2, st
    return st, ra


def _rows_of(cloud_np, pts):
    """index in cloud_np of every row of pts (bitwise), -1 where it is missing"""
    key = {r.tobytes(): i for i, r in enumerate(np.ascontiguousarray(cloud_np, dtype=np.float32))}
    return np.array([key.get(np.ascontiguousarray(p, dtype=np.float32).tobytes(), -1) for p in pts])


def test_typical(gpu_ctx, poses, U):
    P1 = _shell(100, 12)
    P2 = P1[::3]
    A, B = _grid(gpu_ctx, U, P1), _grid(gpu_ctx, U, P2)
    st, _ = _check(gpu_ctx, A, B, poses, expect="hit")
    assert st["last_a"] == len(A) and st["last_b"] == len(B)
    assert st["last_shared"] >= min(len(A), len(B)) - 2 * len(P1)      # a point of P1 may fall into a voxel of U and move its centroid in one map only
    assert st["last_shared"] <= min(len(A), len(B)) and st["unordered"] == 0


@pytest.mark.parametrize("scale", [0.5, 1.25], ids=["only_point_wins", "only_point_loses"])
def test_only_point_on_a_shared_ray(gpu_ctx, orc, poses, U, scale):
    """points that only map A holds, on the rays of shared points as keyframe 0 sees them: nearer (they take the pixel in A's image and not in B's) and farther (they take none)"""
    rows, cols = orc.rimg_size(VFOV, HFOV, ALPHA)
    base = U[2:62]
    P1 = base.copy()
    P1[:, :3] *= np.float32(scale)
    px_u, r_u = orc.pixel(base[:, :3], VFOV, HFOV, rows, cols)
    px_p, r_p = orc.pixel(P1[:, :3], VFOV, HFOV, rows, cols)
    same_px = (px_u == px_p).all(axis=1)
    assert same_px.sum() >= 40 and ((r_p < r_u) if scale < 1.0 else (r_p > r_u))[same_px].all()
    A, B = _grid(gpu_ctx, U, P1), _grid(gpu_ctx, U)
    st, (pts, off) = _check(gpu_ctx, A, B, poses, expect="hit")
    assert st["last_shared"] == len(B) and st["last_a"] - st["last_shared"] == len(P1)
    kf0 = pts[off[0]:off[1]]
    seen = _rows_of(kf0, P1[same_px]) >= 0      # keyframe 0's pose is the identity: its reprojected points are map points
    assert seen.all() if scale < 1.0 else not seen.any()


@pytest.mark.parametrize("only_first", [True, False], ids=["only_index_below_shared", "only_index_above_shared"])
def test_tie_between_a_shared_and_an_only_point(gpu_ctx, orc, poses, U, only_first):
    """a shared point and a point of map A alone in ONE pixel of keyframe 0 with EQUAL range bits: the lower map index wins, as in the plain pass"""
    rows, cols = orc.rimg_size(VFOV, HFOV, ALPHA)

    def on_horizon(az_deg, r):
        a = np.deg2rad(az_deg)
        return np.array([r * np.cos(a), r * np.sin(a), 0.0], np.float32)
    # column 540 covers azimuths of -1/6 .. 1/6 degree; at 30 m the two points lie 7.9 cm apart in y: two voxels, ordered by y
    lo, hi = on_horizon(-0.05, 30.0), on_horizon(0.10, 30.0)
    (_, r_lo) = orc.pixel(lo.reshape(1, 3), VFOV, HFOV, rows, cols)
    found = None
    for step in range(-64, 65):      # move hi's x by ulps until its float range has lo's bits
        c = hi.copy()
        for _ in range(abs(step)):
            c[0] = np.nextafter(c[0], np.float32(np.inf if step > 0 else -np.inf), dtype=np.float32)
        if orc.pixel(c.reshape(1, 3), VFOV, HFOV, rows, cols)[1].view(np.uint32)[0] == r_lo.view(np.uint32)[0]:
            found = c
            break
    assert found is not None, "no coordinates with equal range bits within 64 ulps"
    hi = found
    px, rng = orc.pixel(np.stack([lo, hi]), VFOV, HFOV, rows, cols)
    assert (px[0] == px[1]).all() and rng.view(np.uint32)[0] == rng.view(np.uint32)[1]
    first, second = np.append(lo, 7.0).astype(np.float32), np.append(hi, 9.0).astype(np.float32)      # Morton order of the pair: the lower y first
    only, shared = (first, second) if only_first else (second, first)
    A, B = _grid(gpu_ctx, U, shared.reshape(1, 4), only.reshape(1, 4)), _grid(gpu_ctx, U, shared.reshape(1, 4))
    ia = _rows_of(A.download(), [only, shared])
    assert (ia >= 0).all() and (ia[0] < ia[1]) == only_first, "the pair is not in the index order this case is about"
    st, (pts, off) = _check(gpu_ctx, A, B, poses, expect="hit")
    assert st["last_a"] - st["last_shared"] == 1
    seen = _rows_of(pts[off[0]:off[1]], [only, shared]) >= 0
    assert seen.tolist() == [only_first, not only_first]      # one of them owns the pixel in A's image: the one with the lower index


def test_equal_maps_on_separate_handles(gpu_ctx, poses, U):
    A, B = _grid(gpu_ctx, U), _grid(gpu_ctx, U)
    st, _ = _check(gpu_ctx, A, B, poses, expect="hit")
    assert st["last_shared"] == len(A) == len(B)


def test_disjoint_maps_of_one_frame(gpu_ctx, poses):
    """the same bounding box from different corner points, nothing shared: two plain passes"""
    other = np.array([[-40.0, 40.0, -8.0, 0.0], [40.0, -40.0, 8.0, 0.0]], np.float32)
    A, B = _grid(gpu_ctx, CORNERS, _shell(3000, 21)), _grid(gpu_ctx, other, _shell(3000, 22))
    st, _ = _check(gpu_ctx, A, B, poses, expect="fallback")
    assert st["last_shared"] == 0 and st["last_a"] == len(A)


def test_frames_differ(gpu_ctx, poses, U):
    A, B = _grid(gpu_ctx, U, np.array([[90.0, 3.0, 1.0, 5.0]], np.float32)), _grid(gpu_ctx, U)
    _check(gpu_ctx, A, B, poses, expect="fallback")


def test_no_frame(gpu_ctx, poses, U):
    A = _grid(gpu_ctx, U)
    B = gpu_ctx.upload(A.download())      # the same points, but not out of a grid
    _check(gpu_ctx, A, B, poses, expect="fallback")
    _check(gpu_ctx, B, A, poses, expect="fallback")


def test_applicable_is_what_the_host_knows(gpu_ctx, U):
    """grids of one frame: yes (whatever they share); another frame, no frame, no points: no -- the two-lane hosts keep one map per lane then"""
    A, A2, E = _grid(gpu_ctx, U), _grid(gpu_ctx, U, _shell(50, 12)), gpu_ctx.upload(np.zeros((0, 4), np.float32))
    far = _grid(gpu_ctx, U, np.array([[90.0, 3.0, 1.0, 5.0]], np.float32))
    assert gpu_ctx.reproject_twin_applicable(A, A2) and gpu_ctx.reproject_twin_applicable(A, A.clone())
    assert not gpu_ctx.reproject_twin_applicable(A, far) and not gpu_ctx.reproject_twin_applicable(A, gpu_ctx.upload(A.download()))
    assert not gpu_ctx.reproject_twin_applicable(A, E) and not gpu_ctx.reproject_twin_applicable(E, A)


def test_one_map_empty(gpu_ctx, poses, U):
    A, E = _grid(gpu_ctx, U), gpu_ctx.upload(np.zeros((0, 4), np.float32))
    _check(gpu_ctx, A, E, poses, expect="fallback")
    _check(gpu_ctx, E, A, poses, expect="fallback")
    _check(gpu_ctx, E, E, poses, expect="fallback")


def test_signed_zero_is_not_shared(gpu_ctx, poses, U):
    """+0.0 in one map and -0.0 in the other at an otherwise equal point: two different points (a grid never writes -0.0, so it is put into B's memory)"""
    from ltmapper_amd.removerter import HipOps
    z = np.array([[12.0, 3.0, 0.0, 4.0]], np.float32)
    A, B = _grid(gpu_ctx, U, z), _grid(gpu_ctx, U, z)
    i = int(_rows_of(B.download(), z)[0])
    assert i > 0
    t = HipOps(gpu_ctx).cloud_to_tensor(B)
    t[i, 2] = -0.0
    import torch
    torch.cuda.synchronize()
    assert np.signbit(B.download()[i, 2]) and not np.signbit(A.download()[i, 2])
    st, _ = _check(gpu_ctx, A, B, poses, expect="hit")
    assert st["last_shared"] == len(A) - 1


@pytest.mark.parametrize("kb,ke", [(0, 0), (1, 2), (2, 5), (0, 5)])
def test_keyframe_sub_ranges(gpu_ctx, poses, U, kb, ke):
    A, B = _grid(gpu_ctx, U, _shell(100, 12)), _grid(gpu_ctx, U, _shell(30, 13))
    _check(gpu_ctx, A, B, poses, kb, ke, expect="hit" if ke > kb else "fallback")


def test_images_in_chunks(ltm, U):
    """a context that keeps two keyframes' images at a time: five keyframes are three chunks"""
    ctx = ltm.Context(vfov=VFOV, hfov=HFOV, device=0, max_kf_batch=2)
    try:
        p = ctx.poses(_poses())
        A, B = _grid(ctx, U, _shell(100, 12)), _grid(ctx, U, _shell(30, 13))
        _check(ctx, A, B, p, expect="hit")
        _check(ctx, A, B, p, 1, 4, expect="hit")
    finally:
        ctx.close()


def test_switch_off_is_two_plain_passes(ltm, U, monkeypatch):
    monkeypatch.setenv("LTM_REPROJECT_TWIN", "0")
    ctx = ltm.Context(vfov=VFOV, hfov=HFOV, device=0)
    monkeypatch.delenv("LTM_REPROJECT_TWIN")
    try:
        A, B = _grid(ctx, U, _shell(100, 12)), _grid(ctx, U)
        _check(ctx, A, B, ctx.poses(_poses()), expect="fallback")
    finally:
        ctx.close()


def test_threshold_of_the_shared_share(ltm, U, monkeypatch):
    """half of B is not in A: below the default threshold (two plain passes), above one of 0.3 (one projection of the shared half)"""
    extra = _shell(4000, 31)
    for thr, expect in ((None, "fallback"), ("0.3", "hit")):
        if thr is not None:
            monkeypatch.setenv("LTM_REPROJECT_TWIN_MIN_SHARED", thr)
        ctx = ltm.Context(vfov=VFOV, hfov=HFOV, device=0)
        monkeypatch.delenv("LTM_REPROJECT_TWIN_MIN_SHARED", raising=False)
        try:
            A, B = _grid(ctx, U), _grid(ctx, U, extra)
            st, _ = _check(ctx, A, B, ctx.poses(_poses()), expect=expect)
            assert 0.3 * len(B) < st["last_shared"] < 0.75 * len(B)
        finally:
            ctx.close()
