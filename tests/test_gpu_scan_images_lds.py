"""Scan range images built in LDS (k_scan_rimg_lds): image, per-keyframe maximum and bound image of ltm_debug_scan_images are compared bit for bit with a second
context that runs the fill / global-atomic / read-back kernels (LTM_SCAN_IMG_LDS=0), and the image also with the CPU oracle's scan2RangeImg.  A handful of
keyframes of at most a few thousand points: the edge cases are in where the points are put, not in how many there are."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VFOV, HFOV = 50.0, 360.0
LOT_ALPHAS = [float(np.float32(a)) for a in (2.5, 2.0, 1.5)] + [float(np.float32(0.95 * a)) for a in (2.5, 2.0, 1.5)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dirs(el_deg, az_deg, r):
    el, az = np.deg2rad(np.asarray(el_deg, dtype=np.float64)), np.deg2rad(np.asarray(az_deg, dtype=np.float64))
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), el.shape)
    p = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), np.zeros_like(el)], axis=1)
    return p.astype(np.float32)


def _other_ctx(ltm, vfov, lds):
    old = os.environ.get("LTM_SCAN_IMG_LDS")
    os.environ["LTM_SCAN_IMG_LDS"] = "1" if lds else "0"
    try:
        return ltm.Context(vfov=vfov, hfov=HFOV, device=0)
    finally:
        if old is None:
            del os.environ["LTM_SCAN_IMG_LDS"]
        else:
            os.environ["LTM_SCAN_IMG_LDS"] = old


@pytest.fixture(scope="module")
def ctx_pair(ltm, gpu_ctx):
    """(LDS path, the older kernels): the switch is read when a context is created"""
    a, b = _other_ctx(ltm, VFOV, True), _other_ctx(ltm, VFOV, False)
    yield a, b
    a.close(); b.close()


def _boundary_points(ltm, orc, alphas):
    """two points per band boundary and shape of the plan for `alphas`: the last row of band b and the first row of band b + 1, at their own azimuths"""
    shapes = [orc.rimg_size(VFOV, HFOV, a) for a in alphas]
    nb, row0, _, _ = ltm.scan_bands([s[0] for s in shapes], [s[1] for s in shapes])
    el, want = [], []
    for j, (rows, _) in enumerate(shapes):
        for b in range(1, nb):
            for row in (int(row0[b, j]) - 1, int(row0[b, j])):
                if 0 <= row < rows:
                    el.append(VFOV / 2 - VFOV * row / rows)      # the middle of the row
                    want.append((j, row))
    pts = _dirs(el, np.linspace(-179.0, 179.0, max(len(el), 1))[:len(el)], 7.0 + 0.001 * np.arange(len(el)))
    for (j, row), p in zip(want, pts):      # the construction must hit the rows it names, or the case tests nothing
        rc, _ = orc.pixel(p[None, :3], VFOV, HFOV, *shapes[j])
        assert rc[0, 0] == row, (j, row, rc)
    return pts, nb


@pytest.fixture(scope="module")
def scans(ltm, orc):
    """keyframes: 0 random with clamped and seam points, 1 empty, 2 one point, 3 the origin and a crowded pixel, 4 band boundaries, 5 random, 6 empty (last)"""
    rng = np.random.default_rng(77)

    def cloud(n):
        return _dirs(rng.uniform(-40.0, 40.0, n), rng.uniform(-180.0, 180.0, n), rng.uniform(0.5, 80.0, n))
    k0 = [cloud(3000),
          _dirs([25.0, 25.001, 31.0, 89.0, 90.0, -25.0, -25.001, -40.0, -90.0], np.linspace(-170, 170, 9), 12.0),      # first / last row, beyond +-vfov/2
          np.array([[-5.0, 0.0, 0.1, 0], [-5.0, -0.0, 0.1, 0], [-6.0, 1e-7, 0.2, 0], [-6.0, -1e-7, 0.2, 0],              # both sides of the +-180 degree seam
                    [5.0, 0.0, 0.3, 0], [5.0, -0.0, 0.3, 0], [0.0, 4.0, 0.0, 0], [0.0, -4.0, 0.0, 0]], dtype=np.float32)]
    crowd = _dirs(np.full(400, 3.3) + rng.uniform(-0.01, 0.01, 400), np.full(400, 41.7) + rng.uniform(-0.01, 0.01, 400), rng.choice([9.0, 9.5, 9.0, 11.25], 400))
    k3 = [np.zeros((3, 4), dtype=np.float32), crowd, cloud(500)]
    bpts = [_boundary_points(ltm, orc, al)[0] for al in ([2.5], [2.5, LOT_ALPHAS[3]], LOT_ALPHAS)]
    kfs = [np.concatenate(k0), np.zeros((0, 4), np.float32), _dirs([1.0], [2.0], [30.0]), np.concatenate(k3), np.concatenate(bpts + [cloud(200)]), cloud(2500),
           np.zeros((0, 4), np.float32)]
    off = np.concatenate([[0], np.cumsum([len(k) for k in kfs])]).astype(np.int64)
    return np.concatenate(kfs), off


def _compare(orc, ctxs, pts, off, alphas, thr, kb=0, ke=None, prepare=True, oracle=True, vfov=VFOV):
    """build on both contexts (fresh scan sets: nothing cached), read back every shape, compare"""
    ke = len(off) - 1 if ke is None else ke
    got = []
    for ctx in ctxs:
        ss = ctx.upload_scans(pts, off)
        if prepare:
            ctx.prepare_vote_images(ss, alphas, thr, kb, ke)
        got.append((ss, [ctx.debug_scan_images(ss, a, thr, kb, ke) for a in alphas]))
    for i, a in enumerate(alphas):
        (img, smax, qb), (img0, smax0, qb0) = got[0][1][i], got[1][1][i]
        assert (_bits(img) == _bits(img0)).all(), f"alpha {a}: image"
        assert (_bits(smax) == _bits(smax0)).all(), f"alpha {a}: maximum"
        assert (qb is None) == (qb0 is None) == (thr < 0)
        if qb is not None:
            assert (_bits(qb) == _bits(qb0)).all(), f"alpha {a}: bound image"
        if oracle:
            rows, cols = orc.rimg_size(vfov, HFOV, a)
            for k in range(kb, ke):
                want, _ = orc.range_image(pts[off[k]:off[k + 1]], vfov, HFOV, rows, cols, want_idx=False)
                assert (_bits(img[k - kb]) == _bits(want)).all(), f"alpha {a} keyframe {k}: image against the oracle"
                hit = want[want < 10000.0]
                assert smax[k - kb] == (hit.max() if hit.size else 0.0), f"alpha {a} keyframe {k}: maximum against the oracle's image"
    return got


@pytest.mark.parametrize("thr", [0.1, 0.0, -1.0])
@pytest.mark.parametrize("alphas", [[2.5], [0.5], [2.5, LOT_ALPHAS[3]], LOT_ALPHAS], ids=["1shape-banded", "1shape-1band", "2shapes", "6shapes"])
def test_prepared_images(ltm, orc, ctx_pair, scans, alphas, thr):
    pts, off = scans
    shapes = [orc.rimg_size(VFOV, HFOV, a) for a in alphas]
    nb = ltm.scan_bands([s[0] for s in shapes], [s[1] for s in shapes])[0]
    assert nb == 1 if alphas == [0.5] else nb >= 3
    _compare(orc, ctx_pair, pts, off, alphas, thr)


@pytest.mark.parametrize("thr", [0.1, -1.0])
def test_lazy_single_shape_and_sub_range(orc, ctx_pair, scans, thr):
    """no prepare call: the vote's own lazy build (scan_images), on a sub-range that starts behind keyframe 0 and ends on the empty keyframe"""
    pts, off = scans
    _compare(orc, ctx_pair, pts, off, [2.5], thr, kb=0, ke=len(off) - 1, prepare=False)
    _compare(orc, ctx_pair, pts, off, [2.0], thr, kb=1, ke=5, prepare=False)
    _compare(orc, ctx_pair, pts, off, LOT_ALPHAS, thr, kb=3, ke=7)
    _compare(orc, ctx_pair, pts, off, [2.5, 2.0], thr, kb=1, ke=2)      # the empty keyframe alone: every pixel written, maximum 0


def test_second_threshold_rebuilds_bound_image(orc, ctx_pair, scans):
    pts, off = scans
    got = _compare(orc, ctx_pair, pts, off, [2.5, 2.0], 0.1, oracle=False)
    for a in (2.5, 2.0):
        (i1, s1, q1), (i0, s0, q0) = (ctx.debug_scan_images(ss, a, 0.25) for ctx, (ss, _) in zip(ctx_pair, got))
        assert (_bits(i1) == _bits(i0)).all() and (_bits(s1) == _bits(s0)).all() and (_bits(q1) == _bits(q0)).all()
        first = got[0][1][[2.5, 2.0].index(a)]
        assert (_bits(i1) == _bits(first[0])).all(), "the image is the cached one"
        seen = first[0] < 10000.0
        far = first[2] > 0.0      # (the returns at range 0 have no bound to lower)
        assert far.any() and (q1[far] < first[2][far]).all() and (q1[~far] == 0).all(), "a larger threshold lowers the bound wherever there is one"
        assert (first[2][~seen] == 0).all()
        # and back: the threshold of the prepare call again
        q_again = ctx_pair[0].debug_scan_images(got[0][0], a, 0.1)[2]
        assert (_bits(q_again) == _bits(first[2])).all()


def test_dense_scans_beyond_the_one_pass_gate(orc, ctx_pair):
    """more than scan_multi_max_density (2.5) points per pixel of the smallest shape: with the older kernels the prepare call leaves the images to the votes, one shape at a time; the LDS path builds them in its one pass"""
    rng = np.random.default_rng(5)
    alphas = [0.3, 0.2]                                          # 15 x 108 and 10 x 72 = 720 pixels
    kfs = [_dirs(rng.uniform(-30, 30, n), rng.uniform(-180, 180, n), rng.uniform(1, 50, n)) for n in (3000, 2600, 2900)]
    off = np.concatenate([[0], np.cumsum([len(k) for k in kfs])]).astype(np.int64)
    assert (np.diff(off).mean() / 720) > 2.5
    _compare(orc, ctx_pair, np.concatenate(kfs), off, alphas, 0.1)


def test_shape_the_plan_rejects_takes_the_older_kernels(ltm, orc):
    """one row wider than a band's budget: a 1 degree field of view at some 109 pixels per degree (109 x 39240 for a budget of 155136 bytes)"""
    budget = ltm.scan_bands([1], [1])[3]
    vfov, alpha = 1.0, float(budget // 4 // 360 + 2)
    rows, cols = orc.rimg_size(vfov, HFOV, alpha)
    assert cols * 4 > budget and ltm.scan_bands([rows], [cols])[0] == 0
    rng = np.random.default_rng(9)
    kfs = [_dirs(rng.uniform(-0.7, 0.7, n), rng.uniform(-180, 180, n), rng.uniform(1, 50, n)) for n in (1500, 0, 1)]
    off = np.concatenate([[0], np.cumsum([len(k) for k in kfs])]).astype(np.int64)
    ctxs = _other_ctx(ltm, vfov, True), _other_ctx(ltm, vfov, False)
    try:
        _compare(orc, ctxs, np.concatenate(kfs), off, [alpha], 0.1, vfov=vfov)
        _compare(orc, ctxs, np.concatenate(kfs), off, [alpha], -1.0, prepare=False, oracle=False, vfov=vfov)
    finally:
        for c in ctxs:
            c.close()


def _same(got, want, what):
    for x, y, name in zip(got, want, ("image", "maximum", "bound image")):
        assert (x is None) == (y is None), f"{what}: {name}"
        if x is not None:
            assert x.shape == y.shape and (_bits(x) == _bits(y)).all(), f"{what}: {name}"


TEN_ALPHAS = [float(np.float32(0.1 * i)) for i in range(2, 12)]      # 0.2 .. 1.1


@pytest.mark.parametrize("thr", [0.1, -1.0])
def test_ten_shapes_are_two_groups_of_one_prepare_call(ltm, orc, ctx_pair, scans, thr):
    """more shapes than one pass takes (kMaxScanShapes = 8): 10 x 72 up to 55 x 396, all different, built as a group of eight and a group of two"""
    pts, off = scans
    shapes = [orc.rimg_size(VFOV, HFOV, a) for a in TEN_ALPHAS]
    assert shapes == [(5 * i, 36 * i) for i in range(2, 12)]
    assert ltm.scan_bands([s[0] for s in shapes[:9]], [s[1] for s in shapes[:9]])[0] == 0, "nine shapes are not one pass"
    assert ltm.scan_bands([s[0] for s in shapes[:8]], [s[1] for s in shapes[:8]])[0] >= 1 and ltm.scan_bands([s[0] for s in shapes[8:]], [s[1] for s in shapes[8:]])[0] >= 1
    _compare(orc, ctx_pair, pts, off, TEN_ALPHAS, thr)


def test_repeated_alpha_and_two_orders_of_arrival(orc, ctx_pair, scans):
    """what a scan set already holds is not built again and not disturbed, whichever way it got there: a prepare call for one of two shapes or a vote's lazy build
    (without a threshold: its bound image is made at the read-back), and an alpha named twice in one list"""
    pts, off = scans
    fresh = _compare(orc, ctx_pair, pts, off, [2.5, 2.0], 0.1)
    for ctx, (_, want) in zip(ctx_pair, fresh):
        a = ctx.upload_scans(pts, off)
        ctx.prepare_vote_images(a, [2.5], 0.1)
        first = ctx.debug_scan_images(a, 2.5, 0.1)
        ctx.prepare_vote_images(a, [2.5, 2.0, 2.5], 0.1)
        b = ctx.upload_scans(pts, off)
        lazy = ctx.debug_scan_images(b, 2.0)
        ctx.prepare_vote_images(b, [2.5, 2.0], 0.1)
        _same(first, want[0], "prepared alone")
        _same(lazy, (want[1][0], want[1][1], None), "lazy, no threshold")
        for ss, what in ((a, "prepare, then prepare"), (b, "lazy, then prepare")):
            for i, alpha in enumerate((2.5, 2.0)):
                _same(ctx.debug_scan_images(ss, alpha, 0.1), want[i], f"{what}: alpha {alpha}")


def test_clear_caches_between_two_read_backs(orc, ctx_pair, scans):
    pts, off = scans
    fresh = _compare(orc, ctx_pair, pts, off, [2.0], 0.1, kb=1, ke=6)
    for ctx, (ss, want) in zip(ctx_pair, fresh):
        ctx.clear_caches()
        _same(ctx.debug_scan_images(ss, 2.0, 0.1, 1, 6), want[0], "rebuilt after clear_caches")
        ctx.clear_caches()
        _same(ctx.debug_scan_images(ss, 2.0, -1.0, 1, 6), (want[0][0], want[0][1], None), "rebuilt without a threshold")
