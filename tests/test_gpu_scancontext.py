"""Scan Context on the device (include/ltm.h, "scan context") against the numpy restatement of the reference's lines (tools/sc_numpy.py, which
shares nothing with the library): descriptors bit for bit, keys, pair distance and shift, loop detection, plumbing.

Inputs are built so that the expected result does not hinge on the last bit of an atan: generated points lie in the interior of their bin (ring and
sector fraction in [0.1, 0.9] of the cell), the known-answer points have exact arithmetic, and the realistic scans are checked against a
[lower, upper] pair of descriptors that brackets every point within 1e-5 (relative) of a bin edge.

The restatement is not in this file: tools/sc_numpy.py holds it, because tools/bench_scancontext.py compares against the same text.  It is written
from the reference's lines alone and imports nothing of the library.  An edit to it changes what these tests expect, so it is reviewed like a test."""
import ctypes as C

import numpy as np
import pytest

from sc_cases import away_from, place, polar_points, rotated, session_scans      # the generators, shared with the case builder
from tools import sc_numpy as ref

pytestmark = pytest.mark.gpu

KF_SIZES = (0, 1, 63, 64, 65, 5000)


def edge_case_scans(seed, p):
    """one scan set: keyframes of KF_SIZES points (the 5000-point one with the hard bins), then the two known-answer keyframes"""
    rng = np.random.default_rng(seed)
    R, S = p["num_ring"], p["num_sector"]
    # reserved bins of the large keyframe (distinct where the shape allows it): contention, only value -1000, only values <= -1000, only a negative value
    res = [(R // 2, S // 3), (R - 1, S - 1), (0, S // 2), (R // 3, 0)]
    kfs = []
    for n in KF_SIZES:
        if n < 5000:
            kfs.append(polar_points(rng, n, p))
            continue
        one = lambda b, k: (np.full(k, b[0]), np.full(k, b[1]))
        excl = res if R * S > 8 else ()
        parts = [polar_points(rng, n - 420, p, exclude=excl),
                 place(rng, *one(res[0], 400), p, rng.uniform(-1.0, 6.0, 400)),          # several hundred points in one bin
                 place(rng, *one(res[1], 1), p, [-1002.0]),                            # z + 2 == -1000 exactly
                 place(rng, *one(res[2], 3), p, [-1500.0, -2000.0, -1002.0]),          # every value <= -1000
                 place(rng, *one(res[3], 2), p, [-2.75, -3.5]),                        # negative heights win against -1000
                 place(rng, *away_from(rng.integers(0, R, 4), rng.integers(0, S, 4), S, excl), p, [-2.0] * 4),   # value exactly 0, never in a reserved bin
                 ]
        far = place(rng, rng.integers(0, R, 6), rng.integers(0, S, 6), p, rng.uniform(0, 5, 6))
        far[:, :2] *= np.float32(1.0) + (np.float32(p["max_radius"]) * rng.uniform(1.01, 1.5, 6).astype(np.float32) /
                                         np.hypot(far[:, 0], far[:, 1]))[:, None]      # beyond max_radius
        bad = polar_points(rng, 4, p)
        bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0] = np.nan, np.inf, np.nan, -np.inf
        bad[:, 2] = np.where(np.isfinite(bad[:, 2]), 500.0, bad[:, 2])                  # would dominate any bin if it were not skipped
        allp = np.concatenate(parts + [far, bad])
        kfs.append(allp[rng.permutation(len(allp))])
    over = np.nextafter(np.float32(p["max_radius"]), np.float32(np.inf))
    kfs.append(np.array([[4, 0, 1, 0], [-4, 0, 1.5, 0], [0, 4, 2, 0], [0, -4, 2.5, 0], [p["max_radius"], 0, 3, 0], [over, 0, 50, 0], [-0.0, 5, 4, 0]], np.float32))
    kfs.append(np.array([[0, 0, 7, 0]], np.float32))
    off = np.concatenate([[0], np.cumsum([len(k) for k in kfs])]).astype(np.uint64)
    return np.concatenate(kfs), off


@pytest.fixture(scope="module")
def lot():
    """40 database descriptors (restatement), 40 copies rotated by whole sectors with height noise, 2 unrelated ones"""
    p = ref.params()
    rng = np.random.default_rng(20240611)
    base = ref.descriptors(*session_scans(11, 40, 600, p), p)
    rots = np.array([(0, 1, 7, 30, 59)[k % 5] for k in range(40)])
    copies = np.stack([rotated(rng, base[k], rots[k]) for k in range(40)])
    other = ref.descriptors(*session_scans(12, 2, 600, p), p)
    return dict(p=p, base=base, copies=copies, rots=rots, other=other)


# ------------------------------------------------------------------ 1 + 2: descriptors bit for bit, keys
@pytest.mark.parametrize("shape", [(20, 60), (1, 1), (64, 256)])
def test_descriptors_bitwise_and_keys(gpu_ctx, shape):
    p = ref.params(num_ring=shape[0], num_sector=shape[1])
    scans, off = edge_case_scans(5, p)
    want = ref.descriptors(scans, off, p)
    g = gpu_ctx.upload_scans(scans, off)
    with gpu_ctx.scan_contexts(g, num_ring=shape[0], num_sector=shape[1]) as sc:
        assert sc.info() == (len(off) - 1, shape[0], shape[1])
        desc, rk, sk = sc.download()
    g.free()
    bad = np.argwhere(desc.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, f"{len(bad)} bins differ, first (kf, ring, sector) {bad[:5].tolist()}: {[(desc[tuple(b)], want[tuple(b)]) for b in bad[:5]]}"
    assert (desc[0] == 0).all()                                          # the empty keyframe
    if shape == (20, 60):                                               # known answers, exact arithmetic
        a = np.zeros((20, 60))
        a[0, 0], a[0, 29], a[0, 14], a[0, 44], a[19, 0], a[1, 0] = 3.0, 3.5, 4.0, 4.5, 5.0, 6.0
        assert (desc[6] == a).all(), np.argwhere(desc[6] != a)
        b = np.zeros((20, 60))
        b[0, 0] = 9.0                                                   # (0, 0) lands in ring 1, sector 1
        assert (desc[7] == b).all()
        big = desc[5]
        assert big[19, 59] == 0.0 and big[0, 30] == 0.0                 # only -1000 / only <= -1000
        assert big[6, 0] == -0.75                                       # negative heights win against the initial -1000
        assert big.max() < 100.0                                        # the non-finite points (z = 500) were skipped
    # keys: ring keys within one float ulp, sector keys within 1e-12 (Eigen's summation order is not known)
    want_rk = np.stack([ref.ring_key(d) for d in want])
    want_sk = np.stack([ref.sector_key(d) for d in want])
    ulp = np.spacing(np.abs(want_rk))
    print("ring key max |diff| / ulp", float((np.abs(rk.astype(np.float64) - want_rk) / ulp).max()), "sector key max |diff|", float(np.abs(sk - want_sk).max()))
    assert (np.abs(rk.astype(np.float64) - want_rk.astype(np.float64)) <= ulp).all()
    assert np.abs(sk - want_sk).max() <= 1e-12


# ------------------------------------------------------------------ 3: realistic scans
def bracket(pts, p, tol=1e-5):
    """(lower, upper): descriptors without the points within tol (relative) of a bin edge / with them in both neighbouring bins"""
    R, S = p["num_ring"], p["num_sector"]
    fin = np.isfinite(pts[:, :3]).all(axis=1)
    pts = pts[fin]
    r, theta = ref.polar(pts)
    vr, vs = r.astype(np.float64) / p["max_radius"] * R, theta.astype(np.float64) / 360.0 * S
    h = ref.heights(pts, p)
    near = lambda v: np.abs(v - np.rint(v)) <= tol * np.maximum(np.abs(v), 1.0)
    amb_r, amb_s = near(vr), near(vs)
    amb_out = np.abs(r.astype(np.float64) - p["max_radius"]) <= tol * p["max_radius"]
    inside = ~(r.astype(np.float64) > p["max_radius"])
    cell = lambda v, n: np.clip(np.ceil(v), 1, n).astype(np.int64)
    lo, up = np.full((R, S), -1000.0), np.full((R, S), -1000.0)
    sure = inside & ~amb_r & ~amb_s & ~amb_out
    np.maximum.at(lo, (cell(vr[sure], R) - 1, cell(vs[sure], S) - 1), h[sure])
    np.maximum.at(up, (cell(vr[sure], R) - 1, cell(vs[sure], S) - 1), h[sure])
    for i in np.nonzero((inside | amb_out) & ~sure)[0]:
        rings = {int(np.clip(np.rint(vr[i]) + d, 1, R)) for d in (0, 1)} if amb_r[i] or amb_out[i] else {int(cell(vr[i], R))}
        secs = {int(np.clip(np.rint(vs[i]) + d, 1, S)) for d in (0, 1)} if amb_s[i] else {int(cell(vs[i], S))}
        if amb_s[i] and (np.rint(vs[i]) <= 0 or np.rint(vs[i]) >= S):
            secs |= {1, S}                                              # the seam at 0 / 360 degrees
        for a in rings:
            for b in secs:
                up[a - 1, b - 1] = max(up[a - 1, b - 1], h[i])
    lo[lo == -1000.0] = 0.0
    up[up == -1000.0] = 0.0
    return np.minimum(lo, up), np.maximum(lo, up)


def test_realistic_scans_within_the_edge_bracket(gpu_ctx, small_pair):
    p = ref.params()
    sess = small_pair[0]
    scans, off = sess["scans"], sess["offsets"]
    g = gpu_ctx.upload_scans(scans, off)
    with gpu_ctx.scan_contexts(g) as sc:
        desc, _, _ = sc.download()
    g.free()
    loose = 0
    for k in range(len(off) - 1):
        lo, up = bracket(scans[int(off[k]):int(off[k + 1])], p)
        loose += int((lo != up).sum())
        bad = np.argwhere((desc[k] < lo) | (desc[k] > up))
        assert len(bad) == 0, f"keyframe {k}: bins outside [lower, upper] at {bad[:5].tolist()}"
        assert np.count_nonzero(desc[k]) > 100                          # the scans do fill the descriptor
    frac = loose / desc.size
    print("bins with lower != upper:", loose, "of", desc.size)
    assert frac <= 0.005, f"the inputs leave {frac:.3%} of the bins undecided"


# ------------------------------------------------------------------ 4: pair distance
def pair_list():
    rng = np.random.default_rng(3)
    return np.concatenate([np.stack([np.arange(40), np.arange(40)], axis=1), rng.integers(0, 40, (160, 2))]).astype(np.int32)


@pytest.mark.parametrize("ratio", [0.1, 1.0])
def test_pair_distance_and_shift(gpu_ctx, lot, ratio):
    pairs = pair_list()
    want = [ref.distance(lot["copies"][i], lot["base"][j], ratio, details=True) for i, j in pairs]
    for (d, s, norms, dists), (i, j) in zip(want, pairs):                 # condition on the inputs: nothing hinges on a near-tie
        assert norms[1] - norms[0] > 1e-9, (i, j)
        assert dists[1] - dists[0] > 1e-9, (i, j)
    with gpu_ctx.scan_contexts_from(lot["copies"]) as a, gpu_ctx.scan_contexts_from(lot["base"]) as b:
        dist, shift = a.distance(b, pairs, search_ratio=ratio)
    wd, ws = np.array([w[0] for w in want]), np.array([w[1] for w in want])
    print("ratio", ratio, "max |dist - restatement|", float(np.abs(dist - wd).max()))
    assert (shift == ws).all(), np.nonzero(shift != ws)[0][:5]
    assert np.abs(dist - wd).max() <= 1e-12
    assert (shift[:40] == lot["rots"]).all() and (dist[:40] < 0.01).all()      # the copies are found at their rotation


def test_pair_distance_exact_ties(gpu_ctx):
    col = np.arange(1.0, 21.0)
    same = np.repeat(col[:, None], 60, axis=1)                              # every column identical: every shift ties, the first (0) wins
    descs = np.stack([same, same.copy(), np.zeros((20, 60))])
    with gpu_ctx.scan_contexts_from(descs) as sc:
        dist, shift = sc.distance(sc, [[0, 1], [0, 2], [2, 0], [2, 2]], search_ratio=1.0)
        d01, s01 = sc.distance(sc, [[0, 1]])
    assert shift.tolist() == [0, 0, 0, 0] and s01.tolist() == [0]
    assert abs(dist[0]) <= 1e-12 and abs(d01[0]) <= 1e-12
    assert (dist[1:] == 10000000.0).all()                                   # an all-zero descriptor: every distance NaN


# ------------------------------------------------------------------ 5: detect
def queries_of(lot):
    rng = np.random.default_rng(8)
    src = np.array([0, 3, 7, 8, 12, 16, 21, 25, 29, 33, 36, 39])
    rots = np.array([(0, 1, 7, 30, 59, 2)[k % 6] for k in range(12)])
    q = np.concatenate([np.stack([rotated(rng, lot["base"][s], r) for s, r in zip(src, rots)]), lot["other"]])
    return q, src, rots


def check_detect(got, want):
    for k in ("loop_id", "nn_idx", "nn_align"):
        assert (got[k] == want[k]).all(), (k, got[k], want[k])
    assert np.abs(got["min_dist"] - want["min_dist"]).max() <= 1e-12
    assert (got["yaw_diff_rad"].view(np.uint32) == want["yaw_diff_rad"].view(np.uint32)).all()


def test_detect_default_and_exhaustive(gpu_ctx, lot):
    q, src, rots = queries_of(lot)
    with gpu_ctx.scan_contexts_from(lot["base"]) as db, gpu_ctx.scan_contexts_from(q) as qs:
        got = db.detect(qs)
        full = db.detect(qs, num_candidates=0, search_ratio=1.0)
    check_detect(got, ref.detect(lot["base"], q, lot["p"]))
    check_detect(full, ref.detect(lot["base"], q, ref.params(num_candidates=0, search_ratio=1.0)))
    for res in (got, full):
        assert (res["loop_id"][:12] == src).all() and (res["nn_align"][:12] == rots).all()      # the copies find their originals at the rotation
        assert (res["loop_id"][12:] == -1).all()                                                 # the unrelated ones find nothing
    assert (full["min_dist"] <= got["min_dist"] + 1e-12).all()


def test_detect_small_and_empty_database(gpu_ctx, lot):
    q, _, _ = queries_of(lot)
    with gpu_ctx.scan_contexts_from(lot["base"][:2]) as db, gpu_ctx.scan_contexts_from(q) as qs:
        check_detect(db.detect(qs), ref.detect(lot["base"][:2], q, lot["p"]))                    # num_candidates 3 > database of 2
    with gpu_ctx.scan_contexts_from(np.zeros((0, 20, 60))) as db, gpu_ctx.scan_contexts_from(q) as qs:
        got = db.detect(qs)
    assert (got["loop_id"] == -1).all() and (got["nn_idx"] == 0).all() and (got["min_dist"] == 10000000.0).all()
    assert (got["nn_align"] == 0).all() and (got["yaw_diff_rad"] == 0).all()


# ------------------------------------------------------------------ 6: plumbing
def test_plumbing(gpu_ctx, ltm):
    before = gpu_ctx.pool_live()
    p = ref.params()
    scans, off = edge_case_scans(6, p)
    g = gpu_ctx.upload_scans(scans, off)
    sc = gpu_ctx.scan_contexts(g, kf_begin=2, kf_end=7)
    assert len(sc) == 5
    desc, rk, sk = sc.download()
    assert (desc.view(np.uint64) == ref.descriptors(scans, off, p)[2:7].view(np.uint64)).all()      # the keyframe range is honoured
    again = gpu_ctx.scan_contexts_from(desc)
    d2, rk2, sk2 = again.download()
    assert (d2.view(np.uint64) == desc.view(np.uint64)).all() and (rk2.view(np.uint32) == rk.view(np.uint32)).all()
    assert (sk2.view(np.uint64) == sk.view(np.uint64)).all()
    lib = gpu_ctx.lib
    # a lane is another context: refused
    lane = gpu_ctx.lane()
    n = C.c_size_t()
    assert lib.ltm_sc_info(lane.h, sc.h, C.byref(n), None, None) == -1
    assert lib.ltm_sc_free(lane.h, sc.h) == -1
    theirs = lane.scan_contexts_from(desc)
    with pytest.raises(ltm.LtmError) as e:
        sc.distance(theirs, [[0, 0]])
    assert e.value.code == -1
    theirs.close()
    lane.close()
    # mismatched shapes, out-of-domain parameters, bad indices
    other = gpu_ctx.scan_contexts_from(np.zeros((2, 10, 60)), num_ring=10)
    for call in (lambda: sc.distance(other, [[0, 0]]), lambda: sc.detect(other), lambda: other.detect(sc), lambda: sc.distance(again, [[0, 5]]),
                 lambda: sc.distance(again, [[-1, 0]]), lambda: sc.distance(again, [[0, 0]], num_sector=30),
                 lambda: gpu_ctx.scan_contexts(g, num_ring=0), lambda: gpu_ctx.scan_contexts(g, max_radius=0.0),
                 lambda: gpu_ctx.scan_contexts(g, kf_begin=3, kf_end=2), lambda: gpu_ctx.scan_contexts(g, kf_end=len(off)),
                 lambda: sc.detect(again, search_ratio=-0.5)):
        with pytest.raises(ltm.LtmError) as e:
            call()
        assert e.value.code == -1
    many = gpu_ctx.scan_contexts_from(np.zeros((66, 20, 60)))                  # num_candidates > 64 and below the database size
    tiny = gpu_ctx.scan_contexts_from(np.zeros((46341, 1, 1)), num_ring=1, num_sector=1)      # 46341^2 >= 2^31 (query, database) pairs in one call
    for call in (lambda: gpu_ctx.scan_contexts(g, num_ring=65), lambda: gpu_ctx.scan_contexts(g, num_sector=257),
                 lambda: many.detect(again, num_candidates=65), lambda: tiny.detect(tiny, num_ring=1, num_sector=1)):
        with pytest.raises(ltm.LtmError) as e:
            call()
        assert e.value.code == -4
    assert (many.detect(again, num_candidates=66)["loop_id"] == -1).all()     # reaching the database size is the exhaustive mode: accepted
    many.close()
    tiny.close()
    h = sc.h
    for s in (sc, again, other):
        s.close()
    assert lib.ltm_sc_info(gpu_ctx.h, h, C.byref(n), None, None) == -1        # a freed handle is refused, not dereferenced
    g.free()
    assert gpu_ctx.pool_live() == before
