"""The search index at the seams of its own kernels (ltm_search_walk.h, ltm_k_search.hip), on the fixtures of tests/search_cases.py: every tree shape around
a leaf and a power-of-two leaf count, every list form of the kNN kernels full and part full, every state of the seed, exact ties, radii on both sides of a
tie and at the ends of the float range, clouds whose distances underflow, are denormal or overflow, and all of it again through ONE batched build.  Every
comparison is exact -- indices equal, distances equal as bit patterns -- against the numpy brute force in the library's documented float arithmetic
(tests/test_search_cases_cpu.py shows on the host that the cases reach what they are named for)."""
import numpy as np
import pytest

import search_cases as sc

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_pairs(name, q_rows, idx, d2):
    """a returned distance is the float recomputation of its pair, bit for bit, and within 1e-6 d + 3 * 2^-149 of the pair's distance d in double (five
    roundings of 2^-24 and three squares that may each lose half a denormal spacing); where d is beyond the float range the float is +inf"""
    c = sc.CASES[name]
    if not len(idx):
        return
    t = c.target[idx, :3]
    q = c.queries[q_rows, :3]
    with np.errstate(all="ignore"):
        dx, dy, dz = q[:, 0] - t[:, 0], q[:, 1] - t[:, 1], q[:, 2] - t[:, 2]
        re = (dx * dx + dy * dy) + dz * dz
    assert (_bits(re) == _bits(d2)).all(), f"{name}: a distance is not the float recomputation of its pair"
    dd = ((q.astype(np.float64) - t.astype(np.float64)) ** 2).sum(axis=1)
    big = dd > FLT_MAX
    assert np.isinf(d2[big]).all()
    err = np.abs(d2[~big].astype(np.float64) - dd[~big])
    assert (err <= 1e-6 * dd[~big] + 3 * sc.DENORM_MIN).all(), f"{name}: a distance is {err.max()} from its double-precision value"


def _check_knn(s, qc, name, k):
    idx, d2 = s.knn(qc, k)
    wi, wd = sc.want_knn(name, k)
    assert idx.shape == wi.shape and d2.shape == wd.shape
    bad = np.flatnonzero((idx != wi).any(axis=1))
    assert bad.size == 0, f"{name} k={k}: {bad.size} rows differ from the brute force, first {bad[:3]}: {idx[bad[:2]]} vs {wi[bad[:2]]}"
    assert (_bits(d2) == _bits(wd)).all(), f"{name} k={k}: distances differ bitwise"
    rows, cols = np.nonzero(idx >= 0)
    _check_pairs(name, rows, idx[rows, cols], d2[rows, cols])
    return idx, d2


def _check_radius(s, qc, name, r, max_nn):
    off, idx, d2 = s.radius(qc, float(r), max_nn)
    woff, wi, wd = sc.want_radius(name, r, max_nn)
    assert off.shape == woff.shape and off[0] == 0 and off[-1] == len(idx) == len(d2)
    bad = np.flatnonzero(np.diff(off.astype(np.int64)) != np.diff(woff.astype(np.int64)))
    assert bad.size == 0, f"{name} r={r!r} max_nn={max_nn}: {bad.size} rows differ in length from the brute force, first {bad[:3]}"
    assert (idx == wi).all(), f"{name} r={r!r} max_nn={max_nn}: indices differ"
    assert (_bits(d2) == _bits(wd)).all(), f"{name} r={r!r} max_nn={max_nn}: distances differ bitwise"
    _check_pairs(name, np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64))), idx, d2)
    return off, idx, d2


def _check_index(ctx, s, name, ks):
    c = sc.CASES[name]
    fin = int(sc.finite_rows(c.target).sum())
    assert s.info() == (len(c.target), fin)
    qc = ctx.upload(c.queries)
    try:
        for k in ks:
            _check_knn(s, qc, name, k)
        for r, max_nn in sc.radius_list(name):
            _check_radius(s, qc, name, r, max_nn)
    finally:
        qc.free()


@pytest.mark.parametrize("n", sc.SHAPE_SIZES)
def test_shape_against_brute_force(gpu_ctx, n):
    name = f"n{n}"
    assert {m for _, m in sc.radius_list(name)} >= {0, 1, 5}
    with gpu_ctx.search_index(sc.SHAPES[name].target) as s:
        assert s.info() == (n + 3, n)
        _check_index(gpu_ctx, s, name, sc.K_ALL)
        # r = +inf: every finite query has all Mf finite points in its row
        off, _, _ = s.radius(sc.SHAPES[name].queries, float("inf"))
        assert (np.diff(off.astype(np.int64)) == np.where(sc.brute(name)[2], n, 0)).all()


@pytest.mark.parametrize("name", list(sc.TIES))
def test_ties_against_brute_force(gpu_ctx, name):
    with gpu_ctx.search_index(sc.TIES[name].target) as s:
        _check_index(gpu_ctx, s, name, sc.K_ALL)
        if name == "lattice_x3":      # r2 = (float)((double)r * r): r = -1 is r = 1
            a, b = s.radius(sc.TIES[name].queries, -1.0), s.radius(sc.TIES[name].queries, 1.0)
            assert len(a[1]) and all((x == y).all() for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(sc.RANGE))
def test_float_range_against_brute_force(gpu_ctx, name):
    c = sc.RANGE[name]
    with gpu_ctx.search_index(c.target) as s:
        _check_index(gpu_ctx, s, name, sc.K_ALL)
        if name == "overflow":
            huge = np.flatnonzero(np.abs(c.queries[:, 0]) > 1e38)
            idx, d2 = s.knn(c.queries, 16)
            far = np.isinf(d2[huge])
            # the rows go on past the finite distances with the +inf ones in index order (not with the -1 of a row that ran out of points)
            assert len(huge) == 3 and far.any(axis=1).all() and (idx[huge] >= 0).all()
            for row, f in zip(idx[huge], far):
                assert (np.diff(row[f]) > 0).all() and not f[0] and f[np.argmax(f):].all()
            # r = +inf is d2 < +inf: the +inf entries are outside
            off, ri, rd = s.radius(c.queries, float("inf"))
            assert np.isfinite(rd).all() and (np.diff(off.astype(np.int64))[huge] < 200).all() and (np.diff(off.astype(np.int64))[huge] >= 1).all()


def test_one_batched_build_of_every_case_answers_like_brute_force(gpu_ctx):
    """every case's target as one keyframe of one scan set, an empty keyframe and one without a finite point in between, one search_index_batch: every index
    answers as the brute force does, hence as its single build.  The segmented sort of the batched build is not stable: coincident_100, two_values_140
    and collapse (few distinct codes) are where a dependence on the order of equal codes would show."""
    names = list(sc.CASES)
    clouds, kf_case = [], []
    nanc = np.full((4, 4), np.nan, np.float32)
    nanc[1, :] = [0.0, np.inf, 0.0, 0.0]
    for i, name in enumerate(names):
        if i == 3:
            clouds.append(np.zeros((0, 4), np.float32)); kf_case.append("empty")
        if i == 17:
            clouds.append(nanc); kf_case.append("non-finite")
        clouds.append(sc.CASES[name].target); kf_case.append(name)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.uint64)
    some_q = gpu_ctx.upload(sc.CASES["n33"].queries)
    live = gpu_ctx.pool_live()
    scans = gpu_ctx.upload_scans(np.concatenate(clouds), off)
    batch = gpu_ctx.search_index_batch(scans)
    assert len(batch) == len(clouds)
    kb, ke = 2, 9      # around the empty keyframe, across a leaf boundary of sizes
    part = gpu_ctx.search_index_batch(scans, kb, ke)
    assert len(part) == ke - kb
    for group, first in ((batch, 0), (part, kb)):
        for j, s in enumerate(group):
            name = kf_case[first + j]
            if name == "empty" or name == "non-finite":
                assert s.info() == (0 if name == "empty" else 4, 0)
                idx, d2 = s.knn(some_q, 4)
                assert (idx == -1).all() and np.isinf(d2).all() and s.radius(some_q, float("inf"))[0][-1] == 0
            else:
                _check_index(gpu_ctx, s, name, sc.K_FEW)
    for s in batch[::-1] + part:
        s.close()
    scans.free()
    assert gpu_ctx.pool_live() == live, "the blocks of both batches must be back in the pool"
    some_q.free()
