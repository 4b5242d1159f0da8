"""The device search index (ltm_search_build / ltm_knn_search / ltm_radius_search): exact k-NN and radius results checked against an independent
numpy brute force (same float arithmetic, ties by index) and against scipy's cKDTree, on random clouds, on adversarial layouts and on the
synthetic lot; tied bit for bit to the coexist / near decisions the product path (ltm_knn_partition, ltm_knn_split_cloud) makes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 16, 17, 64)


def _d2(q, t):
    """FLANN's L2_Simple in float32, ((dx*dx)+dy*dy)+dz*dz, for every (query, target) pair: [nq, nt]"""
    q = np.asarray(q, np.float32)
    t = np.asarray(t, np.float32)
    dx = q[:, None, 0] - t[None, :, 0]
    dy = q[:, None, 1] - t[None, :, 1]
    dz = q[:, None, 2] - t[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def _pair_d2(q, t, idx):
    """the same arithmetic for given pairs: q [n, 3+], t [m, 3+], idx [n, k] (>= 0)"""
    tt = np.asarray(t, np.float32)[idx]
    qq = np.asarray(q, np.float32)[:, None, :]
    dx, dy, dz = qq[..., 0] - tt[..., 0], qq[..., 1] - tt[..., 1], qq[..., 2] - tt[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _brute(q, t):
    """per query: target indices in (d2, index) order over the finite targets, and their d2; non-finite queries get empty rows"""
    fin_t = np.isfinite(t[:, :3]).all(axis=1)
    tf = np.nonzero(fin_t)[0]
    d = _d2(q[:, :3], t[tf, :3]) if len(tf) else np.zeros((len(q), 0), np.float32)
    order = np.argsort(d, axis=1, kind="stable")     # stable on ascending index: ties by index
    fin_q = np.isfinite(q[:, :3]).all(axis=1)
    return tf[order], np.take_along_axis(d, order, axis=1), fin_q


def _check_knn(idx_s, d2_s, q, t, k):
    bi, bd, fin_q = _brute(q, t)
    kk = min(k, bi.shape[1])
    assert idx_s.shape == (len(q), k) and d2_s.shape == (len(q), k)
    want_i = np.full((len(q), k), -1, np.int32)
    want_d = np.full((len(q), k), np.inf, np.float32)
    want_i[fin_q, :kk] = bi[fin_q, :kk]
    want_d[fin_q, :kk] = bd[fin_q, :kk]
    bad = np.nonzero((idx_s != want_i).any(axis=1))[0]
    assert bad.size == 0, f"k={k}: {bad.size} rows differ from the brute force, first {bad[:3]}: {idx_s[bad[:2]]} vs {want_i[bad[:2]]}"
    assert (d2_s.view(np.uint32) == want_d.view(np.uint32)).all(), f"k={k}: distances differ bitwise"
    # the returned distances are the float recomputation of the returned pairs, bit for bit
    ok = idx_s >= 0
    if ok.any():
        re = _pair_d2(q[:, :3], t[:, :3], np.where(ok, idx_s, 0))
        assert (re[ok].view(np.uint32) == d2_s[ok].view(np.uint32)).all()


def _check_radius(res, q, t, r, max_nn=0):
    off, idx, d2 = res
    bi, bd, fin_q = _brute(q, t)
    r2 = np.float32(np.float64(r) * np.float64(r))
    assert off.shape == (len(q) + 1,) and off[0] == 0 and off[-1] == len(idx) == len(d2)
    for i in range(len(q)):
        a, b = int(off[i]), int(off[i + 1])
        m = int((bd[i] < r2).sum()) if fin_q[i] else 0
        if max_nn:
            m = min(m, max_nn)
        assert b - a == m, f"r={r} max_nn={max_nn}: row {i} has {b - a} hits, brute force {m}"
        assert (idx[a:b] == bi[i, :m]).all(), f"r={r}: row {i} indices differ"
        assert (d2[a:b].view(np.uint32) == bd[i, :m].view(np.uint32)).all(), f"r={r}: row {i} distances differ"


def _cloud(rng, n, kind):
    if kind == "random":
        p = rng.uniform(-20, 20, (n, 3))
    elif kind == "clusters":      # three clusters kilometres apart
        c = np.array([[0.0, 0.0, 0.0], [3000.0, -2000.0, 500.0], [-1500.0, 4000.0, -20.0]])
        p = c[rng.integers(0, 3, n)] + rng.normal(0, 1.0, (n, 3))
    elif kind == "plane":
        p = np.stack([rng.uniform(0, 50, n), rng.uniform(0, 50, n), np.zeros(n)], axis=1)
    elif kind == "line":
        s = rng.uniform(-30, 30, n)
        p = np.stack([s, 2 * s, -s], axis=1)
    elif kind == "identical":
        p = np.tile([[1.5, -2.25, 3.0]], (n, 1))
    elif kind == "lattice":      # integer lattice: many exactly equal distances (ties by index)
        p = rng.integers(0, 6, (n, 3)).astype(np.float64)
    else:
        raise ValueError(kind)
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = p
    out[:, 3] = rng.uniform(0, 1, n)
    return out


def _queries(rng, t, n):
    fin = t[np.isfinite(t[:, :3]).all(axis=1)]
    q = fin[rng.integers(0, len(fin), n)].copy()
    q[: n // 2, :3] += rng.normal(0, 0.5, (n // 2, 3)).astype(np.float32)
    lo, hi = fin[:, :3].min(axis=0), fin[:, :3].max(axis=0)
    far = lo + rng.uniform(0, 1, (8, 3)) * (hi - lo)
    far[:, rng.integers(0, 3)] += 1.0e4             # 10^4 m outside the bounding box
    q[-8:, :3] = far
    q[0, :3] = fin[0, :3]                           # exactly on a target point
    return q


@pytest.mark.parametrize("kind", ["random", "clusters", "plane", "line", "identical", "lattice"])
def test_knn_and_radius_exact_against_brute_force(gpu_ctx, kind):
    rng = np.random.default_rng(sum(kind.encode()))
    n = 600 if kind == "identical" else 3000
    t = _cloud(rng, n, kind)
    q = _queries(rng, t, 500)
    # non-finite targets are never returned, non-finite queries get empty rows
    t[7, 0] = np.nan
    t[11, 2] = np.inf
    q[5, 1] = np.nan
    q[9, 0] = -np.inf
    with gpu_ctx.search_index(t) as s:
        assert s.info() == (n, n - 2)
        qc = gpu_ctx.upload(q)
        for k in KS:
            idx, d2 = s.knn(qc, k)
            _check_knn(idx, d2, q, t, k)
        _, bd, fin_q = _brute(q, t)
        for frac in (0.1, 0.5):      # radii that cut through the clusters: the 10 % / 50 % quantile of the 5th-neighbour distance
            r = float(np.float32(float(np.sqrt(np.quantile(bd[fin_q, 4].astype(np.float64), frac))) + 1e-3))      # a float: both sides square the same number
            _check_radius(s.radius(qc, r), q, t, r)
            _check_radius(s.radius(qc, r, max_nn=3), q, t, r, max_nn=3)
        _check_radius(s.radius(qc, 0.0), q, t, 0.0)


def test_knn_kth_distance_matches_ckdtree_on_random_clouds(gpu_ctx):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(7)
    t = _cloud(rng, 20000, "random")
    q = _queries(rng, t, 4000)
    tree = cKDTree(t[:, :3].astype(np.float64))
    with gpu_ctx.search_index(t) as s:
        for k in KS:
            idx, d2 = s.knn(q, k)
            dd, ii = tree.query(q[:, :3].astype(np.float64), k=k + 1, workers=16)
            dd, ii = dd.reshape(len(q), -1), ii.reshape(len(q), -1)
            ref = _pair_d2(q[:, :3], t[:, :3], ii[:, k - 1:k])[:, 0]
            near_tie = np.abs(dd[:, k] - dd[:, k - 1]) <= 1e-6 * dd[:, k]      # float and double may order these two differently
            same = d2[:, k - 1].view(np.uint32) == ref.view(np.uint32)
            assert same[~near_tie].all(), f"k={k}: {(~same[~near_tie]).sum()} k-th distances differ from cKDTree"
            assert np.allclose(d2[near_tie, k - 1], ref[near_tie], rtol=2e-6, atol=0)


def test_knn_result_as_torch_and_bookkeeping(gpu_ctx, ltm):
    import torch
    rng = np.random.default_rng(3)
    t = _cloud(rng, 10, "random")
    q = _queries(rng, t, 40)
    live0 = gpu_ctx.pool_live()
    s = gpu_ctx.search_index(t)
    # k > n: k clamped to the target size, the rest of the row padded
    idx, d2 = s.knn(q, 16)
    assert (idx[:, 10:] == -1).all() and np.isinf(d2[:, 10:]).all() and (idx[np.isfinite(q[:, :3]).all(axis=1), :10] >= 0).all()
    _check_knn(idx, d2, q, t, 16)
    ti, td = s.knn(q, 16, as_torch=True)
    assert ti.is_cuda and ti.dtype == torch.int32 and td.dtype == torch.float32
    assert (ti.cpu().numpy() == idx).all() and (td.cpu().numpy().view(np.uint32) == d2.view(np.uint32)).all()
    off, ri, rd = s.radius(q, 5.0, as_torch=True)
    off_n, ri_n, _ = s.radius(q, 5.0)
    assert (off.cpu().numpy().astype(np.uint64) == off_n).all() and (ri.cpu().numpy() == ri_n).all()
    # k outside [1, 64]
    for bad_k in (0, 65, -1):
        with pytest.raises(ltm.LtmError):
            s.knn(q, bad_k)
    s.close()
    assert gpu_ctx.pool_live() == live0, "a freed index must give its memory back to the pool"
    # an empty target is valid and gives empty rows
    e = gpu_ctx.search_index(np.zeros((0, 4), np.float32))
    assert e.info() == (0, 0)
    idx, d2 = e.knn(q, 5)
    assert (idx == -1).all() and np.isinf(d2).all()
    off, ri, rd = e.radius(q, 1.0)
    assert (off == 0).all() and len(ri) == 0 and len(rd) == 0
    e.close()
    # only non-finite targets: as empty
    nanc = np.full((5, 4), np.nan, np.float32)
    with gpu_ctx.search_index(nanc) as e2:
        assert e2.info() == (5, 0)
        assert (e2.knn(q, 3)[0] == -1).all()
    assert gpu_ctx.pool_live() == live0


def test_index_lifetime_lanes_and_destroy(ltm):
    rng = np.random.default_rng(5)
    t = _cloud(rng, 2000, "random")
    ctx = ltm.Context(vfov=50.0, hfov=360.0, device=0)
    lane = ctx.lane()
    s = ctx.search_index(t)
    q = lane.upload(t[:10])
    lib = ctx.lib
    import ctypes as C
    buf = C.c_void_p()
    assert lib.ltm_buffer_alloc(lane.h, 10 * 4 * 4, C.byref(buf)) == 0
    # an index belongs to the context that built it: a lane is refused (before it could look inside)
    assert lib.ltm_knn_search(lane.h, s.h, q.h, 4, buf, buf) == -1
    res = C.c_void_p()
    assert lib.ltm_radius_search(lane.h, s.h, q.h, 1.0, 0, C.byref(res)) == -1
    assert lib.ltm_search_free(lane.h, s.h) == -1
    lib.ltm_buffer_free(lane.h, buf)
    # indices and results never freed are released by ltm_destroy (the pool ends balanced: nothing live but what handles hold)
    live0 = ctx.pool_live()
    s2 = ctx.search_index(t)
    assert lib.ltm_radius_search(ctx.h, s2.h, ctx.upload(t[:50]).h, 2.0, 0, C.byref(res)) == 0
    assert ctx.pool_live()[0] > live0[0]
    assert lib.ltm_search_result_free(ctx.h, res) == 0
    assert lib.ltm_search_result_free(ctx.h, res) == -1, "a freed result is refused"
    s2.close()
    assert ctx.pool_live() == live0
    s.h = None              # left open on purpose: ltm_destroy releases it
    assert lib.ltm_radius_search(ctx.h, ctx.search_index(t).h, ctx.upload(t[:50]).h, 2.0, 0, C.byref(res)) == 0
    lane.close()
    ctx.close()


def _lot(n_kf, device="cuda:0"):
    from tools import synth
    C = synth.to_numpy(synth.make_session(1, n_kf, device=device))
    Q = synth.to_numpy(synth.make_session(2, n_kf, device=device))
    return C, Q


def _mean_rule(d2, k, thr):
    """Session.cpp:590-599: float(sum of the k squared distances accumulated in double in ascending order) / k, fabs < thr"""
    acc = np.zeros(len(d2), np.float64)
    for j in range(k):
        acc = acc + d2[:, j].astype(np.float64)
    return np.abs(acc.astype(np.float32) / np.float32(k)) < np.float32(thr)


def test_knn_distances_reproduce_the_product_path_decisions(gpu_ctx):
    C, Q = _lot(20)
    ctx = gpu_ctx
    cmap = ctx.voxel_centroid(ctx.merge_to_global(ctx.upload_scans(C["scans"], C["offsets"]), ctx.poses(C["poses"], C["inv"])), 0.05)
    q_scans, q_poses = ctx.upload_scans(Q["scans"], Q["offsets"]), ctx.poses(Q["poses"], Q["inv"])
    g = ctx.merge_to_global(q_scans, q_poses)
    gq = g.download()
    off = Q["offsets"].astype(np.int64)
    # every point's local-frame output as ltm_knn_partition writes it (a threshold nothing fails)
    local_all = ctx.knn_partition(cmap, q_scans, q_poses, 1, 3.0e38)[0].download()[0]
    assert len(local_all) == len(gq)
    with ctx.search_index(cmap) as s:
        for k, thr in ((2, 0.01), (1, 0.2), (5, 0.05), (16, 0.5)):
            _, d2 = s.knn(g, k)
            mask = _mean_rule(d2, k, thr)
            assert 0 < mask.sum() < len(mask), "degenerate"
            co, di = ctx.knn_partition(cmap, q_scans, q_poses, k, thr)
            (co_p, co_o), (di_p, di_o) = co.download(), di.download()
            want_co = np.array([int(mask[off[j]:off[j + 1]].sum()) for j in range(len(off) - 1)])
            assert (np.diff(co_o.astype(np.int64)) == want_co).all(), f"k={k} thr={thr}: coexist counts per keyframe differ"
            assert (co_p.view(np.uint32) == local_all[mask].view(np.uint32)).all(), f"k={k} thr={thr}: coexist points differ"
            assert (di_p.view(np.uint32) == local_all[~mask].view(np.uint32)).all(), f"k={k} thr={thr}: diff points differ"
            near, far = ctx.knn_split_cloud(cmap, g, k, thr)
            assert (near.download().view(np.uint32) == gq[mask].view(np.uint32)).all(), f"k={k} thr={thr}: near split differs"
            assert (far.download().view(np.uint32) == gq[~mask].view(np.uint32)).all(), f"k={k} thr={thr}: far split differs"


def test_knn_and_radius_against_ckdtree_on_the_lot(gpu_ctx):
    from scipy.spatial import cKDTree
    C, Q = _lot(100)
    ctx = gpu_ctx
    cmap = ctx.voxel_centroid(ctx.merge_to_global(ctx.upload_scans(C["scans"], C["offsets"]), ctx.poses(C["poses"], C["inv"])), 0.05)
    t = cmap.download()
    gq = ctx.merge_to_global(ctx.upload_scans(Q["scans"], Q["offsets"]), ctx.poses(Q["poses"], Q["inv"])).download()
    rng = np.random.default_rng(11)
    q = gq[rng.choice(len(gq), size=min(200000, len(gq)), replace=False)]
    tree = cKDTree(t[:, :3].astype(np.float64))
    q64 = q[:, :3].astype(np.float64)
    with ctx.search_index(cmap) as s:
        idx, d2 = s.knn(q, 8)
        dd, ii = tree.query(q64, k=9, workers=16)
        re = _pair_d2(q[:, :3], t[:, :3], idx)
        assert (re.view(np.uint32) == d2.view(np.uint32)).all()
        ref = _pair_d2(q[:, :3], t[:, :3], ii[:, 7:8])[:, 0]
        near_tie = np.abs(dd[:, 8] - dd[:, 7]) <= 1e-6 * dd[:, 8]
        same = d2[:, 7].view(np.uint32) == ref.view(np.uint32)
        assert same[~near_tie].all(), f"{(~same[~near_tie]).sum()} 8th distances differ from cKDTree"
        # the neighbour sets: equal wherever the 8th and 9th neighbours are not (nearly) tied
        sets_ok = (np.sort(idx, axis=1) == np.sort(ii[:, :8], axis=1)).all(axis=1)
        assert sets_ok[~near_tie].all()
        off, ri, rd = s.radius(q, 0.5)
        lists = tree.query_ball_point(q64, 0.5, workers=16, return_sorted=True)
        r2 = np.float32(0.25)
        n_bad = 0
        for i in range(len(q)):
            a, b = int(off[i]), int(off[i + 1])
            got = set(ri[a:b].tolist())
            want = set(lists[i])
            for j in got ^ want:      # only pairs on the boundary (float vs double) may differ
                dj = np.linalg.norm(q64[i] - t[j, :3].astype(np.float64))
                assert abs(dj - 0.5) <= 1e-6, f"query {i}: target {j} at {dj} m differs from cKDTree"
                n_bad += 1
            assert (np.diff(rd[a:b]) >= 0).all() and (rd[a:b] < r2).all()
        assert n_bad <= 10
