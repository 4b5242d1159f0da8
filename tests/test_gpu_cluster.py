"""ltm_search_cluster on the device against the restatement (tools/cluster_numpy.py, pinned on the CPU by tests/test_cluster_api_cpu.py): a set partition and
a few integers per cluster, so everything but the centroid is compared for EQUALITY, on every fixture of tests/cluster_cases.py.  The centroid is a double
sum in another order than numpy's: it has to lie within n * 2^-52 * max|coordinate| of the float64 mean, the rounding bound of an n-term double sum."""
import gc

import numpy as np
import pytest

import cluster_cases as cc
from tools import cluster_numpy as cref

pytestmark = pytest.mark.gpu


def _download(cl):
    """everything a cluster set holds, as host arrays"""
    off, idx = cl.indices()
    return dict(labels=cl.labels(), sizes=cl.sizes.copy(), first=cl.first_index.copy(), offsets=off, idx=idx, boxes=cl.boxes.copy(), centroids=cl.centroids.copy())


def _run(ctx, name):
    pts, tol, lo, hi = cc.CASES[name]
    cloud = ctx.upload(pts)
    index = ctx.search_index(cloud)
    cl = index.cluster(tol, lo, hi)
    got = _download(cl)
    return cloud, index, cl, got


@pytest.fixture(scope="module", autouse=True)
def shared(gpu_ctx):
    """what the parametrised tests share: (cloud, index, cluster set, downloads) per fixture, made on first use.  The pool's live blocks are taken before
    the module's first call and compared after everything the module made has been freed, whichever tests ran and in whichever order."""
    gc.collect()      # handles other modules dropped go back to the pool now, not in the middle of this one
    gpu_ctx.synchronize()
    start = gpu_ctx.pool_live()
    cache = {}
    yield cache
    for cloud, index, cl, _ in cache.values():
        cl.close()
        index.close()
        cloud.free()
    cache.clear()
    gc.collect()
    gpu_ctx.synchronize()
    assert gpu_ctx.pool_live() == start, "the cluster tests left blocks of the pool handed out"


@pytest.fixture
def case(gpu_ctx, shared, request):
    name = request.param
    if name not in shared:
        shared[name] = _run(gpu_ctx, name)
    return (name,) + shared[name]


def _assert_same_bytes(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, f"{what}: {k} {a[k].shape} vs {b[k].shape}"
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def _assert_equals_reference(got, want, pts, what):
    for k in ("labels", "sizes", "first", "offsets", "idx"):
        assert got[k].dtype == want[k].dtype, (what, k, got[k].dtype)
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), f"{what}: {k} differs from the restatement"
    assert got["boxes"].shape == want["boxes"].shape and (got["boxes"].view(np.uint32) == want["boxes"].view(np.uint32)).all(), f"{what}: boxes differ bitwise"
    xyz = np.asarray(pts, np.float32)[:, :3]
    worst = 0.0
    for c in range(len(want["sizes"])):
        m = got["idx"][int(got["offsets"][c]):int(got["offsets"][c + 1])]
        bound = len(m) * 2.0 ** -52 * float(np.abs(xyz[m]).max())
        err = float(np.abs(got["centroids"][c] - want["centroids"][c]).max())
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0.0 else np.inf))
        assert err <= bound, f"{what}: centroid of cluster {c} off by {err:.3e}, bound {bound:.3e}"
    print(f"{what}: {len(want['sizes'])} clusters, worst centroid error / bound {worst:.3f}")


@pytest.mark.parametrize("case", list(cc.CASES), indirect=True)
def test_equals_the_restatement(case):
    name, _, _, cl, got = case
    pts = cc.CASES[name][0]
    want = cc.reference(name)
    assert cl.info() == (len(pts), len(want["sizes"]), len(want["idx"]))
    _assert_equals_reference(got, want, pts, name)


@pytest.mark.parametrize("case", list(cc.CASES), indirect=True)
def test_second_run_gives_identical_bytes(gpu_ctx, case):
    name, _, index, _, got = case
    _, tol, lo, hi = cc.CASES[name]
    with index.cluster(tol, lo, hi) as again:
        _assert_same_bytes(got, _download(again), name)


@pytest.mark.parametrize("case", list(cc.CASES), indirect=True)
def test_another_permutation_gives_the_same_partition(gpu_ctx, case):
    name, _, _, _, got = case
    pts, tol, lo, hi = cc.CASES[name]
    q = np.random.default_rng(99).permutation(len(pts))
    pts2 = np.ascontiguousarray(pts[q])      # point k of the second cloud is point q[k] of the first
    with gpu_ctx.search_index(pts2) as index2, index2.cluster(tol, lo, hi) as cl2:
        got2 = _download(cl2)
    _assert_equals_reference(got2, cref.cluster(pts2, tol, lo, hi), pts2, name + " permuted")

    def partition(g, back):
        return sorted(tuple(sorted(int(back[i]) for i in g["idx"][int(g["offsets"][c]):int(g["offsets"][c + 1])])) for c in range(len(g["sizes"])))

    assert partition(got, np.arange(len(pts))) == partition(got2, q)
    assert (got["sizes"] == got2["sizes"]).all()                                          # numbered by size either way
    assert ((got2["labels"] >= 0) == (got["labels"][q] >= 0)).all()
    if len(set(got["sizes"].tolist())) == len(got["sizes"]):                              # no ties: the numbering itself carries over
        assert (got2["labels"] == got["labels"][q]).all()


@pytest.mark.parametrize("case", list(cc.CASES), indirect=True)
def test_radius_neighbours_carry_the_point_s_label(gpu_ctx, case):
    """against the existing API, independent of the restatement: whatever ltm_radius_search returns for a point at the tolerance is in the point's component"""
    name, _, index, _, got = case
    pts, tol, _, _ = cc.CASES[name]
    fin = np.flatnonzero(np.isfinite(pts[:, :3]).all(axis=1))
    assert (got["labels"][~np.isfinite(pts[:, :3]).all(axis=1)] == -1).all()
    if not len(fin):      # nothing to sample: an empty cloud, or one without a finite point
        assert len(got["sizes"]) == 0
        return
    pick = np.random.default_rng(5).choice(fin, min(200, len(fin)), replace=False)
    off, idx, _ = index.radius(np.ascontiguousarray(pts[pick]), tol)
    checked = 0
    for k, i in enumerate(pick):
        nb = idx[int(off[k]):int(off[k + 1])]
        assert i in nb
        assert (got["labels"][nb] == got["labels"][i]).all(), f"{name}: a neighbour of point {i} has another label"
        checked += len(nb)
    assert checked >= len(pick)      # every sampled point is its own neighbour at least


@pytest.mark.parametrize("case", list(cc.CASES), indirect=True)
def test_extract_returns_the_points_of_every_row(gpu_ctx, case):
    name, cloud, _, cl, got = case
    pts = cc.CASES[name][0]
    ss = cl.extract(cloud)
    out, off = ss.download()
    ss.free()
    assert (off == got["offsets"]).all()
    assert out.tobytes() == np.ascontiguousarray(pts[got["idx"]]).tobytes()
    with pytest.raises(Exception) as e:
        cl.extract(np.zeros((len(pts) + 1, 4), np.float32))
    assert getattr(e.value, "code", None) == -1


def test_counters_show_the_clique_and_the_plain_path(gpu_ctx):
    def stats(name):
        pts, tol, lo, hi = cc.CASES[name]
        gpu_ctx.cluster_stats(reset=True)
        with gpu_ctx.search_index(pts) as index, index.cluster(tol, lo, hi):
            pass
        return gpu_ctx.cluster_stats(reset=True)

    n = len(cc.CASES["tolerance_below_pairs"][0])
    s = stats("tolerance_below_pairs")      # grid points 1 apart, tolerance 0.5: no leaf of 32 points is a clique, no pair is adjacent
    print("tolerance_below_pairs", s)
    assert s["clique_leaves"] == 0 and s["clique_early_exits"] == 0 and s["edges_found"] == 0 and s["pairs_tested"] > 0 and s["leaves_visited"] >= n // 32
    s = stats("tolerance_above_cloud")      # tolerance 10 over a unit cube: every leaf is a clique, every other leaf is left at its first point
    print("tolerance_above_cloud", s)
    assert s["clique_leaves"] == s["leaves_visited"] > 0 and s["clique_early_exits"] == s["edges_found"] == s["pairs_tested"] > 0
    s = stats("duplicates")                 # Morton ties: leaves of coincident points are cliques
    print("duplicates", s)
    assert s["clique_leaves"] > 0 and s["clique_early_exits"] > 0
    s = stats("chain_5000")
    print("chain_5000", s)
    assert s["edges_found"] >= 4999 and s["clique_leaves"] < s["leaves_visited"]
    assert stats("empty") == dict.fromkeys(s, 0)


def _batch(ctx, names):
    """one search index per fixture of `names`, built together: the fixtures are the keyframes of one scan set"""
    pts = [cc.CASES[n][0] for n in names]
    off = np.cumsum([0] + [len(p) for p in pts]).astype(np.uint64)
    ss = ctx.upload_scans(np.concatenate(pts) if pts else np.zeros((0, 4), np.float32), off)
    idx = ctx.search_index_batch(ss)
    ss.free()
    return idx


@pytest.mark.parametrize("n_idx", [1, 2, 65])
def test_batch_equals_single_calls(gpu_ctx, n_idx):
    pool = ["blobs", "empty", "uniform_257", "all_nonfinite", "duplicates", "uniform_33", "one_point", "nonfinite_mixed", "equal_sizes", "filter_seams"]
    names = [pool[k % len(pool)] for k in range(n_idx)]
    tol, lo, hi = 0.4, 2, 600
    indices = _batch(gpu_ctx, names)
    sets = gpu_ctx.cluster(indices, tol, lo, hi)
    assert len(sets) == n_idx
    singles = {}
    for k, name in enumerate(names):
        if name not in singles:
            with indices[k].cluster(tol, lo, hi) as one:
                singles[name] = _download(one)
            _assert_equals_reference(singles[name], cref.cluster(cc.CASES[name][0], tol, lo, hi),
                                     cc.CASES[name][0], f"{name} alone")
        _assert_same_bytes(singles[name], _download(sets[k]), f"{name} as index {k} of {n_idx}")
    for s in sets:
        s.close()
    for i in indices:
        i.close()


def test_the_same_index_twice_in_one_call(gpu_ctx):
    pts, tol, lo, hi = cc.CASES["blobs"]
    with gpu_ctx.search_index(pts) as index, gpu_ctx.search_index(cc.CASES["uniform_255"][0]) as other:
        a, b, c = gpu_ctx.cluster([index, other, index], tol, lo, hi)
        with index.cluster(tol, lo, hi) as one:
            want = _download(one)
        _assert_same_bytes(want, _download(a), "first listing")
        _assert_same_bytes(want, _download(c), "second listing")
        a.close()
        _assert_same_bytes(want, _download(c), "second listing after the first was freed")      # shared blocks live as long as one handle does
        b.close()
        c.close()


def test_errors_return_no_handle_and_leave_the_pool_as_it_was(gpu_ctx, ltm):
    gpu_ctx.synchronize()
    before = gpu_ctx.pool_live()      # whatever the shared fixtures hold stays as it is throughout
    pts = cc.CASES["uniform_257"][0]
    lane = gpu_ctx.lane()
    try:
        foreign = lane.search_index(pts)
        mine = gpu_ctx.search_index(pts)
        live = gpu_ctx.pool_live()
        for bad in ([foreign], [mine, foreign], [mine, mine, foreign]):
            hs = (ltm.C.c_void_p * len(bad))(*[x.h for x in bad])
            out = (ltm.C.c_void_p * len(bad))()
            p = ltm.cluster_params(0.5)
            assert gpu_ctx.lib.ltm_search_cluster(gpu_ctx.h, len(bad), hs, ltm.C.byref(p), out) == -1
            assert all(o is None for o in out)
            assert gpu_ctx.pool_live() == live
        for tol, lo, hi in ((0.0, 1, 0), (float("nan"), 1, 0), (0.5, 0, 0), (0.5, 5, 4)):
            hs = (ltm.C.c_void_p * 1)(mine.h)
            out = (ltm.C.c_void_p * 1)()
            p = ltm.ClusterParams(tol, lo, hi)
            assert gpu_ctx.lib.ltm_search_cluster(gpu_ctx.h, 1, hs, ltm.C.byref(p), out) == -1 and out[0] is None
            assert gpu_ctx.pool_live() == live
        cl = mine.cluster(0.7)
        with pytest.raises(ltm.LtmError) as e:      # a cluster set belongs to its context as well
            lane._ck(lane.lib.ltm_clusters_info(lane.h, cl.h, None, None, None))
        assert e.value.code == -1
        cl.close()
        mine.close()
        foreign.close()
    finally:
        lane.close()
    assert gpu_ctx.pool_live() == before
