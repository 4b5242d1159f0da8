"""Every kernel that walks the box tree of the search index besides the kNN and radius kernels -- normals, statistical and radius outlier removal,
clusters, FPFH, the correspondence step of ICP -- over the case matrix of tests/walker_cases.py: the tree shapes with 0 / 1 / 3 / 31 padding leaves, every
list form full and one past, every state of the seed, exact ties by index on both sides of the seed, radii and tolerances on both sides of a tie, and
clouds whose squared distances underflow, are denormal, overflow or whose codes collapse (tests/test_walker_cases_cpu.py shows on the host that the
cases reach what they are named for).  Each consumer is held against a restatement that never sees a device kNN result: the numpy tools under tools/,
fed by the float brute force of the target against itself.  Then all of it through ONE batched build, whose segmented sort is not stable, and again on a
second run."""
import gc

import numpy as np
import pytest

import fpfh_cases as fc
import icp_fixtures as fx
import normals_cases as nc
import search_cases as sc
import walker_cases as wc
from test_gpu_cluster import _assert_equals_reference as _cluster_equals
from test_gpu_cluster import _download as _cluster_download
from test_gpu_fpfh import _assert_equals_reference as _fpfh_equals
from test_gpu_fpfh import _download as _fpfh_download
from test_gpu_outlier import _download as _outlier_download
from tools import cluster_numpy as cref
from tools import fpfh_numpy as fref
from tools import icp_numpy as iref
from tools import normals_numpy as nref
from tools import outlier_numpy as oref

pytestmark = pytest.mark.gpu

PER_POINT = ("labels", "values")
PER_RECORD = ("n_target", "n_finite", "n_kept", "mean", "stddev", "threshold")


@pytest.fixture(scope="module", autouse=True)
def shared(gpu_ctx):
    """one index per cloud for the whole module, made on first use.  The pool's live blocks are taken before the module's first call and compared after
    everything the module made has been freed, whichever tests ran and in whichever order."""
    gc.collect()
    gpu_ctx.synchronize()
    start = gpu_ctx.pool_live()
    cache = {}
    yield cache
    for cloud, index in cache.values():
        index.close()
        cloud.free()
    cache.clear()
    gc.collect()
    gpu_ctx.synchronize()
    assert gpu_ctx.pool_live() == start, "the walker tests left blocks of the pool handed out"


def _index(ctx, shared, name):
    if name not in shared:
        cloud = ctx.upload(wc.CASES[name])
        shared[name] = (cloud, ctx.search_index(cloud))
        t = wc.CASES[name]
        assert shared[name][1].info() == (len(t), int(sc.finite_rows(t).sum()))
    return shared[name][1]


def _same_bytes(a, b, what, keys=None):
    for k in keys or a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, f"{what}: {k} {a[k].shape} vs {b[k].shape}"
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


# ------------------------------------------------------------------------------------------------------------------ normals
def _check_normals(index, name, k):
    t = wc.CASES[name]
    with np.errstate(all="ignore"):
        r = nref.estimate(t, k)
    fin = sc.finite_rows(t)
    if name in sc.SHAPES and fin.sum() >= 33 and k >= 5:      # a condition on the case, not a measurement: the directions are compared nearly everywhere
        share = float(nc.well_posed(r)[fin].mean())
        assert share >= 0.98, f"{name} k={k}: only {100 * share:.1f} % of the finite points are well-posed"
    index.estimate_normals(k)
    assert index.normals_k() == k
    got = index.normals()
    if fin.sum() < 3:      # no neighbourhood of three: every row is NaN
        assert got.shape == (len(t), 4) and np.isnan(got).all() and np.isnan(r["normals"]).all(), (name, k)
        return
    with np.errstate(all="ignore"):
        # the viewpoint is the origin: |viewpoint - point| is the point's own magnitude (1e7 on offset_1e7, 3e38 on the huge points of overflow, where the
        # flip's dot product is a difference of products of 1e38 that cancel and its sign is rounding noise)
        nc.compare(got, r, f"{name} k={k}", reach=np.abs(t[:, :3].astype(np.float64)).sum(axis=1))


@pytest.mark.parametrize("name", wc.MATRIX)
def test_normals_equal_the_restatement(gpu_ctx, shared, name):
    """NaN pattern, direction within 2^-23 where the gap makes it well-posed, curvature within 1e-12 + 2^-23 curvature on EVERY finite point (what a wrong
    neighbour set moves on the tie clouds, where few directions are well-posed), unit length"""
    index = _index(gpu_ctx, shared, name)
    for k in wc.normals_ks(name):
        _check_normals(index, name, k)


# ----------------------------------------------------------------------------------------------------------------- outliers
def _same_double(a, b):
    a, b = float(a), float(b)
    return (np.isnan(a) and np.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


def _sor_want(name, mean_k):
    """the restatement fed by the brute force: distances from the mean_k + 1 smallest float d2 of every finite point, statistics and labels from them"""
    t = wc.CASES[name]
    fin, _, bd = wc.brute_self(name)
    kk = min(mean_k + 1, len(fin))
    with np.errstate(all="ignore"):
        dist = np.zeros(len(t), np.float32)
        dist[fin] = oref._distance_from_sorted_d2(bd[:, :kk], mean_k)
        return oref._sor_result(t, dist, wc.SOR_STDDEV_MUL)


def _check_sor(got, want, what):
    n = want["n_target"]
    assert got["offsets"].tolist() == [0, n] and (int(got["n_target"][0]), int(got["n_finite"][0])) == (n, want["n_finite"]), what
    assert got["values"].dtype == np.float32 and got["values"].shape == (n,)
    bad = np.flatnonzero(got["values"].view(np.uint32) != want["distances"].view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.size} of {n} distances differ, first at {bad[:3]}: {got['values'][bad[:3]]} vs {want['distances'][bad[:3]]}"
    for k in ("mean", "stddev", "threshold"):      # bit for bit; NaN and the infinities by position (overflow, collapse)
        assert got[k].dtype == np.float64 and _same_double(got[k][0], want[k]), f"{what}: {k} {got[k][0]!r} vs {want[k]!r}"
    assert got["labels"].dtype == np.uint8 and (got["labels"] == want["labels"]).all(), f"{what}: labels differ from the restatement"
    assert int(got["n_kept"][0]) == want["n_kept"] == int(got["labels"].sum()), what


@pytest.mark.parametrize("name", wc.MATRIX)
def test_statistical_outliers_equal_the_brute_force(gpu_ctx, shared, name):
    index = _index(gpu_ctx, shared, name)
    for mean_k in wc.sor_mean_ks(name):
        want = _sor_want(name, mean_k)
        with index.statistical_outliers(mean_k, wc.SOR_STDDEV_MUL) as out:
            _check_sor(_outlier_download(out), want, f"sor {name} mean_k={mean_k}")


def _ror_want(name, r, m):
    t = wc.CASES[name]
    fin, _, _ = wc.brute_self(name)
    nb = np.zeros(len(t), np.int64)
    nb[fin] = wc.self_counts(name, r)
    return oref._ror_result(t, nb, m)


def _check_ror(got, want, what):
    n = want["n_target"]
    assert got["offsets"].tolist() == [0, n] and (int(got["n_target"][0]), int(got["n_finite"][0])) == (n, want["n_finite"]), what
    assert got["values"].dtype == np.uint32 and got["values"].shape == (n,)
    bad = np.flatnonzero(got["values"] != want["counts"])
    assert bad.size == 0, f"{what}: {bad.size} of {n} counts differ, first at {bad[:3]}: {got['values'][bad[:3]]} vs {want['counts'][bad[:3]]}"
    assert (got["labels"] == want["labels"]).all() and int(got["n_kept"][0]) == want["n_kept"] == int(got["labels"].sum()), what


@pytest.mark.parametrize("name", wc.MATRIX)
def test_radius_outliers_equal_the_brute_force(gpu_ctx, shared, name):
    index = _index(gpu_ctx, shared, name)
    for r, m in wc.ror_list(name):
        with index.radius_outliers(float(r), m) as out:
            _check_ror(_outlier_download(out), _ror_want(name, r, m), f"ror {name} r={r!r} min_neighbors={m}")


# ----------------------------------------------------------------------------------------------------------------- clusters
@pytest.mark.parametrize("name", wc.CLUSTER_CLOUDS)
def test_clusters_equal_the_restatement(gpu_ctx, shared, name):
    """everything exact, the centroid within the bound of an n-term double sum; the counter of clique leaves is above 0 where the rule, restated over the
    leaf boxes of the host model, has a clique leaf of two points or more (each of its points but the first visits it), and 0 where it has none"""
    t = wc.CASES[name]
    index = _index(gpu_ctx, shared, name)
    model = sc.tree_model(t)
    leaf_size = np.minimum(sc.LEAF, model.Mf - sc.LEAF * np.arange(model.L))
    for tol in wc.cluster_tolerances(name):
        want = cref.cluster(t, float(tol), 1, None)
        gpu_ctx.cluster_stats(reset=True)
        with index.cluster(float(tol), 1, None) as cl:
            stats = gpu_ctx.cluster_stats(reset=True)
            assert cl.info() == (len(t), len(want["sizes"]), len(want["idx"]))
            _cluster_equals(_cluster_download(cl), want, t, f"{name} tolerance {tol!r}")
        clique = wc.clique_leaves(model, sc.r2_of(tol), "new")
        if (clique & (leaf_size >= 2)).any():
            assert stats["clique_leaves"] > 0, (name, tol, stats)
        if not clique.any():
            assert stats["clique_leaves"] == 0 and stats["clique_early_exits"] == 0, (name, tol, stats)


# --------------------------------------------------------------------------------------------------------------------- FPFH
@pytest.mark.parametrize("name", wc.FPFH_CLOUDS)
def test_fpfh_equals_the_restatement(gpu_ctx, shared, name):
    t = wc.CASES[name]
    index = _index(gpu_ctx, shared, name)
    index.estimate_normals(fc.NORMALS_K)
    normals = np.ascontiguousarray(index.normals()[:, :3])      # the device's own normals: what is under test here is the descriptor
    for k in wc.FPFH_KS:
        with np.errstate(all="ignore"):
            want = fref.fpfh(t, normals, k)
        with index.fpfh(k) as out:
            got = _fpfh_download(out)
            assert out.info() == (1, len(t), k)
        assert got["offsets"].tolist() == [0, len(t)] and (int(got["n_target"][0]), int(got["n_finite"][0])) == (len(t), want["n_finite"])
        _fpfh_equals(got["descriptors"], got["spfh_counts"], want, f"{name} k={k}")


# ---------------------------------------------------------------------------------------------------------------------- ICP
def _icp(ctx, index, source, max_corr):
    return ctx.icp_align([(index, source)], trace=True, max_iterations=1, max_corr_dist=max_corr)


@pytest.mark.parametrize("name", wc.ICP_CLOUDS)
def test_icp_correspondences_equal_the_brute_force(gpu_ctx, shared, name):
    """knn_collect at k = 1.  With the identity start the query is the source point itself (1 * x + 0 + 0 + 0 is exact), so the first iteration's
    correspondences are the brute force's nearest neighbours: their number exactly, their mean float d2 (summed as doubles, in another order) within
    a relative n * 2^-52, the bound of an n-term sum of non-negative terms"""
    c = sc.CASES[name]
    index = _index(gpu_ctx, shared, name)
    _, bd, fq = sc.brute(name)
    d = bd[fq, 0].astype(np.float64)
    for max_corr in wc.ICP_MAX_CORR:
        keep = d <= max_corr * max_corr
        n = int(keep.sum())
        res, tr = _icp(gpu_ctx, index, c.queries, max_corr)
        assert tr.shape == (1, 1, 2)
        assert tr[0, 0, 0] == n, f"{name} max_corr_dist={max_corr}: {tr[0, 0, 0]} correspondences, the brute force has {n}"
        if n:
            want = float(d[keep].mean())
            assert abs(tr[0, 0, 1] - want) <= n * 2.0 ** -52 * want, (name, max_corr, tr[0, 0, 1], want)
        else:
            assert np.isnan(tr[0, 0, 1])
        assert int(res["n_corr"][0]) == n
        if name == "lattice_x3":      # the 64 cell centres tie eight ways: a nearest neighbour taken by another tie rule moves T by centimetres
            assert n >= 64 and np.abs(c.queries[fq, :3]).max() < fx.EXTENT
            want = iref.align(c.target, c.queries, max_corr_dist=max_corr, max_iterations=1)
            assert int(res["iterations"][0]) == want["iterations"] and int(res["state"][0]) == want["state"]
            err = np.abs(np.asarray(res["T"][0]).reshape(4, 4) - want["T"]).max()
            assert err <= fx.tol_T(int(fq.sum())), (name, max_corr, err)


# ------------------------------------------------------------------------------------------------------------ batched build
BATCH_NORMALS_K = fc.NORMALS_K      # the normals FPFH takes
BATCH_FPFH_K = 5
BATCH_SOR = (8, 1.0)
BATCH_RADIUS = 1.0                  # at a tie on the lattice: the six neighbours are at d2 == r2, outside
BATCH_ROR_MIN = 4                   # one more than the three copies of a lattice point
BATCH_MIN_SIZE = 1


def test_one_batched_build_gives_every_consumer_the_bytes_of_the_single_build(gpu_ctx, shared):
    """every cloud of the matrix as one keyframe of one scan set, one search_index_batch, one batched call per consumer: every record is byte for byte
    that of the call on the singly built index.  The segmented sort of the batched build is not stable; coincident_100, lattice_x3, collapse and
    offset_1e7 are where equal codes change places, so this is where a result that depends on the order of equal codes would show."""
    names = list(wc.CASES)
    clouds = [wc.CASES[n] for n in names]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.uint64)
    singles = [_index(gpu_ctx, shared, n) for n in names]
    for s in singles:      # the single indices keep their normals beyond this test: estimated before the pool is looked at
        s.estimate_normals(BATCH_NORMALS_K)
    gpu_ctx.synchronize()
    live = gpu_ctx.pool_live()
    scans = gpu_ctx.upload_scans(np.concatenate(clouds), off)
    batch = gpu_ctx.search_index_batch(scans)
    assert len(batch) == len(names) and all(b.info() == s.info() for b, s in zip(batch, singles))

    gpu_ctx.estimate_normals(batch, BATCH_NORMALS_K)
    for name, b, s in zip(names, batch, singles):
        assert b.normals().tobytes() == s.normals().tobytes(), f"normals of {name} differ between the batched and the single build"

    sets = gpu_ctx.cluster(batch, BATCH_RADIUS, BATCH_MIN_SIZE)
    for name, cl, s in zip(names, sets, singles):
        with s.cluster(BATCH_RADIUS, BATCH_MIN_SIZE) as one:
            _same_bytes(_cluster_download(one), _cluster_download(cl), f"clusters of {name}")
        cl.close()

    for kind, call, args in (("sor", gpu_ctx.statistical_outliers, BATCH_SOR), ("ror", gpu_ctx.radius_outliers, (BATCH_RADIUS, BATCH_ROR_MIN))):
        with call(batch, *args) as out:
            got = _outlier_download(out)
        assert got["offsets"].tolist() == off.tolist()
        for r, (name, s) in enumerate(zip(names, singles)):
            rec = {k: got[k][int(off[r]):int(off[r + 1])] for k in PER_POINT}
            rec.update({k: got[k][r:r + 1] for k in PER_RECORD})
            with call([s], *args) as one:
                _same_bytes(rec, _outlier_download(one), f"{kind} record {r} ({name})", PER_POINT + PER_RECORD)

    with gpu_ctx.fpfh(batch, BATCH_FPFH_K) as out:
        got = _fpfh_download(out)
    assert got["offsets"].tolist() == off.tolist()
    for r, (name, s) in enumerate(zip(names, singles)):
        with s.fpfh(BATCH_FPFH_K) as one:
            want = _fpfh_download(one)
        for key in ("descriptors", "spfh_counts"):
            assert got[key][int(off[r]):int(off[r + 1])].tobytes() == want[key].tobytes(), f"FPFH record {r} ({name}): {key} differs from the single build"
        assert (int(got["n_target"][r]), int(got["n_finite"][r])) == (int(want["n_target"][0]), int(want["n_finite"][0]))

    for b in batch[::-1]:
        b.close()
    scans.free()
    gpu_ctx.synchronize()
    assert gpu_ctx.pool_live() == live, "the blocks of the batch must be back in the pool"


# --------------------------------------------------------------------------------------------------------------- second run
@pytest.mark.parametrize("name", wc.TIES_AND_RANGE)
def test_second_run_gives_identical_bytes(gpu_ctx, shared, name):
    index = _index(gpu_ctx, shared, name)
    c = sc.CASES[name]

    def normals(k):
        index.estimate_normals(k)
        return dict(normals=index.normals())

    def outliers(call, *args):
        with call(*args) as out:
            return _outlier_download(out)

    def clusters(tol):
        with index.cluster(float(tol), 1, None) as cl:
            return _cluster_download(cl)

    def fpfh(k):
        index.estimate_normals(fc.NORMALS_K)
        with index.fpfh(k) as out:
            return _fpfh_download(out)

    def icp():
        res, tr = _icp(gpu_ctx, index, c.queries, 150.0)
        return dict(result=np.frombuffer(res.tobytes(), np.uint8), trace=tr)

    r, m = wc.ror_list(name)[0]
    runs = [("normals k=9", lambda: normals(9)), ("normals k=17", lambda: normals(17)),
            ("sor", lambda: outliers(index.statistical_outliers, 8, wc.SOR_STDDEV_MUL)), ("ror", lambda: outliers(index.radius_outliers, float(r), m)),
            ("clusters", lambda: clusters(wc.cluster_tolerances(name)[0])), ("fpfh", lambda: fpfh(5))]
    if name in wc.ICP_CLOUDS:
        runs.append(("icp", icp))
    for what, run in runs:
        _same_bytes(run(), run(), f"{name} {what}")
