"""ltm_search_filter_statistical / ltm_search_filter_radius on the device against the restatement (tools/outlier_numpy.py, pinned on the CPU by
tests/test_outlier_cases_cpu.py), on every fixture of tests/outlier_cases.py.  Distances, counts, labels, n_finite, n_kept, mean, stddev and threshold are
compared for EQUALITY, bit for bit: the device's arithmetic is stated in include/ltm.h so that both sides round the same way."""
import ctypes as C
import gc

import numpy as np
import pytest

import outlier_cases as oc
from tools import outlier_numpy as oref

pytestmark = pytest.mark.gpu

PER_POINT = ("labels", "values")
PER_RECORD = ("n_target", "n_finite", "n_kept", "mean", "stddev", "threshold")


def _download(out):
    """everything an outlier set holds, as host arrays (values: the distances of a statistical set, the counts of a radius set)"""
    values = out.distances() if out.kind == "statistical" else out.counts()
    return dict(labels=out.labels(), values=values, offsets=out.offsets(), n_target=out.n_target.copy(), n_finite=out.n_finite.copy(), n_kept=out.n_kept.copy(),
                mean=out.mean.copy(), stddev=out.stddev.copy(), threshold=out.threshold.copy())


def _filter(ctx, kind, indices, a, b):
    return ctx.statistical_outliers(indices, a, b) if kind == "sor" else ctx.radius_outliers(indices, a, b)


def _run(ctx, kind, name):
    pts, a, b = oc.case(kind, name)
    cloud = ctx.upload(pts)
    index = ctx.search_index(cloud)
    out = _filter(ctx, kind, [index], a, b)
    return cloud, index, out, _download(out)


@pytest.fixture(scope="module", autouse=True)
def shared(gpu_ctx):
    """what the parametrised tests share: (cloud, index, outlier set, downloads) per fixture, made on first use.  The pool's live blocks are taken before the
    module's first call and compared after everything the module made has been freed, whichever tests ran and in whichever order."""
    gc.collect()      # handles other modules dropped go back to the pool now, not in the middle of this one
    gpu_ctx.synchronize()
    start = gpu_ctx.pool_live()
    cache = {}
    yield cache
    for cloud, index, out, _ in cache.values():
        out.close()
        index.close()
        cloud.free()
    cache.clear()
    gc.collect()
    gpu_ctx.synchronize()
    assert gpu_ctx.pool_live() == start, "the outlier tests left blocks of the pool handed out"


@pytest.fixture
def case(gpu_ctx, shared, request):
    kind, name = request.param
    if (kind, name) not in shared:
        shared[(kind, name)] = _run(gpu_ctx, kind, name)
    return (kind, name) + shared[(kind, name)]


def _ids(cases):
    return [f"{k}-{n}" for k, n in cases]


def _assert_same_bytes(a, b, what, keys=None):
    for k in keys or a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, f"{what}: {k} {a[k].shape} vs {b[k].shape}"
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def _assert_equals_reference(got, want, kind, what):
    """one record against the restatement's dict, bit for bit"""
    n = want["n_target"]
    assert got["offsets"].tolist() == [0, n] and (int(got["n_target"][0]), int(got["n_finite"][0])) == (n, want["n_finite"]), what
    ref_values = want["distances"] if kind == "sor" else want["counts"]
    assert got["values"].dtype == ref_values.dtype and got["values"].shape == (n,)
    bad = np.flatnonzero(got["values"].view(np.uint32) != ref_values.view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.size} of {n} values differ from the restatement, first at {bad[:3]}: {got['values'][bad[:3]]} vs {ref_values[bad[:3]]}"
    if kind == "sor":
        for k in ("mean", "stddev", "threshold"):
            assert got[k].dtype == np.float64 and got[k][0].tobytes() == np.float64(want[k]).tobytes(), f"{what}: {k} {got[k][0]!r} vs {want[k]!r}"
    else:
        assert not got["mean"].any() and not got["stddev"].any() and not got["threshold"].any()
    assert got["labels"].dtype == np.uint8 and (got["labels"] == want["labels"]).all(), f"{what}: labels differ from the restatement"
    assert int(got["n_kept"][0]) == want["n_kept"] == int(got["labels"].sum()), what


@pytest.mark.parametrize("case", oc.ALL, ids=_ids(oc.ALL), indirect=True)
def test_equals_the_restatement(case):
    kind, name, _, _, out, got = case
    assert out.info() == (0 if kind == "sor" else 1, 1, len(oc.case(kind, name)[0]))
    _assert_equals_reference(got, oc.reference(kind, name), kind, f"{kind} {name}")


@pytest.mark.parametrize("case", oc.ALL, ids=_ids(oc.ALL), indirect=True)
def test_second_run_gives_identical_bytes(gpu_ctx, case):
    kind, name, _, index, _, got = case
    _, a, b = oc.case(kind, name)
    run = index.statistical_outliers if kind == "sor" else index.radius_outliers
    with run(a, b) as again:
        _assert_same_bytes(got, _download(again), f"{kind} {name}")


PERMUTED = [c for c in oc.ALL if not c[1].startswith("n163")] + [("sor", "n16385")]


@pytest.mark.parametrize("case", PERMUTED, ids=_ids(PERMUTED), indirect=True)
def test_a_permuted_input_gives_permuted_values(gpu_ctx, case):
    """distances and counts belong to the point, wherever it stands in the input; the radius labels too (the statistical threshold is a sum over the input
    order in a fixed shape: it may move in its last bits, so its labels are checked against the restatement of the permuted input instead)"""
    kind, name, _, _, _, got = case
    pts, a, b = oc.case(kind, name)
    q = np.random.default_rng(99).permutation(len(pts))
    pts2 = np.ascontiguousarray(pts[q])      # point k of the second cloud is point q[k] of the first
    with gpu_ctx.search_index(pts2) as index2, _filter(gpu_ctx, kind, [index2], a, b) as out2:
        got2 = _download(out2)
    assert got2["values"].tobytes() == got["values"][q].tobytes(), f"{kind} {name}: the values did not follow their points"
    assert int(got2["n_finite"][0]) == int(got["n_finite"][0])
    if kind == "ror":
        assert (got2["labels"] == got["labels"][q]).all() and int(got2["n_kept"][0]) == int(got["n_kept"][0])
    want2 = oref.statistical(pts2, a, b) if kind == "sor" else oref.radius(pts2, a, b)
    _assert_equals_reference(got2, want2, kind, f"{kind} {name} permuted")


BATCH_NAMES = ("empty", "plane", "one_point", "non_finite_mixed", "empty", "n257", "two_points", "plane", "all_non_finite", "coincident_500", "n256")
BATCH_PARAMS = [("sor", 8, 1.0), ("sor", 20, 0.5), ("ror", 0.6, 3)]


@pytest.mark.parametrize("kind,a,b", BATCH_PARAMS, ids=[f"{k}-{a}" for k, a, _ in BATCH_PARAMS])
def test_batches_give_every_record_the_bytes_of_its_single_call(gpu_ctx, kind, a, b):
    """batches of 1, 2 and 65 indices, empty ones and repeats among them (the same index object listed again), through one call each"""
    names = sorted(set(BATCH_NAMES))
    clouds = {n: gpu_ctx.upload(oc.SOR[n][0]) for n in names}
    indices = {n: gpu_ctx.search_index(clouds[n]) for n in names}
    single = {}
    for n in names:
        with _filter(gpu_ctx, kind, [indices[n]], a, b) as out:
            single[n] = _download(out)
    for size in (1, 2, 65):
        listed = [BATCH_NAMES[(3 * size + j) % len(BATCH_NAMES)] for j in range(size)]
        with _filter(gpu_ctx, kind, [indices[n] for n in listed], a, b) as out:
            got = _download(out)
            assert out.info() == (0 if kind == "sor" else 1, size, sum(len(oc.SOR[n][0]) for n in listed))
        off = got["offsets"]
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(oc.SOR[n][0]) for n in listed])]).tolist()
        for r, n in enumerate(listed):
            rec = {k: got[k][int(off[r]):int(off[r + 1])] for k in PER_POINT}
            rec.update({k: got[k][r:r + 1] for k in PER_RECORD})
            _assert_same_bytes(rec, single[n], f"{kind} batch of {size}, record {r} ({n})", PER_POINT + PER_RECORD)
    for n in names:
        indices[n].close()
        clouds[n].free()


def test_an_empty_list_gives_an_empty_set(gpu_ctx):
    for kind, a, b in BATCH_PARAMS:
        with _filter(gpu_ctx, kind, [], a, b) as out:
            assert out.info() == (0 if kind == "sor" else 1, 0, 0) and out.offsets().tolist() == [0] and len(out.labels()) == 0 and len(out.n_kept) == 0


SPLIT_NAMES = ("plane", "empty", "non_finite_mixed", "one_point", "n257")


@pytest.mark.parametrize("kind,a,b", BATCH_PARAMS, ids=[f"{k}-{a}" for k, a, _ in BATCH_PARAMS])
def test_split_gives_both_sides_in_input_order(gpu_ctx, ltm, kind, a, b):
    parts = [oc.SOR[n][0] for n in SPLIT_NAMES]
    pts = np.concatenate(parts)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    scans = gpu_ctx.upload_scans(pts, offsets)
    indices = gpu_ctx.search_index_batch(scans)
    with _filter(gpu_ctx, kind, indices, a, b) as out:
        labels, n_kept = out.labels(), out.n_kept
        kept, removed = out.split(scans)
        for side, flag, sizes in ((kept, 1, n_kept), (removed, 0, out.n_target - n_kept)):
            got, off = side.download()
            assert np.diff(off.astype(np.int64)).tolist() == sizes.tolist()
            assert got.view(np.uint32).tobytes() == pts[labels == flag].view(np.uint32).tobytes()      # input order, keyframe after keyframe
            side.free()
        # a scan set of another shape: fewer keyframes, and as many keyframes with other sizes
        other = np.concatenate([[0], np.cumsum([len(p) for p in parts[::-1]])]).astype(np.uint64)
        for bad in (gpu_ctx.upload_scans(pts, offsets[[0, 1, 3, 5]]), gpu_ctx.upload_scans(pts, other)):
            with pytest.raises(ltm.LtmError) as e:
                out.split(bad)
            assert e.value.code == -1
            bad.free()
        with pytest.raises(ltm.LtmError) as e:      # the cloud form takes a set of one record
            out.split(pts)
        assert e.value.code == -1
    # the cloud form
    with _filter(gpu_ctx, kind, [indices[0]], a, b) as one:
        labels = one.labels()
        kept, removed = one.split(parts[0])
        assert kept.download().view(np.uint32).tobytes() == parts[0][labels == 1].view(np.uint32).tobytes() and len(kept) == int(one.n_kept[0])
        assert removed.download().view(np.uint32).tobytes() == parts[0][labels == 0].view(np.uint32).tobytes()
        kept.free()
        removed.free()
        with pytest.raises(ltm.LtmError) as e:
            one.split(parts[0][:-1])
        assert e.value.code == -1
    for index in indices:
        index.close()
    scans.free()


def test_errors_return_no_handle(gpu_ctx, ltm):
    lib = gpu_ctx.lib
    pts = oc.SOR["plane"][0]
    lane = gpu_ctx.lane()
    theirs = lane.search_index(pts)
    with gpu_ctx.search_index(pts) as mine:
        before = gpu_ctx.pool_live()
        nan, inf = float("nan"), float("inf")

        def refused(call, params, handles):
            hs = (C.c_void_p * len(handles))(*handles)
            out = C.c_void_p(0x1234)
            rc = call(gpu_ctx.h, len(handles), hs, None if params is None else C.byref(params), C.byref(out))
            return rc == -1 and out.value is None

        for mean_k, mul in ((0, 1.0), (64, 1.0), (2 ** 31, 1.0), (8, nan), (8, inf), (8, -inf)):
            assert refused(lib.ltm_search_filter_statistical, ltm.SorParams(mean_k, mul), [mine.h]), (mean_k, mul)
        for radius, m in ((0.0, 1), (-1.0, 1), (nan, 1), (inf, 1), (0.5, 0)):
            assert refused(lib.ltm_search_filter_radius, ltm.RorParams(radius, m), [mine.h]), (radius, m)
        good_s, good_r = ltm.sor_params(8, 1.0), ltm.ror_params(0.5, 2)
        for handles in ([theirs.h], [mine.h, theirs.h], [mine.h, None], [mine.h, mine.h, theirs.h]):      # a lane's index, a NULL index: wherever it stands
            assert refused(lib.ltm_search_filter_statistical, good_s, handles)
            assert refused(lib.ltm_search_filter_radius, good_r, handles)
        assert refused(lib.ltm_search_filter_statistical, None, [mine.h]) and refused(lib.ltm_search_filter_radius, None, [mine.h])
        assert lib.ltm_search_filter_statistical(gpu_ctx.h, 1, None, C.byref(good_s), C.byref(C.c_void_p())) == -1
        assert lib.ltm_search_filter_statistical(gpu_ctx.h, 1, (C.c_void_p * 1)(mine.h), C.byref(good_s), None) == -1
        with pytest.raises(ltm.LtmError) as e:
            lane.statistical_outliers([mine], 8, 1.0)      # and the other way round
        assert e.value.code == -1
        # a handle of the other kind has no such array; a freed handle is no handle
        with mine.radius_outliers(0.5, 2) as ror, mine.statistical_outliers(8, 1.0) as sor:
            d, u = np.empty(len(pts), np.float32), np.empty(len(pts), np.uint32)
            assert lib.ltm_outliers_download(gpu_ctx.h, ror.h, *([None] * 7), d.ctypes.data, None) == -1
            assert lib.ltm_outliers_download(gpu_ctx.h, ror.h, None, None, None, d.ctypes.data, *([None] * 5)) == -1
            assert lib.ltm_outliers_download(gpu_ctx.h, sor.h, *([None] * 8), u.ctypes.data) == -1
            assert lib.ltm_outliers_info(lane.h, sor.h, None, None, None) == -1
            stale = sor.h
        assert lib.ltm_outliers_free(gpu_ctx.h, stale) == -1
        gpu_ctx.synchronize()
        assert gpu_ctx.pool_live() == before, "a refused call left blocks of the pool handed out"
    theirs.close()
    lane.close()


def test_counters(gpu_ctx):
    gpu_ctx.outlier_stats(reset=True)
    assert gpu_ctx.outlier_stats() == dict(finite_points=0, distance_evaluations=0, radius_early_stops=0, records=0)
    names = ("plane", "non_finite_mixed", "empty", "all_non_finite", "n257")
    indices = [gpu_ctx.search_index(oc.SOR[n][0]) for n in names]
    with gpu_ctx.statistical_outliers(indices, 8, 1.0) as out:
        finite = int(out.n_finite.sum())
    s = gpu_ctx.outlier_stats()
    assert (s["finite_points"], s["records"], s["radius_early_stops"]) == (finite, len(names), 0)
    assert s["distance_evaluations"] >= 9 * finite      # at least the neighbourhood of every point
    with gpu_ctx.statistical_outliers(indices[:2], 20, 1.0) as out:      # the LDS form counts the same way
        finite += int(out.n_finite.sum())
    s = gpu_ctx.outlier_stats()
    assert (s["finite_points"], s["records"]) == (finite, len(names) + 2)
    gpu_ctx.outlier_stats(reset=True)
    pts, radius, m = oc.ROR["plane_min2"]
    with gpu_ctx.search_index(pts) as index, index.radius_outliers(radius, m) as out:
        s = gpu_ctx.outlier_stats()
        assert (s["finite_points"], s["records"]) == (int(out.n_finite[0]), 1)
        assert 0 < s["radius_early_stops"] <= int(out.n_kept[0])      # only a walk that found its second neighbour can have stopped
        assert s["distance_evaluations"] >= s["finite_points"]
    for index in indices:
        index.close()
