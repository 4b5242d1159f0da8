"""ltm_search_fpfh on the device against the restatement (tools/fpfh_numpy.py, pinned on the CPU by tests/test_fpfh_cases_cpu.py), on every fixture of
tests/fpfh_cases.py.  The normals are the device's own (estimated at k = 10, downloaded, and given to the restatement as float32), or one hand-set normal
written over them where the fixture says so.  SPFH counts are compared for EQUALITY and descriptors bit for bit, NaN rows by position: the device's arithmetic
is stated in include/ltm.h so that both sides round the same way."""
import ctypes as C
import gc

import numpy as np
import pytest

import fpfh_cases as fc
from tools import fpfh_numpy as fref

pytestmark = pytest.mark.gpu


def _set_normals(ctx, index, normal):
    """every stored normal of the index becomes `normal` (curvature 0): the stored array is in the index's own order, so one value for all needs no order"""
    k, dev = C.c_int(), C.c_void_p()
    ctx._ck(ctx.lib.ltm_search_normals_info(ctx.h, index.h, C.byref(k), C.byref(dev)))
    n_finite = index.info()[1]
    assert k.value == fc.NORMALS_K
    if n_finite:
        host = np.tile(np.float32(list(normal) + [0.0]), (n_finite, 1))
        ctx.synchronize()
        ctx._ck(ctx.lib.ltm_buffer_copy(ctx.h, dev, host.ctypes.data, host.nbytes, 0))


def _prepare(ctx, name, index=None):
    """(cloud or None, index with normals, the normals as the restatement takes them)"""
    case = fc.CASES[name]
    cloud = None
    if index is None:
        cloud = ctx.upload(case["points"])
        index = ctx.search_index(cloud)
    index.estimate_normals(fc.NORMALS_K)
    if case["normal"] is not None:
        _set_normals(ctx, index, case["normal"])
    normals = index.normals()[:, :3] if len(case["points"]) else np.zeros((0, 3), np.float32)
    return cloud, index, np.ascontiguousarray(normals)


def _download(out):
    return dict(descriptors=out.descriptors(), spfh_counts=out.spfh_counts(), offsets=out.offsets(), n_target=out.n_target.copy(), n_finite=out.n_finite.copy())


def _assert_same_bytes(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, f"{what}: {k} {a[k].shape} vs {b[k].shape}"
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def _assert_equals_reference(desc, counts, want, what):
    n = want["n_target"]
    assert desc.dtype == np.float32 and desc.shape == (n, 33) and counts.dtype == np.uint8 and counts.shape == (n, 33), what
    bad = np.flatnonzero((counts != want["spfh_counts"]).any(axis=1))
    assert bad.size == 0, f"{what}: the SPFH counts of {bad.size} of {n} points differ, first at {bad[:3]}: {counts[bad[:1]]} vs {want['spfh_counts'][bad[:1]]}"
    nan_got, nan_want = np.isnan(desc), np.isnan(want["descriptors"])
    assert (nan_got == nan_want).all(), f"{what}: NaN rows at other positions"
    bad = np.flatnonzero(((desc.view(np.uint32) != want["descriptors"].view(np.uint32)) & ~nan_want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {n} descriptors differ from the restatement, first at {bad[:3]}: {desc[bad[:1]]} vs {want['descriptors'][bad[:1]]}"


@pytest.fixture(scope="module", autouse=True)
def shared(gpu_ctx):
    """what the parametrised tests share: (cloud, index, normals, descriptor set, downloads, restatement) per fixture, made on first use.  The pool's live
    blocks are taken before the module's first call and compared after everything the module made has been freed."""
    gc.collect()
    gpu_ctx.synchronize()
    start = gpu_ctx.pool_live()
    cache = {}
    yield cache
    for cloud, index, _, out, _, _ in cache.values():
        out.close()
        index.close()
        cloud.free()
    cache.clear()
    gc.collect()
    gpu_ctx.synchronize()
    assert gpu_ctx.pool_live() == start, "the FPFH tests left blocks of the pool handed out"


@pytest.fixture
def case(gpu_ctx, shared, request):
    name = request.param
    if name not in shared:
        cloud, index, normals = _prepare(gpu_ctx, name)
        out = index.fpfh(fc.CASES[name]["k"])
        shared[name] = (cloud, index, normals, out, _download(out), fref.fpfh(fc.CASES[name]["points"], normals, fc.CASES[name]["k"]))
    return (name,) + shared[name]


@pytest.mark.parametrize("case", fc.ALL, indirect=True)
def test_equals_the_restatement(case):
    name, _, _, _, out, got, want = case
    n = len(fc.CASES[name]["points"])
    assert out.info() == (1, n, fc.CASES[name]["k"]) and out.k == fc.CASES[name]["k"]
    assert got["offsets"].tolist() == [0, n] and (int(got["n_target"][0]), int(got["n_finite"][0])) == (n, want["n_finite"])
    _assert_equals_reference(got["descriptors"], got["spfh_counts"], want, name)


@pytest.mark.parametrize("case", fc.ALL, indirect=True)
def test_second_run_gives_identical_bytes(case):
    name, _, index, _, _, got, _ = case
    with index.fpfh(fc.CASES[name]["k"]) as again:
        _assert_same_bytes(got, _download(again), name)


@pytest.mark.parametrize("k", (8, 20))
def test_the_mixed_batch_equals_its_members_one_call_each(gpu_ctx, k):
    """an empty index, a 1-point index, the edge scene and blob(300) in one call, the last two built by ltm_search_build_scanset: byte for byte what one call
    per index gives, equal to the restatement, and the same again on a second run"""
    parts = [fc.CASES[n]["points"] for n in fc.BATCH]
    assert [len(p) for p in parts[:2]] == [0, 1]
    pair = np.concatenate(parts[2:])
    scans = gpu_ctx.upload_scans(pair, np.array([0, len(parts[2]), len(pair)], np.uint64))
    batch_built = gpu_ctx.search_index_batch(scans)
    prepared = [_prepare(gpu_ctx, fc.BATCH[0]), _prepare(gpu_ctx, fc.BATCH[1]), _prepare(gpu_ctx, fc.BATCH[2], batch_built[0]),
                _prepare(gpu_ctx, fc.BATCH[3], batch_built[1])]
    indices = [p[1] for p in prepared]
    single = []
    for index in indices:
        with index.fpfh(k) as out:
            single.append(_download(out))
    with gpu_ctx.fpfh(indices, k) as out, gpu_ctx.fpfh(indices[::-1], k) as reverse:
        got, rev = _download(out), _download(reverse)
        assert out.info() == (4, sum(len(p) for p in parts), k)
    with gpu_ctx.fpfh(indices, k) as again:
        _assert_same_bytes(got, _download(again), "second run of the batch")
    off, roff = got["offsets"], rev["offsets"]
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    for r, (name, pts) in enumerate(zip(fc.BATCH, parts)):
        a, b = int(off[r]), int(off[r + 1])
        for key in ("descriptors", "spfh_counts"):
            assert got[key][a:b].tobytes() == single[r][key].tobytes(), f"batch record {r} ({name}): {key} differs from its own call"
            ra = int(roff[3 - r])
            assert rev[key][ra:ra + len(pts)].tobytes() == single[r][key].tobytes(), f"reversed batch, {name}: {key} differs"
        assert (int(got["n_target"][r]), int(got["n_finite"][r])) == (int(single[r]["n_target"][0]), int(single[r]["n_finite"][0]))
        _assert_equals_reference(got["descriptors"][a:b], got["spfh_counts"][a:b], fref.fpfh(pts, prepared[r][2], k), f"batch record {r} ({name})")
    for cloud, index, _ in prepared:
        index.close()
        if cloud is not None:
            cloud.free()
    scans.free()


def test_an_empty_list_gives_an_empty_set(gpu_ctx):
    with gpu_ctx.fpfh([], 10) as out:
        assert out.info() == (0, 0, 10) and out.offsets().tolist() == [0] and out.descriptors().shape == (0, 33) and len(out.n_target) == 0


def test_kernel_forms_and_counters(gpu_ctx, shared):
    gpu_ctx.fpfh_stats(reset=True)
    assert gpu_ctx.fpfh_stats() == dict(finite_points=0, distance_evaluations=0, pairs_skipped=0, lds_points=0)
    cloud, index, normals = _prepare(gpu_ctx, "blob_k16")
    for k in fc.KS:
        with index.fpfh(k):
            s = gpu_ctx.fpfh_stats(reset=True)
        assert s["finite_points"] == 300 and s["lds_points"] == (300 if k > 16 else 0), (k, s)      # registers up to 16 slots, LDS above
        assert s["distance_evaluations"] >= 300 * k and s["pairs_skipped"] == 0, (k, s)      # at least the neighbourhood of every point
    index.close()
    cloud.free()
    for name, skipped in (("coincident_500", fc.CASES["coincident_500"]["k"] * 499), ("line_normals_along", None), ("duplicates", None)):
        cloud, index, normals = _prepare(gpu_ctx, name)
        want = fref.fpfh(fc.CASES[name]["points"], normals, fc.CASES[name]["k"])["pairs_skipped"]
        with index.fpfh(fc.CASES[name]["k"]):
            s = gpu_ctx.fpfh_stats(reset=True)
        assert s["pairs_skipped"] == want > 0 and (skipped is None or want == skipped), (name, s, want)
        index.close()
        cloud.free()


@pytest.mark.parametrize("name", ("plane", "plane_k32", "non_finite_mixed", "duplicates", "k20_n19"))
def test_collecting_twice_gives_the_bytes_of_the_stored_lists(gpu_ctx, ltm, shared, monkeypatch, name):
    """a context created with LTM_FPFH_LISTS=0 never keeps the lists of the first pass: its weights collect the neighbourhoods again -- twice the distance
    evaluations, the same bytes"""
    case = fc.CASES[name]
    monkeypatch.setenv("LTM_FPFH_LISTS", "0")
    other = ltm.Context(vfov=50.0, hfov=360.0, device=0)
    monkeypatch.delenv("LTM_FPFH_LISTS")
    try:
        results, evals = [], []
        for ctx in (gpu_ctx, other):
            cloud, index, normals = _prepare(ctx, name)
            ctx.fpfh_stats(reset=True)
            with index.fpfh(case["k"]) as out:
                results.append(_download(out))
            evals.append(ctx.fpfh_stats(reset=True)["distance_evaluations"])
            index.close()
            cloud.free()
        _assert_same_bytes(results[0], results[1], name)
        assert evals[1] == 2 * evals[0] > 0, evals
        _assert_equals_reference(results[1]["descriptors"], results[1]["spfh_counts"], fref.fpfh(case["points"], normals, case["k"]), name)
    finally:
        other.close()


def test_errors_return_no_handle_and_leave_the_indices_usable(gpu_ctx, ltm):
    lib = gpu_ctx.lib
    pts = fc.CASES["plane"]["points"]
    lane = gpu_ctx.lane()
    theirs = lane.search_index(pts)
    theirs.estimate_normals(fc.NORMALS_K)
    with gpu_ctx.search_index(pts) as mine, gpu_ctx.search_index(pts) as bare:
        mine.estimate_normals(fc.NORMALS_K)
        with mine.fpfh(10) as first:
            kept = _download(first)
            gpu_ctx.synchronize()
            before = gpu_ctx.pool_live()

            def refused(handles, k):
                hs = (C.c_void_p * max(len(handles), 1))(*handles)
                out = C.c_void_p(0x1234)
                rc = lib.ltm_search_fpfh(gpu_ctx.h, len(handles), hs, k, C.byref(out))
                return rc == -1 and out.value is None

            assert refused([bare.h], 10) and refused([mine.h, bare.h], 10)      # an index without normals
            for k in (1, 65, 0, -3, 2 ** 31 - 1):
                assert refused([mine.h], k), k
            assert refused([mine.h, mine.h], 10)      # the same handle twice
            for handles in ([theirs.h], [mine.h, theirs.h], [mine.h, None]):      # a lane's index, a NULL index: wherever it stands
                assert refused(handles, 10)
            assert lib.ltm_search_fpfh(gpu_ctx.h, 1, None, 10, C.byref(C.c_void_p())) == -1
            assert lib.ltm_search_fpfh(gpu_ctx.h, 1, (C.c_void_p * 1)(mine.h), 10, None) == -1
            with pytest.raises(ltm.LtmError) as e:
                lane.fpfh([mine], 10)      # and the other way round
            assert e.value.code == -1
            assert lib.ltm_fpfh_info(lane.h, first.h, None, None, None) == -1
            gpu_ctx.synchronize()
            assert gpu_ctx.pool_live() == before, "a refused call left blocks of the pool handed out"
            # the indices are as they were: the same descriptors again, and the normals are still the ones estimated
            with mine.fpfh(10) as again:
                _assert_same_bytes(kept, _download(again), "after the refused calls")
            # estimating the normals again (another k) does not disturb the handle that exists
            mine.estimate_normals(5)
            _assert_same_bytes(kept, _download(first), "after the normals were estimated again")
            stale = first.h
        assert lib.ltm_fpfh_free(gpu_ctx.h, stale) == -1      # a freed handle is no handle
    theirs.close()
    lane.close()


def test_pool_is_back_after_free(gpu_ctx):
    pts = fc.CASES["plane"]["points"]
    with gpu_ctx.search_index(pts) as index:
        index.estimate_normals(fc.NORMALS_K)
        gpu_ctx.synchronize()
        before = gpu_ctx.pool_live()
        out = index.fpfh(10)
        gpu_ctx.synchronize()
        during = gpu_ctx.pool_live()
        assert during[0] == before[0] + 3 and during[1] > before[1]      # offsets, descriptors, SPFH words: the lists of the first pass were scratch
        out.close()
        gpu_ctx.synchronize()
        assert gpu_ctx.pool_live() == before


def test_the_device_view_is_the_block_itself(gpu_ctx):
    import torch
    pts = fc.CASES["plane"]["points"]
    with gpu_ctx.search_index(pts) as index:
        index.estimate_normals(fc.NORMALS_K)
        with index.fpfh(10) as out:
            view = out.device_view()
            assert view.shape == (len(pts), 33) and view.dtype == torch.float32 and view.is_cuda
            assert view.data_ptr() == out._device()[1]      # no copy
            assert view.cpu().numpy().tobytes() == out.descriptors().tobytes()
            d = torch.cdist(view[:8], view[:8])
            assert d.shape == (8, 8) and bool(torch.isfinite(d).all())
            del view, d
