"""ltm_fpfh_match on the device against the restatement (tools/sac_numpy.py, pinned on the CPU by tests/test_sac_cases_cpu.py), on every fixture of
tests/sac_cases.py built around the tile height the library reports, and on descriptors the device made itself.  Target rows are compared for EQUALITY and
distances bit for bit: the device's arithmetic is stated in include/ltm.h so that both sides round the same way."""
import gc

import numpy as np
import pytest

import fpfh_cases as fc
import sac_cases as sc
from tools import sac_numpy as sref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(ltm):
    return sc.match_cases(ltm.match_tile_rows())


@pytest.fixture(scope="module", autouse=True)
def pool_is_left_as_found(gpu_ctx):
    """the pool's live blocks are taken before the module's first call and compared after everything the module made has been freed"""
    gc.collect()
    gpu_ctx.synchronize()
    start = gpu_ctx.pool_live()
    yield
    gc.collect()
    gpu_ctx.synchronize()
    assert gpu_ctx.pool_live() == start, "the match tests left blocks of the pool handed out"


def _download(m):
    return dict(indices=m.indices(), distances=m.distances(), offsets=m.offsets(), n_source=m.n_source.copy(), n_target=m.n_target.copy())


def _assert_equals_reference(got, target, source, kc, what):
    idx, dist = sref.match(target, source, kc)
    assert got["indices"].dtype == np.int32 and got["indices"].shape == idx.shape and got["distances"].dtype == np.float32, what
    bad = np.flatnonzero((got["indices"] != idx).any(axis=1))
    assert bad.size == 0, f"{what}: the lists of {bad.size} of {len(source)} source rows differ, first at {bad[:3]}: {got['indices'][bad[:1]]} vs {idx[bad[:1]]}"
    assert got["distances"].tobytes() == dist.tobytes(), f"{what}: distances differ in their bits"


CASE_NAMES = list(sc.match_cases(128))      # the names do not depend on the tile height


@pytest.mark.parametrize("name", CASE_NAMES)
def test_uploaded_rows_equal_the_restatement(gpu_ctx, cases, name):
    target, source, kc = cases[name]
    with gpu_ctx.fpfh_from_rows(target) as t, gpu_ctx.fpfh_from_rows(source) as s:
        assert t.info() == (1, len(target), 0) and t.k == 0 and not t.spfh_counts().any()
        assert int(t.n_target[0]) == len(target) and int(t.n_finite[0]) == int((~np.isnan(target).any(axis=1)).sum())
        assert t.descriptors().tobytes() == target.tobytes()
        with gpu_ctx.fpfh_match(t, s, [(0, 0)], kc) as m:
            assert m.info() == (1, len(source), kc) and m.kc == kc and len(m) == 1
            got = _download(m)
        assert got["offsets"].tolist() == [0, len(source)] and (int(got["n_source"][0]), int(got["n_target"][0])) == (len(source), len(target))
        _assert_equals_reference(got, target, source, kc, name)
        with gpu_ctx.fpfh_match(t, s, [(0, 0)], kc) as again:
            second = _download(again)
        assert all(got[k].tobytes() == second[k].tobytes() for k in got), f"{name}: a second run gives other bytes"


def test_one_call_over_four_pairs_that_share_a_target_equals_the_four_single_calls(gpu_ctx, cases):
    """one target record, four source records of 0, 1, 257 and 66 rows (one with NaN rows) in ONE set, matched in one call: byte for byte the four single
    calls, and equal to the restatement.  The target is the one with NaN rows at its tile boundary"""
    target = cases["nan"][0]
    sources = [cases["ns0"][1], cases["ns1"][1], cases["ns257"][1], cases["nan"][1]]
    off = np.cumsum([0] + [len(s) for s in sources]).astype(np.uint64)
    kc = 9
    with gpu_ctx.fpfh_from_rows(target) as t, gpu_ctx.fpfh_from_rows(np.concatenate(sources), off) as s:
        assert s.info() == (4, int(off[-1]), 0)
        with gpu_ctx.fpfh_match(t, s, [(0, r) for r in range(4)], kc) as m:
            batch = _download(m)
        assert batch["offsets"].tolist() == off.tolist() and batch["n_source"].tolist() == [len(x) for x in sources] and batch["n_target"].tolist() == [len(target)] * 4
        for r in range(4):
            with gpu_ctx.fpfh_match(t, s, [(0, r)], kc) as m:
                single = _download(m)
            a, b = int(off[r]), int(off[r + 1])
            assert batch["indices"][a:b].tobytes() == single["indices"].tobytes() and batch["distances"][a:b].tobytes() == single["distances"].tobytes(), r
            _assert_equals_reference(single, target, sources[r], kc, f"pair {r}")


def test_device_made_fpfh_rows_equal_the_restatement(gpu_ctx):
    """the edge scene and the blob of tests/fpfh_cases.py as two records of ONE descriptor set made by ltm_search_fpfh, matched against each other and
    against themselves (where every row finds itself first, at distance 0, unless it is a NaN row)"""
    names = ("edge", "blob_k8")
    clouds = [gpu_ctx.upload(fc.CASES[n]["points"]) for n in names]
    indices = [gpu_ctx.search_index(c) for c in clouds]
    for i in indices:
        i.estimate_normals(fc.NORMALS_K)
    pairs = [(0, 1), (1, 0), (0, 0)]
    with gpu_ctx.fpfh(indices, 8) as f:
        rows, off = f.descriptors(), f.offsets()
        with gpu_ctx.fpfh_match(f, f, pairs, 5) as m:
            got = _download(m)
    rec = [rows[int(off[r]):int(off[r + 1])] for r in range(2)]
    assert all(len(r) > 256 for r in rec), "more than one workgroup of source rows and more than one tile of target rows"
    at = 0
    for t, s in pairs:
        part = {k: got[k][at:at + len(rec[s])] for k in ("indices", "distances")}
        _assert_equals_reference(part, rec[t], rec[s], 5, f"pair ({t}, {s})")
        at += len(rec[s])
    assert at == len(got["indices"])
    own = got["indices"][at - len(rec[0]):]
    plain = ~np.isnan(rec[0]).any(axis=1)
    assert plain.any() and (got["distances"][at - len(rec[0]):][plain, 0] == 0.0).all() and (own[~plain] == -1).all()
    for x in indices:
        x.close()
    for c in clouds:
        c.free()


def test_domain_errors_leave_no_handle(gpu_ctx, ltm):
    import ctypes as C
    rows = sc.histogram_rows(5, 1)
    live = gpu_ctx.pool_live()
    cloud = gpu_ctx.upload(np.zeros((4, 4), np.float32))
    with gpu_ctx.fpfh_from_rows(rows) as f, gpu_ctx.search_index(cloud) as index:
        rec = np.zeros(1, np.uint32)
        two = np.array([1], np.uint32)

        def call(n, tset, trec, sset, srec, kc):
            out = C.c_void_p(77)
            rc = gpu_ctx.lib.ltm_fpfh_match(gpu_ctx.h, n, tset, trec, sset, srec, kc, C.byref(out))
            assert out.value is None
            return rc

        held = gpu_ctx.pool_live()
        for kc in (0, -1, 17):
            assert call(1, f.h, rec.ctypes.data, f.h, rec.ctypes.data, kc) == -1
        assert call(1, None, rec.ctypes.data, f.h, rec.ctypes.data, 4) == -1
        assert call(1, f.h, rec.ctypes.data, index.h, rec.ctypes.data, 4) == -1, "a handle of another type"
        assert call(1, f.h, None, f.h, rec.ctypes.data, 4) == -1
        assert call(1, f.h, two.ctypes.data, f.h, rec.ctypes.data, 4) == -1, "a record number outside the set"
        assert call(1, f.h, rec.ctypes.data, f.h, two.ctypes.data, 4) == -1
        assert gpu_ctx.lib.ltm_fpfh_match(gpu_ctx.h, 1, f.h, rec.ctypes.data, f.h, rec.ctypes.data, 4, None) == -1
        lane = C.c_void_p()
        gpu_ctx._ck(gpu_ctx.lib.ltm_lane_create(gpu_ctx.h, C.byref(lane)))
        try:
            out = C.c_void_p(77)
            assert gpu_ctx.lib.ltm_fpfh_match(lane, 1, f.h, rec.ctypes.data, f.h, rec.ctypes.data, 4, C.byref(out)) == -1 and out.value is None, "a lane's context"
        finally:
            gpu_ctx.lib.ltm_destroy(lane)
        out = C.c_void_p(77)
        off = np.array([0, 3, 2], np.uint64)
        assert gpu_ctx.lib.ltm_fpfh_upload(gpu_ctx.h, 2, off.ctypes.data, rows.ctypes.data, C.byref(out)) == -1 and out.value is None
        assert gpu_ctx.pool_live() == held, "a refused call kept blocks of the pool"
        with gpu_ctx.fpfh_match(f, f, np.zeros((0, 2), np.int64), 4) as empty:      # no pairs: valid
            assert empty.info() == (0, 0, 4) and empty.indices().shape == (0, 4) and empty.offsets().tolist() == [0]
        m = gpu_ctx.fpfh_match(f, f, [(0, 0)], 4)
        raw = m.h
        m.close()
        assert gpu_ctx.lib.ltm_matches_free(gpu_ctx.h, raw) == -1, "a freed handle is refused, not dereferenced"
    cloud.free()
    gc.collect()
    assert gpu_ctx.pool_live() == live
