"""ltm_sac_align on the device against the restatement (tools/sac_numpy.py, pinned on the CPU by tests/test_sac_cases_cpu.py) on the fixtures of
tests/sac_cases.py: valid bytes, counts, the record and the transform of the best hypothesis, all for EQUALITY (T bit for bit); then the chain into ICP and
verify_loops(coarse="fpfh").  The descriptors are uploaded rows, so that both sides match the same rows; the indices are built one by one
(ltm_search_build keeps ascending index among equal codes, which the restatement's order assumes)."""
import ctypes as C
import gc

import numpy as np
import pytest

import icp_fixtures as fx
import sac_cases as sc
from tools import icp_numpy as iref
from tools import sac_numpy as sref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def block(ltm):
    return ltm.sac_block_points()


@pytest.fixture(scope="module", autouse=True)
def pool_is_left_as_found(gpu_ctx):
    gc.collect()
    gpu_ctx.synchronize()
    start = gpu_ctx.pool_live()
    yield
    gc.collect()
    gpu_ctx.synchronize()
    assert gpu_ctx.pool_live() == start, "the alignment tests left blocks of the pool handed out"


class Prepared:
    """the device side of some cases as ONE batch: clouds, indices (built one by one), uploaded rows as two descriptor sets, the matches"""

    def __init__(self, ctx, cases, kc):
        self.ctx, self.cases = ctx, cases
        self.clouds = [ctx.upload(_xyzi(c[k])) for c in cases for k in ("target", "source")]
        self.indices = [ctx.search_index(c) for c in self.clouds]
        off = lambda k: np.cumsum([0] + [len(c[k]) for c in cases]).astype(np.uint64)      # noqa: E731
        self.trows = ctx.fpfh_from_rows(np.concatenate([c["target_rows"] for c in cases]), off("target_rows"))
        self.srows = ctx.fpfh_from_rows(np.concatenate([c["source_rows"] for c in cases]), off("source_rows"))
        self.matches = ctx.fpfh_match(self.trows, self.srows, [(i, i) for i in range(len(cases))], kc)
        self.pairs = [(self.indices[2 * i], self.indices[2 * i + 1]) for i in range(len(cases))]

    def align(self, **params):
        with self.ctx.sac_align(self.pairs, self.matches, **params) as a:
            return dict(found=a.found.copy(), best=a.best.copy(), consensus=a.consensus.copy(), n_valid=a.n_valid.copy(), n_prerejected=a.n_prerejected.copy(),
                        n_eval=a.n_eval.copy(), T=a.T.copy(), hyp_counts=a.hypothesis_counts(), hyp_valid=a.hypothesis_valid(), info=a.info())

    def close(self):
        for h in [self.matches, self.trows, self.srows] + self.indices:
            h.close()
        for c in self.clouds:
            c.free()


def _xyzi(p):
    return np.concatenate([p, np.zeros((len(p), 1), np.float32)], axis=1) if len(p) else np.zeros((0, 4), np.float32)


def _assert_equals_reference(got, i, want, what):
    assert got["hyp_valid"][i].tolist() == want["hyp_valid"].tolist(), f"{what}: valid bytes differ"
    bad = np.flatnonzero(got["hyp_counts"][i] != want["hyp_counts"])
    assert bad.size == 0, f"{what}: the counts of {bad.size} hypotheses differ, first at {bad[:3]}: {got['hyp_counts'][i][bad[:3]]} vs {want['hyp_counts'][bad[:3]]}"
    for k in ("n_valid", "n_prerejected", "best", "consensus", "n_eval", "found"):
        assert int(got[k][i]) == int(want[k]), f"{what}: {k} {int(got[k][i])} vs {int(want[k])}"
    T = got["T"][i]
    if want["best"] < 0:
        assert np.isnan(T).all(), f"{what}: T of a record without a valid hypothesis must be NaN"
    else:
        assert T.tobytes() == np.ascontiguousarray(want["T"], np.float64).tobytes(), f"{what}: T differs in its bits:\n{T}\nvs\n{want['T']}"
        assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]


CASE_NAMES = list(sc.sac_cases(1024))      # the names do not depend on the block


@pytest.mark.parametrize("name", CASE_NAMES)
def test_equals_the_restatement(gpu_ctx, block, name):
    case = sc.sac_cases(block)[name]
    idx, _, want = sc.restated(name, block)
    prep = Prepared(gpu_ctx, [case], case["kc"])
    try:
        assert prep.matches.indices().tolist() == idx.tolist(), "the matches are those of the restatement"
        got = prep.align(**case["params"])
        assert got["info"] == (1, case["params"]["max_iterations"])
        _assert_equals_reference(got, 0, want, name)
        again = prep.align(**case["params"])
        assert all(got[k].tobytes() == again[k].tobytes() for k in got if k != "info"), f"{name}: a second run gives other bytes"
    finally:
        prep.close()


def test_a_mixed_batch_equals_the_single_calls(gpu_ctx, block):
    """six records of mixed sizes under one parameter set, two of them sharing nothing and one with an empty source: byte for byte the single calls,
    equal to the restatement, and the same bytes on a second run"""
    cases = [sc.sac_cases(block)[n] for n in sc.BATCH]
    params = dict(inlier_distance=1.0, max_iterations=70, seed=9, similarity_threshold=0.2, inlier_fraction=0.25, eval_stride=2)
    prep = Prepared(gpu_ctx, cases, 3)
    try:
        batch = prep.align(**params)
        assert batch["info"] == (len(cases), 70)
        again = prep.align(**params)
        assert all(batch[k].tobytes() == again[k].tobytes() for k in batch if k != "info")
    finally:
        prep.close()
    for i, (name, case) in enumerate(zip(sc.BATCH, cases)):
        single = Prepared(gpu_ctx, [case], 3)
        try:
            got = single.align(**params)
        finally:
            single.close()
        for k in got:
            if k != "info":
                assert got[k][0].tobytes() == batch[k][i].tobytes(), f"{name}: {k} of the batch differs from the single call"
        idx, _ = sref.match(case["target_rows"], case["source_rows"], 3)
        _assert_equals_reference(batch, i, sref.align(case["target"], case["source"], idx, **params), name)


def test_one_index_may_serve_many_pairs(gpu_ctx, block):
    """the same target and source indices listed for two pairs of one call (their row tables are made once): both records are the single call's"""
    case = sc.sac_cases(block)["far"]
    prep = Prepared(gpu_ctx, [case], 3)
    try:
        one = prep.align(**case["params"])
        with gpu_ctx.fpfh_match(prep.trows, prep.srows, [(0, 0), (0, 0)], 3) as m, gpu_ctx.sac_align(prep.pairs * 2, m, **case["params"]) as a:
            assert a.T[0].tobytes() == a.T[1].tobytes() == one["T"][0].tobytes() and a.hypothesis_counts().tolist() == [one["hyp_counts"][0].tolist()] * 2
    finally:
        prep.close()


def test_the_counters_show_prerejection_and_the_early_ending_walk(gpu_ctx, block):
    case = sc.sac_cases(block)["far"]
    want = sc.restated("far", block)[2]
    prep = Prepared(gpu_ctx, [case], 3)
    try:
        gpu_ctx.sac_stats(reset=True)
        prep.align(**case["params"])
        stats = gpu_ctx.sac_stats(reset=True)
    finally:
        prep.close()
    assert stats["prerejected"] == want["n_prerejected"] > 0
    assert stats["early_hits"] == int(want["hyp_counts"].sum()) > 0, "every inlier is a walk that ended at its first hit"
    assert stats["inlier_tests"] == want["n_eval"] * want["n_valid"] and stats["records"] == 1
    assert gpu_ctx.sac_stats() == dict(inlier_tests=0, prerejected=0, early_hits=0, records=0)


def test_domain_errors_leave_no_handle(gpu_ctx, ltm, block):
    case = sc.sac_cases(block)["far"]
    prep = Prepared(gpu_ctx, [case], 3)
    try:
        held = gpu_ctx.pool_live()
        t, s = (C.c_void_p * 1)(prep.pairs[0][0].h), (C.c_void_p * 1)(prep.pairs[0][1].h)

        def call(n=1, targets=t, sources=s, matches=prep.matches.h, ctx=gpu_ctx.h, null_params=False, **over):
            p = ltm.sac_params(**dict(case["params"]))
            for k, v in over.items():
                setattr(p, k, v)
            out = C.c_void_p(77)
            rc = gpu_ctx.lib.ltm_sac_align(ctx, n, targets, sources, matches, None if null_params else C.byref(p), C.byref(out))
            assert out.value is None
            return rc

        assert call(null_params=True) == -1 and call(targets=None) == -1 and call(sources=None) == -1 and call(matches=None) == -1
        assert call(n=2, targets=(C.c_void_p * 2)(t[0], t[0]), sources=(C.c_void_p * 2)(s[0], s[0])) == -1, "n_pairs is not the match handle's"
        assert call(n=0) == -1
        assert call(targets=s, sources=t) == -1, "an index whose points are not the rows of its match record"
        assert call(targets=(C.c_void_p * 1)(None)) == -1 and call(matches=prep.trows.h) == -1
        for over in (dict(max_iterations=0), dict(max_iterations=16385), dict(similarity_threshold=1.0), dict(similarity_threshold=-0.1),
                     dict(similarity_threshold=float("nan")), dict(inlier_distance=0.0), dict(inlier_distance=float("inf")), dict(inlier_distance=float("nan")),
                     dict(inlier_fraction=1.5), dict(inlier_fraction=float("nan")), dict(eval_stride=0)):
            assert call(**over) == -1, over
        lane = C.c_void_p()
        gpu_ctx._ck(gpu_ctx.lib.ltm_lane_create(gpu_ctx.h, C.byref(lane)))
        try:
            assert call(ctx=lane) == -1, "a lane's context"
        finally:
            gpu_ctx.lib.ltm_destroy(lane)
        assert gpu_ctx.pool_live() == held, "a refused call kept blocks of the pool"
        with pytest.raises(ValueError):
            gpu_ctx.sac_align(prep.pairs, prep.matches)      # inlier_distance has no usable default
        with gpu_ctx.fpfh_match(prep.trows, prep.srows, np.zeros((0, 2), np.int64), 3) as m0, gpu_ctx.sac_align([], m0, inlier_distance=1.0) as a0:
            assert a0.info() == (0, 1000) and a0.T.shape == (0, 4, 4) and a0.hypothesis_counts().shape == (0, 1000)
    finally:
        prep.close()


def test_sac_then_icp_ends_where_the_restatements_chain_ends(gpu_ctx):
    """the well-posed pair (30 degrees, 3 m): sac_align's T is the restatement's bit for bit, and icp_align(init=T) ends within icp_fixtures.tol_T of
    tools/icp_numpy.align started from the restatement's T -- where identity does not lead"""
    w = sc.well_posed()
    case = dict(target=w["target"], source=w["source"], target_rows=w["target_rows"], source_rows=w["source_rows"])
    prep = Prepared(gpu_ctx, [case], sc.WELL_POSED["kc"])
    try:
        got = prep.align(**sc.WELL_POSED["sac"])
        _assert_equals_reference(got, 0, w["align"], "well posed")
        assert got["found"][0] == 1 and int(got["consensus"][0]) == sc.WELL_POSED_CONSENSUS
        res = gpu_ctx.icp_align([(prep.pairs[0][0], _xyzi(w["source"]))], init=got["T"], **sc.WELL_POSED["icp"])
        cold = gpu_ctx.icp_align([(prep.pairs[0][0], _xyzi(w["source"]))], **sc.WELL_POSED["icp"])
    finally:
        prep.close()
    want = iref.align(w["target"], w["source"], init=w["align"]["T"], **sc.WELL_POSED["icp"])
    assert res["converged"][0] == want["converged"] == 1
    assert np.abs(res["T"][0].reshape(4, 4) - want["T"]).max() <= fx.tol_T(len(w["source"]))
    assert sc.displacement(cold["T"][0].reshape(4, 4), want["T"], w["source"]) > sc.WELL_POSED["sac"]["inlier_distance"]


def test_verify_loops_with_coarse_fpfh_accepts_the_moved_pair_that_it_rejects_without(gpu_ctx):
    """two scan sets of one keyframe each, the well-posed pair: normals, FPFH, matches, sac and ICP all on the device.  Without the coarse step ICP starts
    from identity, far outside its basin, and the pair is rejected; with it the pair is accepted and ends within the fixture's noise of where the
    restatement's ICP ends from the ground truth"""
    w = sc.well_posed()
    tscans = gpu_ctx.upload_scans(_xyzi(w["target"]), np.array([0, len(w["target"])], np.uint64))
    sscans = gpu_ctx.upload_scans(_xyzi(w["source"]), np.array([0, len(w["source"])], np.uint64))
    try:
        kw = dict(search_num=0, leaf=0.0, **sc.WELL_POSED["icp"])
        plain, ok_plain = gpu_ctx.verify_loops(tscans, sscans, [(0, 0)], **kw)
        coarse, ok_coarse = gpu_ctx.verify_loops(tscans, sscans, [(0, 0)], coarse="fpfh", fpfh_k=sc.WELL_POSED["fpfh_k"], match_k=sc.WELL_POSED["kc"],
                                                 sac=sc.WELL_POSED["sac"], **kw)
    finally:
        tscans.free()
        sscans.free()
    want = iref.align(w["target"], w["source"], init=w["GT"], **sc.WELL_POSED["icp"])
    assert not ok_plain[0] and ok_coarse[0]
    assert sc.displacement(coarse["T"][0].reshape(4, 4), want["T"], w["source"]) < sc.WELL_POSED["noise"]
    assert sc.displacement(plain["T"][0].reshape(4, 4), want["T"], w["source"]) > sc.WELL_POSED["sac"]["inlier_distance"]


def test_verify_loops_keeps_the_given_start_of_a_pair_the_coarse_step_does_not_find(gpu_ctx):
    """inlier_fraction = 1 cannot be met, so no pair is `found`: the pair then starts from the init the caller gave (the ground truth: accepted), and from
    identity without one (rejected, as without the coarse step)"""
    w = sc.well_posed()
    tscans = gpu_ctx.upload_scans(_xyzi(w["target"]), np.array([0, len(w["target"])], np.uint64))
    sscans = gpu_ctx.upload_scans(_xyzi(w["source"]), np.array([0, len(w["source"])], np.uint64))
    try:
        kw = dict(search_num=0, leaf=0.0, coarse="fpfh", fpfh_k=sc.WELL_POSED["fpfh_k"], match_k=sc.WELL_POSED["kc"],
                  sac=dict(sc.WELL_POSED["sac"], inlier_fraction=1.0, max_iterations=50), **sc.WELL_POSED["icp"])
        _, ok_given = gpu_ctx.verify_loops(tscans, sscans, [(0, 0)], init=w["GT"][None], **kw)
        _, ok_none = gpu_ctx.verify_loops(tscans, sscans, [(0, 0)], **kw)
    finally:
        tscans.free()
        sscans.free()
    assert ok_given[0] and not ok_none[0]
