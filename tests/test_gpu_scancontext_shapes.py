"""Scan Context on the device at the shapes, database sizes and ties the default 20 x 60 tests do not reach: every case of tests/sc_cases.py (which
tests/test_sc_cases_cpu.py shows to be well-posed and to reach its branch) through ScanContexts.distance / ScanContexts.detect and, for the descriptor
cases, ltm_sc_from_scanset, against the numpy restatement tools/sc_numpy.py.  Shifts and indices must be equal, yaw_diff_rad bitwise equal, distances
within 1e-12 of the restatement (the bound of tests/test_gpu_scancontext.py; device and restatement add in the same order, so the printed maxima are
expected to be zero or a few ulps), and the context's pool holds after every family what it held before.

Measured on the MI355X: max |dist - restatement| is 0.0 at every shape and search_ratio of the pair family, max |min_dist - restatement| is 0.0 in
every detect case, and the descriptors are equal bit for bit (ring and sector keys of the existing descriptor test: 0 ulp, 0.0)."""
import numpy as np
import pytest

import sc_cases as sc
from tools import sc_numpy as ref

pytestmark = pytest.mark.gpu

TOL = 1e-12      # tests/test_gpu_scancontext.py: test_pair_distance_and_shift, check_detect


@pytest.fixture
def pool(gpu_ctx):
    before = gpu_ctx.pool_live()
    yield
    assert gpu_ctx.pool_live() == before


def sets_of(gpu_ctx, p, *arrays):
    return [gpu_ctx.scan_contexts_from(a, num_ring=p["num_ring"], num_sector=p["num_sector"]) for a in arrays]


def check_detect(got, want, what):
    for k in ("loop_id", "nn_idx", "nn_align"):
        assert (got[k] == want[k]).all(), (what, k, got[k].tolist(), want[k].tolist())
    assert np.abs(got["min_dist"] - want["min_dist"]).max() <= TOL, (what, got["min_dist"].tolist(), want["min_dist"].tolist())
    assert (got["yaw_diff_rad"].view(np.uint32) == want["yaw_diff_rad"].view(np.uint32)).all(), what
    return float(np.abs(got["min_dist"] - want["min_dist"]).max())


def run_detect_case(gpu_ctx, c):
    db, qs = sets_of(gpu_ctx, c["p"], c["db"], c["queries"])
    worst = 0.0
    try:
        for run in c["runs"]:
            got = db.detect(qs, num_candidates=run["num_candidates"], search_ratio=run["search_ratio"], dist_thres=c["p"]["dist_thres"])
            worst = max(worst, check_detect(got, run["want"], (c["name"], run["num_candidates"], run["search_ratio"])))
    finally:
        db.close()
        qs.close()
    print(c["name"], "max |min_dist - restatement|", worst)


# ------------------------------------------------------------------ pair distance and shift
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_distance_and_shift_at_shape(gpu_ctx, pool, shape):
    c = sc.shape_case(*shape)
    a, b = sets_of(gpu_ctx, c["p"], c["copies"], c["base"])
    worst = 0.0
    try:
        for run in c["runs"]:
            dist, shift = a.distance(b, c["pairs"], search_ratio=run["search_ratio"])
            err = float(np.abs(dist - run["dist"]).max())
            worst = max(worst, err)
            print(c["name"], "ratio", run["search_ratio"], "max |dist - restatement|", err)
            assert (shift == run["shift"]).all(), (run["search_ratio"], np.nonzero(shift != run["shift"])[0][:5], shift.tolist(), run["shift"].tolist())
            assert err <= TOL, (run["search_ratio"], err)
            assert (shift[:sc.N_BASE] == c["rots"]).all() and (dist[:sc.N_BASE] < 0.01).all()      # the copies are found at their rotation
    finally:
        a.close()
        b.close()
    print(c["name"], "max |dist - restatement| over the ratios", worst)


def test_one_by_one_known_answers(gpu_ctx, pool):
    c = sc.one_by_one_case()
    (s,) = sets_of(gpu_ctx, c["p"], c["descs"])
    try:
        for ratio in (0.0, 0.1, 1.0):
            dist, shift = s.distance(s, c["pairs"], search_ratio=ratio)
            assert (shift == c["shift"]).all() and (dist == c["dist"]).all(), (ratio, dist.tolist(), shift.tolist())
    finally:
        s.close()


# ------------------------------------------------------------------ detect
@pytest.mark.parametrize("shape", sc.DETECT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("nd", sc.CANDIDATE_ND)
def test_detect_candidates_with_exact_ties(gpu_ctx, pool, shape, nd):
    run_detect_case(gpu_ctx, sc.candidate_case(*shape, nd))


@pytest.mark.parametrize("shape", sc.DETECT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_detect_exhaustive_past_64_entries(gpu_ctx, pool, shape):
    run_detect_case(gpu_ctx, sc.exhaustive_case(*shape))


@pytest.mark.parametrize("order", [(3, 7), (7, 3)], ids=["nan-first", "inf-first"])
def test_detect_orders_nan_after_inf_key_distances(gpu_ctx, pool, order):
    """include/ltm.h: "a NaN key distance sorts last" -- after a +inf one too, whatever the indices"""
    run_detect_case(gpu_ctx, sc.nonfinite_case(*order))


# ------------------------------------------------------------------ descriptors from scans
def check_descriptors(gpu_ctx, c):
    p = c["p"]
    R, S = p["num_ring"], p["num_sector"]
    n_kf, kb = len(c["offsets"]) - 1, c["kf_begin"]
    want = np.zeros((n_kf, R, S))
    want[c["nonempty"]] = c["want"]
    want = want[kb:]
    g = gpu_ctx.upload_scans(c["scans"], c["offsets"])
    try:
        with gpu_ctx.scan_contexts(g, kf_begin=kb, num_ring=R, num_sector=S) as s:
            assert s.info() == (n_kf - kb, R, S)
            desc, rk, sk = s.download()
    finally:
        g.free()
    bad = np.argwhere(desc.view(np.uint64) != want.view(np.uint64))                        # the whole array, zeros included
    assert len(bad) == 0, f"{c['name']}: {len(bad)} bins differ, first (kf, ring, sector) {bad[:5].tolist()}"
    full = c["nonempty"][c["nonempty"] >= kb] - kb
    want_rk = np.stack([ref.ring_key(want[k]) for k in full])
    want_sk = np.stack([ref.sector_key(want[k]) for k in full])
    assert (np.abs(rk[full].astype(np.float64) - want_rk.astype(np.float64)) <= np.spacing(np.abs(want_rk))).all()      # as test_descriptors_bitwise_and_keys
    assert np.abs(sk[full] - want_sk).max() <= 1e-12
    empty = np.ones(n_kf - kb, bool)
    empty[full] = False
    assert (rk[empty] == 0).all() and (sk[empty] == 0).all()


@pytest.mark.parametrize("kf_begin", [0, 3])
def test_descriptors_of_more_than_65535_keyframes(gpu_ctx, pool, kf_begin):
    check_descriptors(gpu_ctx, sc.many_keyframes_case(kf_begin))


@pytest.mark.parametrize("shape", sc.BLOCK_EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_descriptors_either_side_of_the_scatter_lds_limit(gpu_ctx, pool, shape):
    check_descriptors(gpu_ctx, sc.block_edge_case(*shape))
