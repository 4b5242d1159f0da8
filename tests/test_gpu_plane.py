"""ltm_scanset_segment_planes / ltm_cloud_segment_plane on the device against the restatement (tools/plane_numpy.py, pinned on the CPU by
tests/test_plane_cases_cpu.py), on every fixture of tests/plane_cases.py.  The hypothesis-count matrix, the valid bytes, found / best / consensus / n_valid are
integers decided by + - x in double: compared for EQUALITY.  The labels are compared for equality with the restatement's label expression evaluated at the
DEVICE's coefficients and plane point (no square root, no division).  Only the coefficients and the plane point carry a tolerance, the measured one:
tests/test_plane_cases_cpu.py sums the moments in the fixed shape and in three random orders and takes the largest difference over the fixtures (refined:
4.441e-16; unrefined, against numpy's own normalisation: 8.882e-16); 100 x that for the Jacobi sweep order and the final normalisation."""
import gc
import hashlib
import math

import numpy as np
import pytest

import plane_cases as pc
from tools import plane_numpy as pref

pytestmark = pytest.mark.gpu

MEASURED_REFINED = 4.441e-16
MEASURED_UNREFINED = 8.882e-16
COEFF_TOL_REFINED = 100.0 * MEASURED_REFINED
COEFF_TOL_UNREFINED = 100.0 * MEASURED_UNREFINED

# sha256 of ltm_search_estimate_normals' output on normals_cases.sphere() (as XYZI, intensity 0), viewpoint (0.5, -1, 20), taken on the commit before the
# Jacobi routine moved to ltm_covariance.h: k = 16 (lists in registers), k = 17 (lists in LDS)
NORMALS_CLOUD_SHA256 = "437a6d9c115825ea43cdc22af6aeb8fabe97367e22e2cadcf11ec8a1ded7d030"
NORMALS_SHA256 = {16: "2a3f3366fe2648d40287d4e6c3244d1049fc1e560803b6beb279673596966327", 17: "46aa1fbe635ec848c2fdb775dd0cff77841362af05f8e1db7b95fc47949212ad"}


def _segment(ctx, scans, p, kf_begin=0, kf_end=None):
    return ctx.segment_planes(scans, p["distance_threshold"], p["max_iterations"], p["axis"], p["eps_angle"], p["seed"], p["refine"], kf_begin, kf_end)


def _download(pl):
    """everything a plane set holds, as host arrays"""
    return dict(found=pl.found.copy(), best=pl.best.copy(), consensus=pl.consensus.copy(), n_valid=pl.n_valid.copy(), n_inliers=pl.n_inliers.copy(),
                refined=pl.refined.copy(), coeff=pl.coefficients.copy(), point=pl.points.copy(), labels=pl.labels(), counts=pl.hypothesis_counts(),
                valid=pl.hypothesis_valid())


def _upload(ctx, clouds):
    off = np.cumsum([0] + [len(c) for c in clouds]).astype(np.uint64)
    return ctx.upload_scans(np.concatenate(clouds) if clouds else np.zeros((0, 4), np.float32), off), off


def _run(ctx, name):
    pts, p = pc.CASES[name]
    scans, _ = _upload(ctx, [pts])
    pl = _segment(ctx, scans, p)
    return scans, pl, _download(pl)


@pytest.fixture(scope="module", autouse=True)
def shared(gpu_ctx):
    """what the parametrised tests share: (scan set, plane set, downloads) per fixture, made on first use.  The pool's live blocks are taken before the
    module's first call and compared after everything the module made has been freed."""
    gc.collect()
    gpu_ctx.synchronize()
    start = gpu_ctx.pool_live()
    cache = {}
    yield cache
    for scans, pl, _ in cache.values():
        pl.close()
        scans.free()
    cache.clear()
    gc.collect()
    gpu_ctx.synchronize()
    assert gpu_ctx.pool_live() == start, "the plane tests left blocks of the pool handed out"


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


def _record(got, k, n0, n1):
    """record k of a batch download as the download of a single call"""
    out = {key: got[key][k:k + 1] for key in ("found", "best", "consensus", "n_valid", "n_inliers", "refined", "coeff", "point", "counts", "valid")}
    out["labels"] = got["labels"][n0:n1]
    return out


def _assert_equals_reference(got, want, pts, p, what):
    """one record against the restatement"""
    H = p["max_iterations"]
    assert got["counts"].dtype == np.uint32 and got["counts"].shape == (1, H) and got["valid"].dtype == np.uint8 and got["valid"].shape == (1, H)
    assert (got["valid"][0] == want["valid"]).all(), f"{what}: valid bytes differ from the restatement"
    assert (got["counts"][0] == want["counts"]).all(), f"{what}: hypothesis counts differ from the restatement"
    assert not got["counts"][0][want["valid"] == 0].any()
    for key in ("found", "best", "consensus", "n_valid"):
        assert int(got[key][0]) == int(want[key]), f"{what}: {key} {got[key][0]} vs {want[key]}"
    assert got["labels"].dtype == np.uint8 and got["labels"].shape == (len(pts),)
    assert int(got["n_inliers"][0]) == int(got["labels"].sum()), f"{what}: n_inliers is not the label sum"
    if not want["found"]:
        assert np.isnan(got["coeff"]).all() and np.isnan(got["point"]).all() and not got["labels"].any() and got["refined"][0] == 0 and got["best"][0] == -1
        return
    # labels: the restatement's expression at the device's own coefficients and plane point
    assert (got["labels"] == pref.labels(pts, got["coeff"][0], got["point"][0], p["distance_threshold"])).all(), f"{what}: labels differ"
    assert int(got["refined"][0]) == int(want["refined"]), f"{what}: refined flag"
    tol = COEFF_TOL_REFINED if want["refined"] else COEFF_TOL_UNREFINED
    err = max(float(np.abs(got["coeff"][0] - want["coeff"]).max()), float(np.abs(got["point"][0] - want["point"]).max()))
    print(f"{what}: consensus {want['consensus']}, inliers {int(got['n_inliers'][0])}, refined {want['refined']}, coefficient error {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol, f"{what}: coefficients or plane point off by {err:.3e}, tolerance {tol:.3e}"
    assert abs(float(np.dot(got["coeff"][0, :3], got["coeff"][0, :3])) - 1.0) < 1e-14


@pytest.mark.parametrize("case", list(pc.CASES), indirect=True)
def test_equals_the_restatement(case):
    name, _, pl, got = case
    pts, p = pc.CASES[name]
    assert pl.info() == (1, len(pts), p["max_iterations"])
    _assert_equals_reference(got, pc.reference(name), pts, p, name)


@pytest.mark.parametrize("case", list(pc.CASES), indirect=True)
def test_second_run_and_the_cloud_form_give_identical_bytes(gpu_ctx, case):
    name, scans, _, got = case
    pts, p = pc.CASES[name]
    with _segment(gpu_ctx, scans, p) as again:
        _assert_same_bytes(got, _download(again), name)
    with gpu_ctx.segment_plane(pts, p["distance_threshold"], p["max_iterations"], p["axis"], p["eps_angle"], p["seed"], p["refine"]) as one:
        _assert_same_bytes(got, _download(one), name + " as a cloud")


@pytest.mark.parametrize("case", list(pc.CASES), indirect=True)
def test_split_returns_inliers_and_rest_in_order(gpu_ctx, case):
    name, scans, pl, got = case
    pts = pc.CASES[name][0]
    inl, rest = pl.split(scans)
    a, off_a = inl.download()
    b, off_b = rest.download()
    inl.free()
    rest.free()
    lab = got["labels"].astype(bool)
    assert off_a.tolist() == [0, int(got["n_inliers"][0])] and off_b.tolist() == [0, len(pts) - int(got["n_inliers"][0])]
    assert a.tobytes() == np.ascontiguousarray(pts[lab]).tobytes() and b.tobytes() == np.ascontiguousarray(pts[~lab]).tobytes()
    merged = np.empty_like(pts)
    merged[lab], merged[~lab] = a, b
    assert merged.tobytes() == pts.tobytes()      # together they are the scan, in order


def test_split_refuses_another_scan_set_and_the_cloud_twin_works(gpu_ctx, shared, ltm):
    name = "plane_noise"
    if name not in shared:
        shared[name] = _run(gpu_ctx, name)
    scans, pl, got = shared[name]
    pts, p = pc.CASES[name]
    other, _ = _upload(gpu_ctx, [pts[:-1]])
    two, _ = _upload(gpu_ctx, [pts[:600], pts[600:]])
    cloud = gpu_ctx.upload(pts)
    live = gpu_ctx.pool_live()
    for bad in (other, two, cloud):      # another point count, other keyframes, and a handle of a scan set is not split as a cloud
        with pytest.raises(ltm.LtmError) as e:
            pl.split(bad)
        assert e.value.code == -1
        assert gpu_ctx.pool_live() == live
    with gpu_ctx.segment_plane(cloud, p["distance_threshold"], p["max_iterations"], p["axis"], p["eps_angle"], p["seed"], p["refine"]) as one:
        a, b = one.split(cloud)
        lab = got["labels"].astype(bool)
        assert a.download().tobytes() == np.ascontiguousarray(pts[lab]).tobytes() and b.download().tobytes() == np.ascontiguousarray(pts[~lab]).tobytes()
        a.free()
        b.free()
        with pytest.raises(ltm.LtmError) as e:
            one.split(scans)
        assert e.value.code == -1
    for h in (other, two, cloud):
        h.free()


def test_the_rest_of_the_ground_split_finds_the_wall(gpu_ctx, shared):
    name = "wall_and_ground_axis"
    if name not in shared:
        shared[name] = _run(gpu_ctx, name)
    scans, pl, got = shared[name]
    pts = pc.CASES[name][0]
    p_free = pc.CASES["wall_and_ground"][1]
    ground, rest = pl.split(scans)
    assert got["coeff"][0, 2] > 0.99 and abs(got["coeff"][0, 3] - 1.9) < 0.05      # the ground z = -1.9, normal towards the axis
    with _segment(gpu_ctx, rest, p_free) as second:
        g2 = _download(second)
        rest_pts = rest.download()[0]
        _assert_equals_reference(g2, pref.segment(rest_pts, p_free), rest_pts, p_free, "rest of the ground split")
        assert abs(g2["coeff"][0, 0]) > 0.99 and abs(g2["coeff"][0, 3] + 8.0) < 0.05 and g2["consensus"][0] > 1900      # the wall x = 8
        wall, clutter = second.split(rest)
        assert wall.info()[1] == g2["n_inliers"][0] and ground.info()[1] + wall.info()[1] + clutter.info()[1] == len(pts)
        wall.free()
        clutter.free()
    ground.free()
    rest.free()


BATCH_POOL = ["plane_noise", "empty", "size_257", "all_nonfinite", "wall_and_ground", "three_points", "one_point", "nonfinite_mixed", "collinear",
              "size_2049", "equal_support"]


@pytest.mark.parametrize("n_kf", [1, 2, 65])
def test_batch_equals_single_calls(gpu_ctx, n_kf):
    """keyframes of one scan set, empty ones among them and one scan present twice (the pool repeats): every record has the bytes of its single call"""
    names = [BATCH_POOL[k % len(BATCH_POOL)] for k in range(n_kf)]
    p = pref.params(0.08, 100, axis=(0.1, 0.0, 1.0), eps_angle=math.radians(40.0), seed=3)
    scans, off = _upload(gpu_ctx, [pc.CASES[n][0] for n in names])
    singles = {}
    for name in set(names):
        pts = pc.CASES[name][0]
        one_scan, _ = _upload(gpu_ctx, [pts])
        with _segment(gpu_ctx, one_scan, p) as one:
            singles[name] = _download(one)
        one_scan.free()
        _assert_equals_reference(singles[name], pref.segment(pts, p), pts, p, f"{name} alone")
    with _segment(gpu_ctx, scans, p) as batch:
        assert batch.info() == (n_kf, int(off[-1]), 100)
        got = _download(batch)
        for k, name in enumerate(names):
            _assert_same_bytes(singles[name], _record(got, k, int(off[k]), int(off[k + 1])), f"{name} as keyframe {k} of {n_kf}")
        inl, rest = batch.split(scans)
        assert np.diff(inl.offsets().astype(np.int64)).tolist() == got["n_inliers"].tolist()
        assert (inl.offsets() + rest.offsets() == off).all()
        inl.free()
        rest.free()
    if n_kf > 4:      # a sub-range: records kf_begin .. kf_end - 1, the same bytes; and the empty range
        kb, ke = 3, n_kf - 7
        with _segment(gpu_ctx, scans, p, kb, ke) as part:
            assert part.info() == (ke - kb, int(off[ke] - off[kb]), 100)
            gp = _download(part)
            for k in range(kb, ke):
                _assert_same_bytes(singles[names[k]], _record(gp, k - kb, int(off[k] - off[kb]), int(off[k + 1] - off[kb])), f"keyframe {k} of the sub-range")
            inl, rest = part.split(scans)
            assert np.diff(inl.offsets().astype(np.int64)).tolist() == gp["n_inliers"].tolist() and inl.n_kf == ke - kb
            inl.free()
            rest.free()
        with _segment(gpu_ctx, scans, p, 5, 5) as none:
            assert none.info() == (0, 0, 100) and none.labels().shape == (0,) and none.hypothesis_counts().shape == (0, 100) and len(none.found) == 0
            inl, rest = none.split(scans)
            assert inl.info() == (0, 0) and rest.info() == (0, 0)
            inl.free()
            rest.free()
    scans.free()


def test_errors_return_no_handle_and_leave_the_pool_as_it_was(gpu_ctx, ltm):
    C = ltm.C
    gpu_ctx.synchronize()
    before = gpu_ctx.pool_live()
    pts = pc.CASES["size_257"][0]
    lane = gpu_ctx.lane()
    try:
        mine, _ = _upload(gpu_ctx, [pts, pts])
        foreign, _ = _upload(lane, [pts])
        for _ in range(64):      # a lane's handle is a number of its own context: take one that this context does not happen to use
            if gpu_ctx.lib.ltm_scanset_info(gpu_ctx.h, foreign.h, None, None) != 0:
                break
            more, _ = _upload(lane, [pts])
            foreign.free()
            foreign = more
        foreign_cloud = lane.upload(pts)
        live = gpu_ctx.pool_live()
        p = ltm.plane_params(0.1)

        def refused(call):
            out = C.c_void_p(0x1234)
            assert call(out) == -1 and out.value is None      # LTM_E_INVALID, and no handle
            assert gpu_ctx.pool_live() == live

        refused(lambda out: gpu_ctx.lib.ltm_scanset_segment_planes(gpu_ctx.h, foreign.h, 0, 1, C.byref(p), C.byref(out)))      # a lane's scan set
        if gpu_ctx.lib.ltm_cloud_size(gpu_ctx.h, foreign_cloud.h, C.byref(C.c_size_t())) != 0:
            refused(lambda out: gpu_ctx.lib.ltm_cloud_segment_plane(gpu_ctx.h, foreign_cloud.h, C.byref(p), C.byref(out)))
        refused(lambda out: gpu_ctx.lib.ltm_scanset_segment_planes(gpu_ctx.h, mine.h, 0, 1, None, C.byref(out)))
        refused(lambda out: gpu_ctx.lib.ltm_scanset_segment_planes(gpu_ctx.h, mine.h, 2, 1, C.byref(p), C.byref(out)))
        refused(lambda out: gpu_ctx.lib.ltm_scanset_segment_planes(gpu_ctx.h, mine.h, 0, 3, C.byref(p), C.byref(out)))
        nan, inf = float("nan"), float("inf")
        z3, up = (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)
        for thr, it, axis, eps in ((0.0, 128, z3, 0.0), (-1.0, 128, z3, 0.0), (nan, 128, z3, 0.0), (inf, 128, z3, 0.0), (0.1, 0, z3, 0.0), (0.1, 4097, z3, 0.0),
                                   (0.1, 128, (nan, 0.0, 1.0), 0.0), (0.1, 128, (0.0, inf, 0.0), 0.0), (0.1, 128, up, -0.1), (0.1, 128, up, nan), (0.1, 128, up, inf)):
            q = ltm.PlaneParams(thr, it, 0, (C.c_double * 3)(*axis), eps, 1)
            refused(lambda out: gpu_ctx.lib.ltm_scanset_segment_planes(gpu_ctx.h, mine.h, 0, 2, C.byref(q), C.byref(out)))
        assert gpu_ctx.lib.ltm_scanset_segment_planes(gpu_ctx.h, mine.h, 0, 2, C.byref(p), None) == -1
        assert gpu_ctx.pool_live() == live
        # eps_angle >= pi / 2 means unconstrained, and without an axis eps_angle is not looked at
        with gpu_ctx.segment_planes(mine, 0.05, 96, axis=up, eps_angle=2.0) as wide, gpu_ctx.segment_planes(mine, 0.05, 96) as free:
            assert (wide.hypothesis_valid() == free.hypothesis_valid()).all() and (wide.hypothesis_counts() == free.hypothesis_counts()).all()
            assert (np.abs(wide.coefficients) == np.abs(free.coefficients)).all() and (wide.coefficients[:, 2] > 0).all()
            with pytest.raises(ltm.LtmError) as e:      # a plane set belongs to its context as well
                lane._ck(lane.lib.ltm_planes_info(lane.h, wide.h, None, None, None))
            assert e.value.code == -1
        mine.free()
        foreign.free()
        foreign_cloud.free()
    finally:
        lane.close()
    gc.collect()
    assert gpu_ctx.pool_live() == before


def test_counters_count_finite_points_times_valid_hypotheses(gpu_ctx):
    """a fixture built for it: three records -- a plane with non-finite points under an axis that refuses part of the hypotheses, a collinear record (no valid
    hypothesis, so no test), an empty one"""
    names = ["nonfinite_mixed", "collinear", "empty", "size_2049"]
    p = pref.params(0.05, 77, axis=(0.0, 0.0, 1.0), eps_angle=math.radians(14.0), seed=9)
    want_tests = want_valid = want_refined = 0
    for name in names:
        pts = pc.CASES[name][0]
        r = pref.segment(pts, p)
        want_tests += int(np.isfinite(pts[:, :3]).all(axis=1).sum()) * r["n_valid"]
        want_valid += r["n_valid"]
        want_refined += r["refined"]
    assert 0 < want_valid < 2 * 77 and want_refined == 2
    scans, _ = _upload(gpu_ctx, [pc.CASES[n][0] for n in names])
    gpu_ctx.plane_stats(reset=True)
    with _segment(gpu_ctx, scans, p) as pl:
        assert pl.n_valid.sum() == want_valid
    s = gpu_ctx.plane_stats(reset=True)
    print(s)
    assert s == dict(point_hypothesis_tests=want_tests, valid_hypotheses=want_valid, records=4, records_refined=want_refined)
    assert gpu_ctx.plane_stats() == dict.fromkeys(s, 0)
    scans.free()


def test_labels_as_torch(gpu_ctx, shared):
    name = "size_1025"
    if name not in shared:
        shared[name] = _run(gpu_ctx, name)
    _, pl, got = shared[name]
    t = pl.labels(as_torch=True)
    import torch
    assert t.is_cuda and t.dtype == torch.uint8 and (t.cpu().numpy() == got["labels"]).all()


def test_estimate_normals_bytes_did_not_move_with_the_jacobi_routine(gpu_ctx):
    import normals_cases as nc
    pts = nc.sphere()
    cloud = np.ascontiguousarray(np.concatenate([pts, np.zeros((len(pts), 1), np.float32)], axis=1))
    assert hashlib.sha256(cloud.tobytes()).hexdigest() == NORMALS_CLOUD_SHA256      # the fixture itself is the one the hashes were taken on
    for k, want in NORMALS_SHA256.items():
        with gpu_ctx.search_index(cloud) as idx:
            idx.estimate_normals(k, (0.5, -1.0, 20.0))
            assert hashlib.sha256(idx.normals().tobytes()).hexdigest() == want, f"k = {k}"
