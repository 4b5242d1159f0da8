"""ltm_icp_align_plane on the device against the numpy restatement of include/ltm.h's "icp, point-to-plane" (tools/icp_plane_numpy.py).  The device runs
with the normals it estimated itself (k = 10), the restatement with the restatement's float normals (tools/normals_numpy.py).  The fixtures are those of
tests/normals_cases.py -- the clouds of tests/icp_fixtures.py -- which tests/test_icp_plane_api_cpu.py checks on the CPU (the order of the sums decides
nothing discrete on them).

Bounds, as tests/icp_fixtures.py derives them for the point-to-point routine: device and restatement differ in summation order and in the route of the
solve (Cholesky against LU), about 1e-14 -- unless that moves one transformed coordinate across a float rounding boundary, which moves one query by one
ulp (2^-23 * 16 m) and the estimate by about ulp / N: tol_T = 2^-23 * 16 / 8 ~ 2.4e-7 on every entry of T for N >= 64 source points within 16 m (scaled by
64 / N below that); fitness, last_mse and the trace MSEs get the relative tol_rel = 4 tol_T / 16.  The normals add nothing to this: a component may differ
by one float ulp (6e-8 relative, tests/test_gpu_normals.py), which changes a row's right side n . (q - p), at most a few centimetres here, by 1e-9 and
the estimate by 1e-9 / N."""
import ctypes as C

import numpy as np
import pytest

import icp_fixtures as fx
import normals_cases as nc
from tools import icp_plane_numpy as plane_ref

pytestmark = pytest.mark.gpu


def _compare(got, trace, want, n_source, what, scale=1.0):
    """one device record (and its trace rows) against the restatement's result"""
    assert (int(got["iterations"]), int(got["state"]), int(got["converged"]), int(got["n_corr"])) == \
        (want["iterations"], want["state"], want["converged"], want["n_corr"]), what
    dT = np.abs(got["T"] - want["T"]).max()
    rel = lambda a, b: 0.0 if a == b else abs(a - b) / abs(b)      # noqa: E731
    dm = max(rel(float(got["fitness"]), want["fitness"]), rel(float(got["last_mse"]), want["last_mse"]))
    if trace is not None:
        wt = want["trace"]
        assert trace.shape == wt.shape, what
        assert (np.isnan(trace) == np.isnan(wt)).all(), what
        ran = ~np.isnan(wt[:, 0])
        assert (trace[ran, 0] == wt[ran, 0]).all(), (what, "n_corr per iteration")
        ok = ~np.isnan(wt[:, 1])
        if ok.any():
            dm = max(dm, (np.abs(trace[ok, 1] - wt[ok, 1]) / wt[ok, 1]).max())
    print(f"{what}: iterations {want['iterations']} state {want['state']} max |dT| {dT:.3e} (bound {scale * fx.tol_T(n_source):.3e}) "
          f"max relative mse difference {dm:.3e} (bound {scale * fx.tol_rel(n_source):.3e})")
    assert dT <= scale * fx.tol_T(n_source), (what, dT)
    assert dm <= scale * fx.tol_rel(n_source), (what, dm)


def _finite(src):
    return int(np.isfinite(src[:, :3]).all(axis=1).sum())


def _indices(gpu_ctx, targets, viewpoint=(0.0, 0.0, 0.0)):
    """search indices with device-estimated normals, all in one call"""
    idx = [gpu_ctx.search_index(t) for t in targets]
    gpu_ctx.estimate_normals(idx, nc.ICP_NORMAL_K, np.tile(np.float32(viewpoint), (len(idx), 1)))
    return idx


def _close(idx):
    for i in idx:
        i.close()


def test_scene_fixtures_in_one_batch(gpu_ctx):
    fixtures = [nc.plane_fixture("scene", name) for name in fx.SCENES]
    idx = _indices(gpu_ctx, [f[0] for f in fixtures])
    res, tr = gpu_ctx.icp_align([(i, f[1]) for i, f in zip(idx, fixtures)], trace=True, method="plane")
    for k, (name, (t, s, n, want)) in enumerate(zip(fx.SCENES, fixtures)):
        _compare(res[k], tr[k], want, len(s), name)
        assert want["iterations"] < fx.scene_fixture(name)[2]["iterations"]
    _close(idx)


def test_outliers_and_the_correspondence_limit(gpu_ctx):
    t, s, _, near = nc.plane_fixture("outlier", None, 1.0)
    far = nc.plane_fixture("outlier", None, 150.0)[3]
    idx = _indices(gpu_ctx, [t])
    r1, t1 = gpu_ctx.icp_align([(idx[0], s)], trace=True, method="plane", max_corr_dist=1.0)
    r2, t2 = gpu_ctx.icp_align([(idx[0], s)], trace=True, method="plane", max_corr_dist=150.0)
    _close(idx)
    assert (t1[0, :near["iterations"], 0] == 600).all() and (t2[0, :far["iterations"], 0] == 640).all()
    _compare(r1[0], t1[0], near, 640, "outliers, limit 1.0")
    _compare(r2[0], t2[0], far, 640, "outliers, limit 150.0")


def test_tree_and_block_edges(gpu_ctx):
    fixtures = [nc.plane_fixture("edge", k) for k in range(nc.N_EDGE)]
    idx = _indices(gpu_ctx, [f[0] for f in fixtures])
    res, tr = gpu_ctx.icp_align([(i, f[1]) for i, f in zip(idx, fixtures)], trace=True, method="plane")
    for k, (t, s, n, want) in enumerate(fixtures):
        _compare(res[k], tr[k], want, _finite(s), f"target {len(t)} source {len(s)}")
    assert res[0]["state"] == 5 and res[0]["converged"] == 0 and (res[0]["T"] == np.eye(4)).all(), "three correspondences do not determine six unknowns"
    _close(idx)


def test_far_from_the_origin(gpu_ctx):
    t, s, n, want = nc.plane_fixture("far", nc.FAR_SCENE)
    idx = _indices(gpu_ctx, [t], fx.FAR)
    res, tr = gpu_ctx.icp_align([(idx[0], s)], trace=True, method="plane")
    _close(idx)
    _compare(res[0], tr[0], want, len(s), "2 km from the origin", scale=nc.FAR_SCALE)


def test_degenerate_systems_and_inputs(gpu_ctx, ltm):
    empty = np.zeros((0, 4), np.float32)
    init = fx.rigid(2.0, (0.1, 0.0, 0.0))
    pt, ps = nc.plane_z0()
    lt, ls = fx.lattice_pair()
    rng = np.random.default_rng(81)
    cloud = rng.uniform(-5, 5, (100, 3)).astype(np.float32)
    two = rng.uniform(-5, 5, (2, 3)).astype(np.float32)
    bare = gpu_ctx.search_index(lt)
    ip, il, i2, ie = _indices(gpu_ctx, [pt, lt, two, empty])
    # a target without normals is refused
    with pytest.raises(ltm.LtmError) as e:
        gpu_ctx.icp_align([(il, ls), (bare, ls)], method="plane")
    assert e.value.code == -1
    # a single exact plane: state 5, not converged, T = init, the iteration's correspondences on record
    res, tr = gpu_ctx.icp_align([(ip, ps)], init=init[None], trace=True, method="plane")
    r = res[0]
    assert (r["state"], r["converged"], r["iterations"], r["n_corr"]) == (5, 0, 0, len(ps)) and (r["T"] == init).all()
    assert tr[0, 0, 0] == len(ps) and np.isfinite(tr[0, 0, 1]) and np.isnan(tr[0, 1:]).all()
    want = plane_ref.align(pt, nc.nref.estimate(pt, nc.ICP_NORMAL_K)["normals"], ps, init=init)
    _compare(r, tr[0], want, len(ps), "a single exact plane")
    # fewer than three correspondences: two source points; a target whose normals are NaN (two points) loses every correspondence
    res = gpu_ctx.icp_align([(il, ls[:2]), (i2, cloud)], method="plane")
    assert [(r["state"], r["converged"], r["iterations"], r["n_corr"]) for r in res] == [(0, 0, 0, 2), (0, 0, 0, 0)]
    assert (res[0]["T"] == np.eye(4)).all() and np.isfinite(res[1]["fitness"]) and res[1]["last_mse"] == plane_ref.DBL_MAX
    # empty source, empty target, no iteration allowed: the start transform comes back
    res = gpu_ctx.icp_align([(il, empty), (ie, ls)], init=np.stack([init, init]), method="plane")
    for r in res:
        assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 0)
        assert r["fitness"] == plane_ref.DBL_MAX and r["last_mse"] == plane_ref.DBL_MAX and (r["T"] == init).all()
    res, tr = gpu_ctx.icp_align([(il, ls)], trace=True, max_iterations=0, method="plane")
    assert (res[0]["iterations"], res[0]["converged"], res[0]["fitness"]) == (0, 0, plane_ref.DBL_MAX) and tr.shape == (1, 0, 2)
    # the lattice's known answer holds for this method too
    res = gpu_ctx.icp_align([(il, ls)], method="plane")
    fx.check_known_answer(res[0], 1e-9)
    _close([bare, ip, il, i2, ie])


def test_reproducibility_and_the_scan_set_form(gpu_ctx):
    """byte-identical results run to run, alone, duplicated and among other pairs; sources read in place from a scan set give the cloud form's bytes"""
    names = list(fx.SCENES)
    (ta, sa, _, wa), (tb, sb, _, wb), (tc, sc, _, wc) = (nc.plane_fixture("scene", n) for n in names)
    ot, os_, _, ow = nc.plane_fixture("outlier", None, 150.0)      # runs to the iteration limit: the other pairs stop long before it
    ia, ib, ic, io = _indices(gpu_ctx, [ta, tb, tc, ot])
    batch = [(ib, sb), (ia, sa), (io, os_), (ic, sc), (ia, sa)]
    r1, t1 = gpu_ctx.icp_align(batch, trace=True, method="plane")
    r2, t2 = gpu_ctx.icp_align(batch, trace=True, method="plane")
    assert r1.tobytes() == r2.tobytes() and t1.tobytes() == t2.tobytes()
    alone, ta1 = gpu_ctx.icp_align([(ia, sa)], trace=True, method="plane")
    assert alone[0].tobytes() == r1[1].tobytes() == r1[4].tobytes()
    assert ta1[0].tobytes() == t1[1].tobytes() == t1[4].tobytes()
    assert r1[2]["iterations"] > r1[1]["iterations"]
    # the scan-set form
    xyzi = lambda a: np.concatenate([a, np.zeros((len(a), 1), np.float32)], axis=1)      # noqa: E731
    srcs = [sb, sa, os_, sc]
    off = np.concatenate([[0], np.cumsum([len(a) for a in srcs])]).astype(np.uint64)
    ss = gpu_ctx.upload_scans(np.concatenate([xyzi(a) for a in srcs]), off)
    r3, t3 = gpu_ctx.icp_align([(ib, (ss, 0)), (ia, (ss, 1)), (io, (ss, 2)), (ic, (ss, 3)), (ia, (ss, 1))], trace=True, method="plane")
    assert r3.tobytes() == r1.tobytes() and t3.tobytes() == t1.tobytes()
    ss.free()
    _close([ia, ib, ic, io])


def test_launch_counts_do_not_grow_with_the_batch(gpu_ctx):
    fixtures = [nc.plane_fixture("scene", n) for n in fx.SCENES]
    slow = max(fixtures, key=lambda f: f[3]["iterations"])
    idx = _indices(gpu_ctx, [f[0] for f in fixtures])
    pairs8 = [(idx[k % 3], fixtures[k % 3][1]) for k in range(8)]
    k_slow = [f is slow for f in fixtures].index(True)
    counts = {}
    gpu_ctx.profile_enable(True)
    try:
        for what, pairs in (("one", [(idx[k_slow], slow[1])]), ("eight", pairs8)):
            gpu_ctx.profile_reset()
            gpu_ctx.icp_align(pairs, method="plane")
            prof = gpu_ctx.profile_read()
            counts[what] = prof["icp_iter"]["launches"]
            assert prof["icp_fitness"]["launches"] == 2
    finally:
        gpu_ctx.profile_enable(False)
        _close(idx)
    # two launches per iteration of the slowest pair, plus what is enqueued before the host looks at the counter again (a constant)
    assert counts["eight"] <= 2 * slow[3]["iterations"] + 16, counts
    assert counts["eight"] <= counts["one"], counts


def test_foreign_handles_and_pool_bookkeeping(gpu_ctx, ltm):
    t, s = fx.lattice_pair()
    other = ltm.Context(vfov=50.0, hfov=360.0, device=0)
    theirs = other.search_index(t)
    theirs.estimate_normals(nc.ICP_NORMAL_K)
    mine = _indices(gpu_ctx, [t])[0]
    src = gpu_ctx.upload(np.concatenate([s, np.zeros((len(s), 1), np.float32)], axis=1))
    live0 = gpu_ctx.pool_live()
    res = gpu_ctx.icp_align([(mine, src), (mine, src)], trace=True, method="plane")[0]
    assert gpu_ctx.pool_live() == live0, "ltm_icp_align_plane must give every block back to the pool"
    assert res[0].tobytes() == res[1].tobytes()
    with pytest.raises(ltm.LtmError) as e:
        gpu_ctx.icp_align([(mine, src), (theirs, src)], method="plane")
    assert e.value.code == -1
    out = np.zeros(1, ltm.ICP_RESULT)
    th = (C.c_void_p * 1)(mine.h)
    sh = (C.c_uint64 * 1)(0xdeadbeef)
    assert gpu_ctx.lib.ltm_icp_align_plane(gpu_ctx.h, 1, th, sh, None, None, out.ctypes.data, None) == -1
    with pytest.raises(ltm.LtmError):
        gpu_ctx.icp_align([(mine, src)], method="plane", max_corr_dist=float("nan"))
    bare = gpu_ctx.search_index(t)
    live1 = gpu_ctx.pool_live()
    with pytest.raises(ltm.LtmError):
        gpu_ctx.icp_align([(mine, src), (bare, src)], method="plane")      # no normals on the second target
    assert gpu_ctx.pool_live() == live1
    bare.close()
    assert gpu_ctx.pool_live() == live0
    # the point-to-point entry points do not care about normals
    a = gpu_ctx.icp_align([(mine, src)])
    fx.check_known_answer(a[0], 1e-12)
    mine.close()
    theirs.close()
    other.close()
