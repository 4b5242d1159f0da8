"""ltm_icp_align_gicp on the device against the numpy restatement of include/ltm.h's "icp, generalized" (tools/icp_gicp_numpy.py).  The device runs with
the normals it estimated itself on BOTH sides, the restatement with the restatement's float normals (tools/normals_numpy.py).  The fixtures are those of
tests/gicp_cases.py, which tests/test_icp_gicp_api_cpu.py checks on the CPU: every normal that enters a correspondence is well-posed, and neither the
order of the sums nor one float ulp on every normal component decides anything discrete on them.

Bounds: those of tests/gicp_cases.py -- fx.tol_T / fx.tol_rel times gc.T_FACTOR, whose derivation (one ulp on a normal moves a correspondence's weight
across the surfaces by 2^-21 / (2 epsilon) = 2.4e-4, M's largest eigenvalue being 1 / (2 epsilon)) stands there."""
import ctypes as C

import numpy as np
import pytest

import gicp_cases as gc
import icp_fixtures as fx
import normals_cases as nc
from tools import icp_gicp_numpy as gicp_ref
from tools import normals_numpy as nref

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
    print(f"{what}: iterations {want['iterations']} state {want['state']} max |dT| {dT:.3e} (bound {gc.tol_T(n_source, scale):.3e}) "
          f"max relative mse difference {dm:.3e} (bound {gc.tol_rel(n_source, scale):.3e})")
    assert dT <= gc.tol_T(n_source, scale), (what, dT)
    assert dm <= gc.tol_rel(n_source, scale), (what, dm)


def _indices(gpu_ctx, clouds, k=nc.ICP_NORMAL_K, viewpoint=(0.0, 0.0, 0.0)):
    """search indices with device-estimated normals, all in one call; k: one value or one per cloud (one call per distinct value)"""
    idx = [gpu_ctx.search_index(c) for c in clouds]
    ks = [k] * len(idx) if np.isscalar(k) else list(k)
    for kk in sorted(set(ks)):
        sel = [i for i, x in zip(idx, ks) if x == kk]
        gpu_ctx.estimate_normals(sel, kk, np.tile(np.float32(viewpoint), (len(sel), 1)))
    return idx


def _close(idx):
    for i in idx:
        i.close()


def test_scene_fixtures_in_one_batch(gpu_ctx):
    fixtures = [gc.gicp_fixture("scene", name) for name in gc.SCENES]
    ks = [gc.normal_k("scene", name) for name in gc.SCENES]
    ti = _indices(gpu_ctx, [f[0] for f in fixtures], ks)
    si = _indices(gpu_ctx, [f[1] for f in fixtures], ks)
    res, tr = gpu_ctx.icp_align(list(zip(ti, si)), trace=True, method="gicp")
    for k, (name, f) in enumerate(zip(gc.SCENES, fixtures)):
        _compare(res[k], tr[k], f[4], len(f[1]), name)
        assert res[k]["converged"] == 1
    _close(ti + si)


def test_outliers_and_the_correspondence_limit(gpu_ctx):
    t, s, _, _, near = gc.gicp_fixture("outlier", None, 1.0)
    far = gc.gicp_fixture("outlier", None, 150.0)[4]
    it, is_ = _indices(gpu_ctx, [t, s])
    r1, t1 = gpu_ctx.icp_align([(it, is_)], trace=True, method="gicp", max_corr_dist=1.0)
    r2, t2 = gpu_ctx.icp_align([(it, is_)], trace=True, method="gicp", max_corr_dist=150.0)
    _close([it, is_])
    assert (t1[0, :near["iterations"], 0] == 600).all() and (t2[0, :far["iterations"], 0] == 640).all()
    _compare(r1[0], t1[0], near, 640, "outliers, limit 1.0")
    _compare(r2[0], t2[0], far, 640, "outliers, limit 150.0")


def test_tree_and_block_edges(gpu_ctx):
    fixtures = [gc.gicp_fixture("edge", k) for k in range(gc.N_EDGE)]
    ti = _indices(gpu_ctx, [f[0] for f in fixtures])
    si = _indices(gpu_ctx, [f[1] for f in fixtures])
    res, tr = gpu_ctx.icp_align(list(zip(ti, si)), trace=True, method="gicp")
    for k, f in enumerate(fixtures):
        _compare(res[k], tr[k], f[4], gc.finite_count(f[1]), f"target {len(f[0])} source {len(f[1])}")
    assert res[0]["n_corr"] == 3 and res[0]["converged"] == 1, "three correspondences are enough for a positive definite weight"
    _close(ti + si)


def test_far_from_the_origin(gpu_ctx):
    t, s, _, _, want = gc.gicp_fixture("far", gc.FAR_SCENE)
    it, is_ = _indices(gpu_ctx, [t, s], viewpoint=fx.FAR)
    res, tr = gpu_ctx.icp_align([(it, is_)], trace=True, method="gicp")
    _close([it, is_])
    _compare(res[0], tr[0], want, len(s), "2 km from the origin", scale=gc.FAR_SCALE)


def test_degenerate_inputs(gpu_ctx, ltm):
    empty = np.zeros((0, 4), np.float32)
    init = fx.rigid(2.0, (0.1, 0.0, 0.0))
    pt, ps = nc.plane_z0()
    lt, ls = fx.lattice_pair()
    rng = np.random.default_rng(81)
    cloud = rng.uniform(-5, 5, (100, 3)).astype(np.float32)
    two = rng.uniform(-5, 5, (2, 3)).astype(np.float32)
    bare_t, bare_s = gpu_ctx.search_index(lt), gpu_ctx.search_index(ls)
    ip, isp, il, ils, i2, ic, ie = _indices(gpu_ctx, [pt, ps, lt, ls, two, cloud, empty])
    # a target or a source without normals is refused, and nothing stays allocated
    live = gpu_ctx.pool_live()
    for pairs in ([(il, ils), (bare_t, ils)], [(il, ils), (il, bare_s)]):
        with pytest.raises(ltm.LtmError) as e:
            gpu_ctx.icp_align(pairs, method="gicp")
        assert e.value.code == -1 and gpu_ctx.pool_live() == live
    # fewer than three correspondences: a two-point source (its normals are NaN: nothing is kept); a target whose normals are all NaN
    res = gpu_ctx.icp_align([(il, i2), (i2, ic)], method="gicp")
    assert [(r["state"], r["converged"], r["iterations"], r["n_corr"]) for r in res] == [(0, 0, 0, 0), (0, 0, 0, 0)]
    assert (res[0]["T"] == np.eye(4)).all() and np.isfinite(res[1]["fitness"]) and res[1]["last_mse"] == gicp_ref.DBL_MAX
    # empty source index, empty target, no iteration allowed: the start transform comes back
    res = gpu_ctx.icp_align([(il, ie), (ie, ils)], init=np.stack([init, init]), method="gicp")
    for r in res:
        assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 0)
        assert r["fitness"] == gicp_ref.DBL_MAX and r["last_mse"] == gicp_ref.DBL_MAX and (r["T"] == init).all()
    res, tr = gpu_ctx.icp_align([(il, ils)], init=init[None], trace=True, max_iterations=0, method="gicp")
    r = res[0]
    assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 0) and tr.shape == (1, 0, 2)
    assert r["fitness"] == gicp_ref.DBL_MAX and r["last_mse"] == gicp_ref.DBL_MAX and (r["T"] == init).all()
    # a single exact plane with its source index: the plane alone leaves three unknowns free, and GICP goes on -- what the restatement gives
    want = gicp_ref.align(pt, nref.estimate(pt, nc.ICP_NORMAL_K)["normals"], ps, nref.estimate(ps, nc.ICP_NORMAL_K)["normals"], init=init)
    assert want["state"] != 5
    res, tr = gpu_ctx.icp_align([(ip, isp)], init=init[None], trace=True, method="gicp")
    _compare(res[0], tr[0], want, len(ps), "a single exact plane")
    _close([bare_t, bare_s, ip, isp, il, ils, i2, ic, ie])


def test_reproducibility_and_shared_indices(gpu_ctx):
    """byte-identical results run to run, alone, duplicated and among other pairs, one of which runs to the iteration limit; one index as the target of
    one pair and the source of another in the same batch"""
    names = list(fx.SCENES)
    fa, fb, fc = (gc.gicp_fixture("scene", n) for n in names)
    ti = _indices(gpu_ctx, [fa[0], fb[0], fc[0]])
    si = _indices(gpu_ctx, [fa[1], fb[1], fc[1]])
    ia, ib, ic = ti
    sa, sb, sc = si
    # no fixture keeps this method busy for long (the outlier pair stops after 3 iterations, a start 25 degrees and 3 m off after 5): the pair that runs to
    # the iteration limit is the one started far off, under a limit of 4, which the first pair (3 iterations) does not reach
    off = fx.rigid(25.0, (2.0, -2.0, 0.5))
    eye = np.eye(4)
    batch = [(ib, sb), (ia, sa), (ic, sc), (ic, sc), (ia, sa)]
    init = np.stack([eye, eye, off, eye, eye])
    r1, t1 = gpu_ctx.icp_align(batch, init=init, trace=True, method="gicp", max_iterations=4)
    r2, t2 = gpu_ctx.icp_align(batch, init=init, trace=True, method="gicp", max_iterations=4)
    assert r1.tobytes() == r2.tobytes() and t1.tobytes() == t2.tobytes()
    alone, ta1 = gpu_ctx.icp_align([(ia, sa)], trace=True, method="gicp", max_iterations=4)
    assert alone[0].tobytes() == r1[1].tobytes() == r1[4].tobytes()
    assert ta1[0].tobytes() == t1[1].tobytes() == t1[4].tobytes()
    assert r1[2]["state"] == 1 and r1[2]["iterations"] == 4 > r1[1]["iterations"], "the pair started far off runs to the iteration limit"
    # one index on both sides of one batch: the dense target as a target, and as the source of another pair
    x1 = gpu_ctx.icp_align([(ia, sa), (ib, ia)], method="gicp", max_iterations=4)
    x2 = gpu_ctx.icp_align([(ib, ia)], method="gicp", max_iterations=4)
    assert x1[0].tobytes() == alone[0].tobytes() and x1[1].tobytes() == x2[0].tobytes()
    _close(ti + si)


def test_launch_counts_do_not_grow_with_the_batch(gpu_ctx):
    fixtures = [gc.gicp_fixture("scene", n) for n in fx.SCENES]
    slow = max(fixtures, key=lambda f: f[4]["iterations"])
    k_slow = [f is slow for f in fixtures].index(True)
    ti = _indices(gpu_ctx, [f[0] for f in fixtures])
    si = _indices(gpu_ctx, [f[1] for f in fixtures])
    pairs8 = [(ti[k % 3], si[k % 3]) for k in range(8)]
    counts = {}
    gpu_ctx.profile_enable(True)
    try:
        for what, pairs in (("one", [(ti[k_slow], si[k_slow])]), ("eight", pairs8)):
            gpu_ctx.profile_reset()
            gpu_ctx.icp_align(pairs, method="gicp")
            prof = gpu_ctx.profile_read()
            counts[what] = prof["icp_iter"]["launches"]
            assert prof["icp_fitness"]["launches"] == 2
            assert "icp_prepare" not in prof or prof["icp_prepare"]["launches"] == 0, "the sources are read in place: nothing to prepare"
    finally:
        gpu_ctx.profile_enable(False)
        _close(ti + si)
    assert counts["eight"] <= 2 * slow[4]["iterations"] + 16, counts
    assert counts["eight"] <= counts["one"], counts


def test_foreign_handles_and_pool_bookkeeping(gpu_ctx, ltm):
    t, s = fx.lattice_pair()
    other = ltm.Context(vfov=50.0, hfov=360.0, device=0)
    theirs = other.search_index(t)
    theirs.estimate_normals(nc.ICP_NORMAL_K)
    mine, src = _indices(gpu_ctx, [t, s])
    live0 = gpu_ctx.pool_live()
    res = gpu_ctx.icp_align([(mine, src), (mine, src)], trace=True, method="gicp")[0]
    assert gpu_ctx.pool_live() == live0, "ltm_icp_align_gicp must give every block back to the pool"
    assert res[0].tobytes() == res[1].tobytes()
    for pairs in ([(mine, src), (theirs, src)], [(mine, src), (mine, theirs)]):
        with pytest.raises(ltm.LtmError) as e:
            gpu_ctx.icp_align(pairs, method="gicp")
        assert e.value.code == -1 and gpu_ctx.pool_live() == live0
    out = np.zeros(1, ltm.ICP_RESULT)
    th = (C.c_void_p * 1)(mine.h)
    sh = (C.c_void_p * 1)(0xdeadbeef)
    assert gpu_ctx.lib.ltm_icp_align_gicp(gpu_ctx.h, 1, th, sh, None, None, 1e-3, out.ctypes.data, None) == -1
    assert gpu_ctx.lib.ltm_icp_align_gicp(gpu_ctx.h, 1, sh, th, None, None, 1e-3, out.ctypes.data, None) == -1
    sh[0] = src.h
    for eps in (0.0, -1.0, 1.5, float("nan")):
        assert gpu_ctx.lib.ltm_icp_align_gicp(gpu_ctx.h, 1, th, sh, None, None, eps, out.ctypes.data, None) == -1
    with pytest.raises(ltm.LtmError):
        gpu_ctx.icp_align([(mine, src)], method="gicp", max_corr_dist=float("nan"))
    assert gpu_ctx.pool_live() == live0
    # epsilon = 1 is allowed: every weight is I / 2 and the method is point-to-point's linearised step
    one = gpu_ctx.icp_align([(mine, src)], method="gicp", gicp_epsilon=1.0)
    assert one[0]["converged"] == 1 and abs(one[0]["T"][0, 3] - 0.25) < 1e-6
    # the other methods on the same indices are what they were
    cloud = gpu_ctx.upload(np.concatenate([s, np.zeros((len(s), 1), np.float32)], axis=1))
    fx.check_known_answer(gpu_ctx.icp_align([(mine, cloud)])[0], 1e-12)
    fx.check_known_answer(gpu_ctx.icp_align([(mine, cloud)], method="plane")[0], 1e-9)
    cloud.free()
    assert gpu_ctx.pool_live() == live0
    _close([mine, src])
    theirs.close()
    other.close()


def _affines_of(ltm, poses16):
    """the 6-D poses of a synthetic session (planar: x, y, z, yaw) as float affines"""
    P = poses16.reshape(-1, 4, 4)
    p6 = np.stack([P[:, 0, 3], P[:, 1, 3], P[:, 2, 3], np.zeros(len(P)), np.zeros(len(P)), np.arctan2(P[:, 1, 0], P[:, 0, 0])], axis=1)
    return ltm.pose6d_to_affine3f(p6.astype(np.float32))


def test_verify_loops_is_the_hand_driven_chain(gpu_ctx, ltm):
    from tools import synth
    A = synth.to_numpy(synth.make_session(1, 12, "small"))
    B = synth.to_numpy(synth.make_session(2, 12, "small"))
    ta, sa = _affines_of(ltm, A["poses"]), _affines_of(ltm, B["poses"])
    tscans, sscans = gpu_ctx.upload_scans(A["scans"], A["offsets"]), gpu_ctx.upload_scans(B["scans"], B["offsets"])
    pairs = [(k, k) for k in range(0, 12, 2)] + [(4, 7)]      # target key 4 twice: its submap and index are made once
    icp = dict(max_iterations=20)
    live = gpu_ctx.pool_live()
    res, accept = gpu_ctx.verify_loops(tscans, sscans, pairs, ta, sa, search_num=2, leaf=0.3, method="gicp", normal_k=20, **icp)
    assert gpu_ctx.pool_live() == live
    # by hand: loop_submaps -> search_index_batch x 2 -> estimate_normals -> icp_align
    tkeys = sorted({t for t, _ in pairs})
    tsub = gpu_ctx.loop_submaps(tscans, tkeys, 2, 0.3, ta)
    ssub = gpu_ctx.loop_submaps(sscans, [s for _, s in pairs], 0, 0.3, sa)
    ti, si = gpu_ctx.search_index_batch(tsub), gpu_ctx.search_index_batch(ssub)
    vp = np.concatenate([np.asarray(ta).reshape(-1, 3, 4)[tkeys, :, 3], np.asarray(sa).reshape(-1, 3, 4)[[s for _, s in pairs], :, 3]])
    gpu_ctx.estimate_normals(ti + si, 20, vp)
    want = gpu_ctx.icp_align([(ti[tkeys.index(t)], si[j]) for j, (t, _) in enumerate(pairs)], method="gicp", **icp)
    _close(ti + si)
    tsub.free()
    ssub.free()
    assert res.tobytes() == want.tobytes()
    assert (accept == ((want["converged"] != 0) & (want["fitness"] <= 0.5))).all()
    assert (res["iterations"] > 0).all() and (res["n_corr"] > 100).all()
    # batches cut by the point budget give what one batch gives; no normal_k: the method's own 20
    res2, accept2 = gpu_ctx.verify_loops(tscans, sscans, pairs, ta, sa, search_num=2, leaf=0.3, max_batch_points=1, method="gicp", **icp)
    assert res2.tobytes() == res.tobytes() and (accept2 == accept).all()
    assert gpu_ctx.pool_live() == live
    tscans.free()
    sscans.free()
