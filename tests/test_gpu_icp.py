"""ltm_icp_align on the device against the numpy restatement of include/ltm.h's ICP arithmetic (tools/icp_numpy.py).  The fixtures and the bounds are
those of tests/icp_fixtures.py, which tests/test_icp_api_cpu.py checks on the CPU (the order of the sums decides nothing discrete on them).

tol_T (icp_fixtures.tol_T): device and restatement differ only in summation order and SVD route, about 1e-14 -- unless that moves one transformed
coordinate across a float rounding boundary, which moves one query by one ulp and the estimate by about ulp / N: 2^-23 * 16 / 8 ~ 2.4e-7 on every
entry of T for N >= 64 source points within 16 m; fitness, last_mse and the trace MSEs get the relative 4 * tol_T / extent."""
import numpy as np
import pytest

import icp_fixtures as fx
from tools import icp_numpy as ref

pytestmark = pytest.mark.gpu


def _compare(got, trace, want, n_source, what):
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
    print(f"{what}: iterations {want['iterations']} state {want['state']} max |dT| {dT:.3e} (bound {fx.tol_T(n_source):.3e}) "
          f"max relative mse difference {dm:.3e} (bound {fx.tol_rel(n_source):.3e})")
    assert dT <= fx.tol_T(n_source), (what, dT)
    assert dm <= fx.tol_rel(n_source), (what, dm)
    return dT


def _finite(src):
    return int(np.isfinite(src[:, :3]).all(axis=1).sum())


def test_known_answers(gpu_ctx):
    for off, bound in (((0.0, 0.0, 0.0), 1e-12), (fx.FAR, 1e-9)):
        t, s = fx.lattice_pair(off)
        with gpu_ctx.search_index(t) as idx:
            res, tr = gpu_ctx.icp_align([(idx, s)], trace=True)
        fx.check_known_answer(res[0], bound)
        assert res[0]["converged"] == 1 and (tr[0, :2, 0] == 40).all() and np.isnan(tr[0, 2:]).all()
        assert abs(tr[0, 0, 1] - 0.0625) <= 1e-15 and (res[0]["T"][3] == (0, 0, 0, 1)).all()


def test_scene_fixtures_in_one_batch(gpu_ctx):
    fixtures = [fx.scene_fixture(name) for name in fx.SCENES]
    idx = [gpu_ctx.search_index(t) for t, _, _ in fixtures]
    res, tr = gpu_ctx.icp_align([(i, s) for i, (_, s, _) in zip(idx, fixtures)], trace=True)
    for k, (name, (t, s, want)) in enumerate(zip(fx.SCENES, fixtures)):
        _compare(res[k], tr[k], want, len(s), name)
    for i in idx:
        i.close()


def test_outliers_and_the_correspondence_limit(gpu_ctx):
    t, s, near = fx.outlier_fixture(1.0)
    _, _, far = fx.outlier_fixture(150.0)
    with gpu_ctx.search_index(t) as idx:
        r1, t1 = gpu_ctx.icp_align([(idx, s)], trace=True, max_corr_dist=1.0)
        r2, t2 = gpu_ctx.icp_align([(idx, s)], trace=True, max_corr_dist=150.0)
    assert (t1[0, :near["iterations"], 0] == 600).all() and (t2[0, :far["iterations"], 0] == 640).all()
    _compare(r1[0], t1[0], near, 640, "outliers, limit 1.0")
    _compare(r2[0], t2[0], far, 640, "outliers, limit 150.0")
    assert np.abs(r1[0]["T"] - r2[0]["T"]).max() > 0.1


def test_tree_and_block_edges(gpu_ctx):
    fixtures = fx.edge_fixtures()
    idx = [gpu_ctx.search_index(t) for t, _, _ in fixtures]
    res, tr = gpu_ctx.icp_align([(i, s) for i, (_, s, _) in zip(idx, fixtures)], trace=True)
    for k, (t, s, want) in enumerate(fixtures):
        _compare(res[k], tr[k], want, _finite(s), f"target {len(t)} source {len(s)}")
    for i in idx:
        i.close()


def test_source_block_edges_in_one_batch_are_the_pairs_alone(gpu_ctx):
    """sources on both sides of one and of two 256-point workgroups against one 1025-point target: in one batch (their spans of the block table lie one
    behind the other) each gives, byte for byte, what the same pair gives alone"""
    rng = np.random.default_rng(37)
    target = rng.uniform(-8.0, 8.0, (1025, 3)).astype(np.float32)
    sources = []
    for k, ns in enumerate((256, 257, 512, 513)):
        src = target[rng.choice(1025, ns, replace=False)].astype(np.float64) + rng.normal(0.0, 0.01, (ns, 3))
        sources.append(fx.apply(np.linalg.inv(fx.rigid(2.0 + 0.3 * k, (0.05, -0.04, 0.03), pitch_deg=1.0)), src))
    with gpu_ctx.search_index(target) as idx:
        res, tr = gpu_ctx.icp_align([(idx, s) for s in sources], trace=True)
        for k, s in enumerate(sources):
            alone, ta = gpu_ctx.icp_align([(idx, s)], trace=True)
            assert alone[0].tobytes() == res[k].tobytes() and ta[0].tobytes() == tr[k].tobytes(), len(s)
            assert res[k]["converged"] == 1 and res[k]["iterations"] >= 1 and res[k]["n_corr"] == len(s), len(s)


def _is_rotation(T):
    R = T[:3, :3]
    return np.isfinite(T).all() and np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12 and (T[3] == (0, 0, 0, 1)).all()


def test_degenerate_inputs(gpu_ctx):
    t, s = fx.lattice_pair()
    empty = np.zeros((0, 4), np.float32)
    init = fx.rigid(10.0, (1.0, 2.0, 3.0))
    far = s + np.float32(100.0) * np.float32((0.0, 0.0, 1.0))
    rng = np.random.default_rng(41)
    t1, t2 = rng.uniform(-5, 5, (1, 3)).astype(np.float32), rng.uniform(-5, 5, (2, 3)).astype(np.float32)
    cloud = rng.uniform(-5, 5, (100, 3)).astype(np.float32)
    with gpu_ctx.search_index(t) as it, gpu_ctx.search_index(empty) as ie, gpu_ctx.search_index(t1) as i1, gpu_ctx.search_index(t2) as i2:
        # empty source, empty target: the start transform comes back
        res = gpu_ctx.icp_align([(it, empty), (ie, s)], init=np.stack([init, init]))
        for r in res:
            assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 0)
            assert r["fitness"] == ref.DBL_MAX and r["last_mse"] == ref.DBL_MAX and (r["T"] == init).all()
        res, tr = gpu_ctx.icp_align([(it, s)], trace=True, max_iterations=0)
        assert (res[0]["iterations"], res[0]["converged"], res[0]["fitness"]) == (0, 0, ref.DBL_MAX) and tr.shape == (1, 0, 2)
        # every point beyond the limit: nothing to estimate from, the fitness is still that of the source where it is
        want = ref.align(t, far, max_corr_dist=1.0)
        res, tr = gpu_ctx.icp_align([(it, far)], trace=True, max_corr_dist=1.0)
        assert (want["iterations"], want["converged"], want["state"], want["n_corr"]) == (0, 0, 0, 0)
        _compare(res[0], tr[0], want, len(far), "all beyond the limit")
        assert (res[0]["T"] == np.eye(4)).all() and tr[0, 0, 0] == 0 and np.isnan(tr[0, 0, 1])
        # one and two target points: the rotation is not unique -- finite, orthonormal, det +1, and the same every time
        a = gpu_ctx.icp_align([(i1, cloud), (i2, cloud)])
        b = gpu_ctx.icp_align([(i1, cloud), (i2, cloud)])
        assert a.tobytes() == b.tobytes()
        for r in a:
            assert _is_rotation(r["T"]) and np.isfinite(r["fitness"]) and r["iterations"] >= 1


def test_reproducibility(gpu_ctx):
    """Byte-identical results run to run and whatever else is in the batch.  Started from the restatement's final T the device does what the restatement
    does from there: at most 2 iterations on the fixtures of icp_fixtures.RESTART_QUIET; on scene_3000_700 the restatement itself runs 3 (a stop by the
    transform test is not a fixed point), measured on the device: 3, 1 and 1 iterations."""
    names = list(fx.SCENES)
    (ta, sa, wa), (tb, sb, wb), (tc, sc, wc) = (fx.scene_fixture(n) for n in names)
    assert wb["iterations"] < wa["iterations"] < wc["iterations"]
    ia, ib, ic = gpu_ctx.search_index(ta), gpu_ctx.search_index(tb), gpu_ctx.search_index(tc)
    # the same batch twice
    batch = [(ib, sb), (ia, sa), (ic, sc), (ia, sa)]
    r1, t1 = gpu_ctx.icp_align(batch, trace=True)
    r2, t2 = gpu_ctx.icp_align(batch, trace=True)
    assert r1.tobytes() == r2.tobytes() and t1.tobytes() == t2.tobytes()
    # a pair alone, duplicated inside a batch, and between one that stops earlier and one that stops later
    alone, ta1 = gpu_ctx.icp_align([(ia, sa)], trace=True)
    assert alone[0].tobytes() == r1[1].tobytes() == r1[3].tobytes()
    assert ta1[0].tobytes() == t1[1].tobytes() == t1[3].tobytes()
    assert r1[0]["iterations"] < r1[1]["iterations"] < r1[2]["iterations"]
    # started from the restatement's answer: what the restatement does from there, which is nothing to speak of (at most 2 iterations) on the quiet fixtures
    res = gpu_ctx.icp_align([(ia, sa), (ib, sb), (ic, sc)], init=np.stack([wa["T"], wb["T"], wc["T"]]))
    for name, r, s_ in zip(names, res, (sa, sb, sc)):
        _compare(r, None, fx.restart_fixture(name), len(s_), name + " restarted")
        if name in fx.RESTART_QUIET:
            assert r["iterations"] <= 2 and r["converged"] == 1, (name, r["iterations"])
    for i in (ia, ib, ic):
        i.close()


def test_launch_counts_do_not_grow_with_the_batch(gpu_ctx):
    names = list(fx.SCENES)
    fixtures = [fx.scene_fixture(n) for n in names]
    slow = max(fixtures, key=lambda f: f[2]["iterations"])
    idx = [gpu_ctx.search_index(t) for t, _, _ in fixtures]
    pairs8 = [(idx[k % 3], fixtures[k % 3][1]) for k in range(8)]
    k_slow = [f is slow for f in fixtures].index(True)
    counts = {}
    gpu_ctx.profile_enable(True)
    try:
        for what, pairs in (("one", [(idx[k_slow], slow[1])]), ("eight", pairs8)):
            gpu_ctx.profile_reset()
            gpu_ctx.icp_align(pairs)
            prof = gpu_ctx.profile_read()
            counts[what] = prof["icp_iter"]["launches"]
            assert prof["icp_fitness"]["launches"] == 2
    finally:
        gpu_ctx.profile_enable(False)
        for i in idx:
            i.close()
    # two launches per iteration of the slowest pair, plus what is enqueued before the host looks at the counter again (a constant)
    assert counts["eight"] <= 2 * slow[2]["iterations"] + 16, counts
    assert counts["eight"] <= counts["one"], counts


def test_foreign_handles_and_pool_bookkeeping(gpu_ctx, ltm):
    import ctypes as C
    t, s = fx.lattice_pair()
    other = ltm.Context(vfov=50.0, hfov=360.0, device=0)
    theirs = other.search_index(t)
    mine = gpu_ctx.search_index(t)
    src = gpu_ctx.upload(np.concatenate([s, np.zeros((len(s), 1), np.float32)], axis=1))
    live0 = gpu_ctx.pool_live()
    res = gpu_ctx.icp_align([(mine, src), (mine, src)], trace=True)[0]
    assert gpu_ctx.pool_live() == live0, "ltm_icp_align must give every block back to the pool"
    assert res[0].tobytes() == res[1].tobytes()
    # an index of another context is refused (before anything is allocated), and so is a cloud handle that was never issued
    with pytest.raises(ltm.LtmError) as e:
        gpu_ctx.icp_align([(mine, src), (theirs, src)])
    assert e.value.code == -1
    out = np.zeros(1, ltm.ICP_RESULT)
    th = (C.c_void_p * 1)(mine.h)
    sh = (C.c_uint64 * 1)(0xdeadbeef)
    assert gpu_ctx.lib.ltm_icp_align(gpu_ctx.h, 1, th, sh, None, None, out.ctypes.data, None) == -1
    with pytest.raises(ltm.LtmError):
        gpu_ctx.icp_align([(mine, src)], max_corr_dist=float("nan"))
    assert gpu_ctx.pool_live() == live0
    mine.close()
    theirs.close()
    other.close()
