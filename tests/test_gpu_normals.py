"""ltm_search_estimate_normals on the device against the numpy restatement of include/ltm.h's "normals" (tools/normals_numpy.py).  The fixtures are those
of tests/normals_cases.py, which tests/test_normals_cases_cpu.py checks on the CPU.

Bounds.  Device and restatement form the same covariance in double from the same neighbours in the same order and differ in the eigen-solver (cyclic Jacobi
against LAPACK): the directions agree to about 1e-16 / gap, 1e-12 at the gaps the fixtures keep (>= 1e-3), the eigenvalues to about 1e-16 relative.  What
is compared is the float the double is rounded to, and a difference of 1e-12 can move a double across one rounding boundary: a component, of magnitude at
most 1, may differ by one float ulp, 2^-23 at the most; the curvature by 1e-12 + 2^-23 curvature.  The sign after the viewpoint flip is compared wherever
the flip's dot product is not within 1e-6 of zero."""
import ctypes as C

import numpy as np
import pytest

import normals_cases as nc
from tools import normals_numpy as nref

pytestmark = pytest.mark.gpu

_compare = nc.compare      # the comparison rule, shared with tests/test_gpu_walker_edges.py


@pytest.mark.parametrize("name", nc.NORMALS_FIXTURES)
def test_against_the_restatement(gpu_ctx, name):
    cloud, k, vp, r = nc.normals_fixture(name)
    with gpu_ctx.search_index(cloud) as idx:
        assert idx.normals_k() == 0
        idx.estimate_normals(k, vp)
        assert idx.normals_k() == k
        _compare(idx.normals(), r, name)


def test_small_targets_and_k_beyond_the_target(gpu_ctx):
    """1 ... 257 points (leaves of 32, targets that are one leaf, block edges of 64 and 256), at k on both sides of the register / LDS split and beyond
    the target's size"""
    rng = np.random.default_rng(71)
    sizes = (1, 2, 3, 31, 32, 33, 64, 65, 256, 257)
    clouds = [rng.uniform(-8.0, 8.0, (n, 3)).astype(np.float32) for n in sizes]
    for k in (5, 16, 40, 64):
        idx = [gpu_ctx.search_index(c) for c in clouds]
        gpu_ctx.estimate_normals(idx, k)
        for n, c, i in zip(sizes, clouds, idx):
            got = i.normals()
            if n < 3:
                assert got.shape == (n, 4) and np.isnan(got).all(), (n, k)
            else:
                _compare(got, nref.estimate(c, k), f"{n} points, k = {k}")
            i.close()


def test_degenerate_neighbourhoods(gpu_ctx):
    # duplicated points: zero covariance gives curvature 0 and a finite unit normal
    dup = np.tile(np.float32([[1.5, -2.0, 0.25]]), (40, 1))
    # collinear points: finite, unit, and the same on a second run
    line = (np.arange(100, dtype=np.float32)[:, None] * np.float32([[0.1, 0.2, -0.05]])).astype(np.float32)
    for k in (10, 20):
        with gpu_ctx.search_index(dup) as a, gpu_ctx.search_index(line) as b:
            gpu_ctx.estimate_normals([a, b], k)
            na, nb = a.normals(), b.normals()
            assert (na[:, 3] == 0).all()
            for n in (na, nb):
                assert np.isfinite(n).all() and np.abs(np.linalg.norm(n[:, :3].astype(np.float64), axis=1) - 1.0).max() < 1e-6
            assert (nb[:, 3] >= 0).all() and (nb[:, 3] < 1e-6).all()
            b.estimate_normals(k)
            assert b.normals().tobytes() == nb.tobytes()


def test_non_finite_points_and_an_empty_index_in_the_batch(gpu_ctx):
    rng = np.random.default_rng(72)
    c = rng.uniform(-8.0, 8.0, (300, 3)).astype(np.float32)
    bad = rng.choice(300, 9, replace=False)
    c[bad, rng.integers(0, 3, 9)] = np.float32([np.nan, np.inf, -np.inf] * 3)
    other = rng.uniform(-8.0, 8.0, (100, 3)).astype(np.float32)
    all_bad = np.full((5, 3), np.nan, np.float32)
    a, e, z, b = gpu_ctx.search_index(c), gpu_ctx.search_index(np.zeros((0, 3), np.float32)), gpu_ctx.search_index(all_bad), gpu_ctx.search_index(other)
    gpu_ctx.estimate_normals([a, e, z, b], 10)
    got = a.normals()
    assert np.isnan(got[bad]).all() and np.isfinite(np.delete(got, bad, axis=0)).all()
    _compare(got, nref.estimate(c, 10), "300 points, 9 of them not finite")
    assert e.normals().shape == (0, 4) and e.normals_k() == 10
    assert np.isnan(z.normals()).all() and z.normals().shape == (5, 4)
    _compare(b.normals(), nref.estimate(other, 10), "behind the empty indices")
    for i in (a, e, z, b):
        i.close()


def _scan_set(gpu_ctx, clouds):
    pts = np.concatenate([np.concatenate([c, np.zeros((len(c), 1), np.float32)], axis=1) for c in clouds])
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.uint64)
    return gpu_ctx.upload_scans(pts, off)


def test_one_batch_of_mixed_handles_equals_each_alone(gpu_ctx):
    """handles of ltm_search_build and ltm_search_build_scanset in one call: the bytes are those of estimating each index alone, with its own viewpoint,
    and the whole batch is one launch however many indices it holds"""
    rng = np.random.default_rng(73)
    clouds = [rng.uniform(-8.0, 8.0, (n, 3)).astype(np.float32) for n in (500, 70, 257, 1000, 33)]
    vps = rng.uniform(-3.0, 3.0, (5, 3)).astype(np.float32)
    live0 = gpu_ctx.pool_live()
    ss = _scan_set(gpu_ctx, clouds[:3])
    batch = gpu_ctx.search_index_batch(ss) + [gpu_ctx.search_index(c) for c in clouds[3:]]
    order = [3, 0, 4, 2, 1]
    for k in (12, 24):
        gpu_ctx.profile_enable(True)
        try:
            launches = {}
            for what, sel in (("one", order[:1]), ("five", order)):
                gpu_ctx.profile_reset()
                gpu_ctx.estimate_normals([batch[j] for j in sel], k, vps[sel])
                launches[what] = gpu_ctx.profile_read()["normals"]["launches"]
        finally:
            gpu_ctx.profile_enable(False)
        assert launches == {"one": 1, "five": 1}, launches
        together = [i.normals() for i in batch]
        for j, (c, i) in enumerate(zip(clouds, batch)):
            with gpu_ctx.search_index(c) as alone:
                alone.estimate_normals(k, vps[j])
                assert alone.normals().tobytes() == together[j].tobytes(), (k, j)
            _compare(together[j], nref.estimate(c, k, vps[j]), f"batch member {j}, k = {k}")
    for i in batch:
        i.close()
    ss.free()
    assert gpu_ctx.pool_live() == live0


def test_estimating_again_replaces_and_the_pool_is_clean(gpu_ctx, ltm):
    rng = np.random.default_rng(74)
    c1, c2 = (rng.uniform(-8.0, 8.0, (n, 3)).astype(np.float32) for n in (400, 150))
    live0 = gpu_ctx.pool_live()
    a = gpu_ctx.search_index(c1)
    blocks_a = gpu_ctx.pool_live()[0] - live0[0]
    b = gpu_ctx.search_index(c2)
    live1 = gpu_ctx.pool_live()
    with pytest.raises(ltm.LtmError) as e:
        a.normals()      # no normals yet
    assert e.value.code == -1
    gpu_ctx.estimate_normals([a, b], 8)
    assert gpu_ctx.pool_live()[0] == live1[0] + 1, "one pool block per call, shared by its handles"
    first = a.normals()
    a.estimate_normals(20)      # a keeps a block of its own now; b still holds the shared one
    assert gpu_ctx.pool_live()[0] == live1[0] + 2
    assert a.normals_k() == 20 and b.normals_k() == 8
    assert a.normals().tobytes() != first.tobytes()
    _compare(a.normals(), nref.estimate(c1, 20), "estimated again with k = 20")
    _compare(b.normals(), nref.estimate(c2, 8), "left alone")
    b.estimate_normals(8)       # the last reference to the shared block goes
    assert gpu_ctx.pool_live()[0] == live1[0] + 2
    # error paths leave the pool and the indices as they were: bad k, a handle twice, a non-finite viewpoint
    live2 = gpu_ctx.pool_live()
    th = (C.c_void_p * 2)(a.h, a.h)
    assert gpu_ctx.lib.ltm_search_estimate_normals(gpu_ctx.h, 2, th, 10, None) == -1
    for k in (2, 65, 0, -1):
        assert gpu_ctx.lib.ltm_search_estimate_normals(gpu_ctx.h, 1, th, k, None) == -1
    vp = np.float32([0.0, np.nan, 0.0])
    assert gpu_ctx.lib.ltm_search_estimate_normals(gpu_ctx.h, 1, th, 10, vp.ctypes.data) == -1
    assert gpu_ctx.pool_live() == live2 and a.normals_k() == 20
    a.close()
    assert gpu_ctx.pool_live()[0] == live1[0] + 2 - (blocks_a + 1)      # a's index blocks and its normals are back, b's normals remain
    b.close()
    assert gpu_ctx.pool_live() == live0


def test_foreign_and_freed_handles_are_refused(gpu_ctx, ltm):
    rng = np.random.default_rng(75)
    c = rng.uniform(-8.0, 8.0, (50, 3)).astype(np.float32)
    other = ltm.Context(vfov=50.0, hfov=360.0, device=0)
    theirs, mine, gone = other.search_index(c), gpu_ctx.search_index(c), gpu_ctx.search_index(c)
    gone_h = gone.h
    gone.close()
    live0 = gpu_ctx.pool_live()
    out = np.zeros((50, 4), np.float32)
    k = C.c_int(-7)
    for h in (theirs.h, gone_h):
        th = (C.c_void_p * 2)(mine.h, h)
        assert gpu_ctx.lib.ltm_search_estimate_normals(gpu_ctx.h, 2, th, 10, None) == -1
        assert gpu_ctx.lib.ltm_search_normals_info(gpu_ctx.h, h, C.byref(k), None) == -1
        assert gpu_ctx.lib.ltm_search_normals_download(gpu_ctx.h, h, out.ctypes.data) == -1
    assert mine.normals_k() == 0, "a refused call changes no index"
    assert gpu_ctx.pool_live() == live0
    mine.close()
    theirs.close()
    other.close()
