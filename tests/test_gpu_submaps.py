"""The loop submaps on the device: ltm_submaps_assemble against the numpy restatement (tools/submap_numpy.py) and against the existing voxel grid,
ltm_search_build_scanset against the single build (query results byte for byte), ltm_icp_align_scanset against the cloud form, and Context.verify_loops
against the same pipeline put together from the calls that existed before (scan_of_keyframe, a numpy float transform, upload_scans, voxel_grid_scanset,
search_index, icp_align).  Everything is compared bit for bit: both sides run the same float operations in the same order.

Non-finite points: a NaN the host makes (x86: sign bit set) and one the device makes (sign bit clear) differ in their bits, and what the voxel grid does
with a NaN depends on its bits (its bounding box orders floats by their bits).  So the gather test, whose scan set holds a NaN and an infinite point,
compares the finite / non-finite masks and the finite points, as the interface promises; the grid tests against the RESTATEMENT use the same scan set
without those two points, and one more grid test keeps them and compares against the existing grid applied to the device's own ungridded output."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import icp_fixtures as fx
from tools import submap_numpy as ref

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 1000, 3]      # an empty first keyframe and the edges of the gather's 256-point workgroups
KEYS = [-3, 0, 3, 6, 9, 100]
SEARCH_NUMS = (0, 2, 25)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def gather_scene(with_bad):
    """(points, offsets, affines): 7 keyframes within 30 m; with_bad puts one NaN and one infinite coordinate in; seeded poses whose translations run from
    metres to kilometres"""
    rng = np.random.default_rng(7)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
    pts = np.concatenate([rng.uniform(-30.0, 30.0, (int(off[-1]), 3)), rng.uniform(0.0, 255.0, (int(off[-1]), 1))], axis=1).astype(np.float32)
    pts[5, 1] = -0.0
    if with_bad:
        pts[300, 2] = np.nan
        pts[900, 0] = np.inf
    poses = np.concatenate([rng.uniform(-1.0, 1.0, (len(SIZES), 3)) * np.array([3.0, 30.0, 300.0, 3000.0, 5.0, 50.0, 500.0])[:, None],
                            rng.uniform(-np.pi, np.pi, (len(SIZES), 3))], axis=1).astype(np.float32)
    from ltmapper_amd import capi
    return pts, off, capi.pose6d_to_affine3f(poses)


def _same_scanset(got, want_pts, want_off, what):
    assert (got.offsets() == want_off).all(), (what, got.offsets(), want_off)
    g = got.download()[0]
    assert (_bits(g) == _bits(want_pts)).all(), what


@pytest.mark.parametrize("search_num", SEARCH_NUMS)
@pytest.mark.parametrize("with_affines", (False, True))
def test_gather_alone(gpu_ctx, search_num, with_affines):
    pts, off, aff = gather_scene(True)
    aff = aff if with_affines else None
    want, want_off = ref.assemble(pts, off, KEYS, search_num, aff)
    scans = gpu_ctx.upload_scans(pts, off)
    live = gpu_ctx.pool_live()
    out = gpu_ctx.loop_submaps(scans, KEYS, search_num, leaf=0.0, affines=aff)
    assert (out.offsets() == want_off).all()
    got = out.download()[0]
    fin_g, fin_w = np.isfinite(got[:, :3]).all(axis=1), np.isfinite(want[:, :3]).all(axis=1)
    assert (fin_g == fin_w).all()
    assert (~fin_w).any() and fin_w.any()      # key 3 always brings the keyframe with the NaN point in
    assert (_bits(got[fin_w]) == _bits(want[fin_w])).all()
    assert (_bits(got[:, 3]) == _bits(want[:, 3])).all()      # the intensity is copied whatever the coordinates are
    if not with_affines and len(got):
        assert not (np.signbit(got[fin_w, :3]) & (got[fin_w, :3] == 0.0)).any()      # the identity still runs: -0.0 became +0.0
    out.free()
    assert gpu_ctx.pool_live() == live
    scans.free()


@pytest.mark.parametrize("with_affines", (False, True))
def test_grid_pcl_order_is_the_existing_grid_of_the_restatement(gpu_ctx, with_affines):
    pts, off, aff = gather_scene(False)
    aff = aff if with_affines else None
    scans = gpu_ctx.upload_scans(pts, off)
    for search_num in SEARCH_NUMS:
        want, want_off = ref.assemble(pts, off, KEYS, search_num, aff)
        cat = gpu_ctx.upload_scans(want, want_off)
        grid = gpu_ctx.voxel_grid_scanset(cat, 0.3)
        out = gpu_ctx.loop_submaps(scans, KEYS, search_num, leaf=0.3, affines=aff, order="pcl")
        assert 0 < grid.info()[1] <= len(want)
        _same_scanset(out, grid.download()[0], grid.offsets(), f"search_num {search_num}")
        for h in (cat, grid, out):
            h.free()
    scans.free()


def test_grid_input_order_is_the_existing_grid_with_the_variable_set(gpu_ctx):
    """order = 0 is LTM_VOXELGRID_ORDER=input of the existing entry point, which reads the variable on every call; with the variable set the other way the
    new call still does what its argument says"""
    pts, off, aff = gather_scene(False)
    scans = gpu_ctx.upload_scans(pts, off)
    want, want_off = ref.assemble(pts, off, KEYS, 25, aff)
    cat = gpu_ctx.upload_scans(want, want_off)
    old = os.environ.get("LTM_VOXELGRID_ORDER")
    try:
        os.environ["LTM_VOXELGRID_ORDER"] = "input"
        grid_in = gpu_ctx.voxel_grid_scanset(cat, 0.3)
        out_pcl = gpu_ctx.loop_submaps(scans, KEYS, 25, leaf=0.3, affines=aff, order="pcl")
    finally:
        if old is None:
            del os.environ["LTM_VOXELGRID_ORDER"]
        else:
            os.environ["LTM_VOXELGRID_ORDER"] = old
    grid_pcl = gpu_ctx.voxel_grid_scanset(cat, 0.3)
    out_in = gpu_ctx.loop_submaps(scans, KEYS, 25, leaf=0.3, affines=aff, order="input")
    _same_scanset(out_in, grid_in.download()[0], grid_in.offsets(), "input order")
    _same_scanset(out_pcl, grid_pcl.download()[0], grid_pcl.offsets(), "pcl order under LTM_VOXELGRID_ORDER=input")
    for h in (cat, grid_in, grid_pcl, out_in, out_pcl, scans):
        h.free()


def test_grid_keeps_the_existing_treatment_of_non_finite_points(gpu_ctx):
    """the scan set WITH the NaN and the infinite point: the gridded output is the existing grid applied to the ungridded output, both orders"""
    pts, off, aff = gather_scene(True)
    scans = gpu_ctx.upload_scans(pts, off)
    cat = gpu_ctx.loop_submaps(scans, KEYS, 25, leaf=0.0, affines=aff)
    for order in ("pcl", "input"):
        old = os.environ.get("LTM_VOXELGRID_ORDER")
        try:
            if order == "input":
                os.environ["LTM_VOXELGRID_ORDER"] = "input"
            grid = gpu_ctx.voxel_grid_scanset(cat, 0.3)
        finally:
            if order == "input":
                if old is None:
                    del os.environ["LTM_VOXELGRID_ORDER"]
                else:
                    os.environ["LTM_VOXELGRID_ORDER"] = old
        out = gpu_ctx.loop_submaps(scans, KEYS, 25, leaf=0.3, affines=aff, order=order)
        _same_scanset(out, grid.download()[0], grid.offsets(), order)
        grid.free()
        out.free()
    cat.free()
    scans.free()


def test_leaf_too_small_passes_the_transformed_input_through(gpu_ctx):
    """60 m at 1e-3 m is 6e4 cells per axis: more than INT32_MAX in all, PCL's "leaf size is too small" early-out for every window of two points or more"""
    pts, off, aff = gather_scene(False)
    scans = gpu_ctx.upload_scans(pts, off)
    want, want_off = ref.assemble(pts, off, KEYS, 2, aff)
    out = gpu_ctx.loop_submaps(scans, KEYS, 2, leaf=1e-3, affines=aff)
    _same_scanset(out, want, want_off, "pass-through")
    out.free()
    scans.free()


def test_invalid_arguments_and_pool(gpu_ctx, ltm):
    pts, off, aff = gather_scene(False)
    scans = gpu_ctx.upload_scans(pts, off)
    big = gpu_ctx.upload_scans(np.zeros((1 << 20, 4), np.float32), np.array([0, 1 << 20], np.uint64))
    live = gpu_ctx.pool_live()
    lib, out = gpu_ctx.lib, C.c_uint64()
    keys = np.asarray(KEYS, np.int32)

    def call(scanset=None, search_num=2, leaf=0.3, order=1, k=keys):
        return lib.ltm_submaps_assemble(gpu_ctx.h, (scans if scanset is None else scanset).h, None, k.ctypes.data, k.size, search_num, leaf, order, C.byref(out))

    assert call(search_num=-1) == -1
    assert call(leaf=-0.3) == -1 and call(leaf=float("nan")) == -1 and call(leaf=float("inf")) == -1
    assert call(order=2) == -1 and call(order=-1) == -1
    assert lib.ltm_submaps_assemble(gpu_ctx.h, 0xdead, None, keys.ctypes.data, keys.size, 2, 0.3, 1, C.byref(out)) == -1
    assert lib.ltm_submaps_assemble(gpu_ctx.h, scans.h, None, keys.ctypes.data, keys.size, 2, 0.3, 1, None) == -1
    # 4096 windows of one 2^20-point keyframe reach the 32-bit point-index limit of the grid: refused from the host offsets, before anything is allocated
    assert call(scanset=big, search_num=0, leaf=0.0, k=np.zeros(4096, np.int32)) == -4
    assert call(scanset=big, search_num=0, leaf=0.3, k=np.zeros(4096, np.int32)) == -4
    hs = (C.c_void_p * 8)()
    assert lib.ltm_search_build_scanset(gpu_ctx.h, scans.h, 3, 8, hs) == -1 and lib.ltm_search_build_scanset(gpu_ctx.h, scans.h, 4, 3, hs) == -1
    assert lib.ltm_search_build_scanset(gpu_ctx.h, scans.h, 0, 7, None) == -1
    assert gpu_ctx.pool_live() == live
    assert call(k=np.zeros(0, np.int32)) == 0      # no window: an empty scan set
    empty = ltm.ScanSet(gpu_ctx, out.value)
    assert empty.info() == (0, 0)
    empty.free()
    assert gpu_ctx.pool_live() == live
    big.free()
    scans.free()


# ---------------------------------------------------------------------------------------------------------------- batched build
BUILD_SIZES = [0, 1, 31, 32, 33, 1025, 5000]      # the 32-point leaf and the power-of-two leaf counts of the box tree


@functools.lru_cache(maxsize=None)
def build_scene():
    rng = np.random.default_rng(17)
    off = np.concatenate([[0], np.cumsum(BUILD_SIZES)]).astype(np.uint64)
    pts = np.concatenate([rng.uniform(-8.0, 8.0, (int(off[-1]), 3)), np.zeros((int(off[-1]), 1))], axis=1).astype(np.float32)
    a, b = int(off[2]), int(off[3])
    pts[a:b, :3] = np.float32([np.nan, np.inf, -np.inf])[rng.integers(0, 3, (b - a, 3))]      # keyframe 2 (31 points): nothing finite
    pts[a:b, 0] = np.nan
    a, b = int(off[4]), int(off[5])
    pts[a:b, :3] = np.float32([1.0, -2.0, 0.5]) + np.linspace(-4.0, 4.0, b - a, dtype=np.float32)[:, None] * np.float32([1.0, 0.5, 0.25])   # keyframe 4: a line
    a = int(off[5])
    pts[a + 100:a + 300, :3] = pts[a + 100, :3]      # keyframe 5: 200 exact duplicates of one point
    pts[int(off[6]) + 7, 1] = np.nan                 # and one non-finite point among the 5000
    queries = np.concatenate([rng.uniform(-9.0, 9.0, (497, 3)), pts[a + 100:a + 101, :3], [[np.nan, 0.0, 0.0]], [[100.0, 100.0, 100.0]]]).astype(np.float32)
    return pts, off, queries


def _same_queries(a, b, q, what):
    assert a.info() == b.info(), what
    for k in (1, 8):
        ia, da = a.knn(q, k)
        ib, db = b.knn(q, k)
        assert (ia == ib).all() and (_bits(da) == _bits(db)).all(), (what, "knn", k)
    for max_nn in (0, 5):
        ra, rb = a.radius(q, 1.5, max_nn), b.radius(q, 1.5, max_nn)
        assert (ra[0] == rb[0]).all() and (ra[1] == rb[1]).all() and (_bits(ra[2]) == _bits(rb[2])).all(), (what, "radius", max_nn)
    return a.info()


def test_batched_build_answers_like_the_single_build(gpu_ctx):
    pts, off, q = build_scene()
    scans = gpu_ctx.upload_scans(pts, off)
    qc = gpu_ctx.upload(np.concatenate([q, np.zeros((len(q), 1), np.float32)], axis=1))
    live = gpu_ctx.pool_live()
    batch = gpu_ctx.search_index_batch(scans)
    assert len(batch) == len(BUILD_SIZES)
    infos = []
    for kf, b in enumerate(batch):
        cloud = gpu_ctx.scan_of_keyframe(scans, kf)
        with gpu_ctx.search_index(cloud) as single:
            infos.append(_same_queries(b, single, qc, f"keyframe {kf}"))
        cloud.free()
    assert infos == [(0, 0), (1, 1), (31, 0), (32, 32), (33, 33), (1025, 1025), (5000, 4999)]
    # a sub-range is the same slice of the full batch
    part = gpu_ctx.search_index_batch(scans, 2, 6)
    assert len(part) == 4
    for j, p in enumerate(part):
        _same_queries(p, batch[2 + j], qc, f"sub-range keyframe {2 + j}")
    assert gpu_ctx.search_index_batch(scans, 3, 3) == []
    # handles go one by one, in any order; the blocks the batch shares return with the last of them
    for i in (5, 0, 6, 2, 4, 1):
        batch[i].close()
    _same_queries(batch[3], part[1], qc, "the last handle of a batch still answers")
    batch[3].close()
    for i in (2, 0, 3, 1):
        part[i].close()
    assert gpu_ctx.pool_live() == live
    qc.free()
    scans.free()


CHUNK_SIZES = [1023, 0, 1024, 2049]      # both sides of the 1024-point chunk of the segmented build kernels, an empty keyframe between, and past two chunks


@functools.lru_cache(maxsize=None)
def chunk_scene():
    rng = np.random.default_rng(23)
    off = np.concatenate([[0], np.cumsum(CHUNK_SIZES)]).astype(np.uint64)
    pts = np.concatenate([rng.uniform(-8.0, 8.0, (int(off[-1]), 3)), np.zeros((int(off[-1]), 1))], axis=1).astype(np.float32)
    pts[int(off[3]) + 2048, 2] = np.inf      # the one point of the last keyframe's third chunk is not finite
    queries = np.concatenate([rng.uniform(-9.0, 9.0, (254, 3)), [[np.nan, 0.0, 0.0]], [[100.0, 100.0, 100.0]]]).astype(np.float32)
    return pts, off, queries


def test_batched_build_at_the_chunk_edges_answers_like_the_single_build(gpu_ctx):
    pts, off, q = chunk_scene()
    scans = gpu_ctx.upload_scans(pts, off)
    qc = gpu_ctx.upload(np.concatenate([q, np.zeros((len(q), 1), np.float32)], axis=1))
    live = gpu_ctx.pool_live()
    batch = gpu_ctx.search_index_batch(scans)
    infos = []
    for kf, b in enumerate(batch):
        cloud = gpu_ctx.scan_of_keyframe(scans, kf)
        with gpu_ctx.search_index(cloud) as single:
            infos.append(_same_queries(b, single, qc, f"keyframe {kf}"))
        cloud.free()
    assert infos == [(1023, 1023), (0, 0), (1024, 1024), (2049, 2048)]
    for b in batch:
        b.close()
    assert gpu_ctx.pool_live() == live
    qc.free()
    scans.free()


def test_batched_build_serves_icp_like_the_single_build(gpu_ctx):
    near, far = fx.lattice_pair(), fx.lattice_pair(fx.FAR)
    tg = np.concatenate([near[0], far[0]])
    tg = np.concatenate([tg, np.zeros((len(tg), 1), np.float32)], axis=1)
    scans = gpu_ctx.upload_scans(tg, np.array([0, len(near[0]), len(tg)], np.uint64))
    batch = gpu_ctx.search_index_batch(scans)
    single = [gpu_ctx.search_index(near[0]), gpu_ctx.search_index(far[0])]
    got, gt = gpu_ctx.icp_align([(batch[0], near[1]), (batch[1], far[1])], trace=True)
    want, wt = gpu_ctx.icp_align([(single[0], near[1]), (single[1], far[1])], trace=True)
    assert got.tobytes() == want.tobytes() and gt.tobytes() == wt.tobytes()
    fx.check_known_answer(got[0], 1e-12)
    fx.check_known_answer(got[1], 1e-9)
    for i in batch + single:
        i.close()
    scans.free()


# ------------------------------------------------------------------------------------------------------- icp from a scan set
def test_icp_align_from_a_scan_set_is_the_cloud_form(gpu_ctx):
    t1, s1, _ = fx.scene_fixture("scene_2000_65")
    t2, s2 = fx.edge_pairs()[-1]      # 257 source points, five of them non-finite
    t3, s3 = fx.lattice_pair()
    srcs = [s1, s2, s3, np.zeros((0, 3), np.float32)]
    flat = np.concatenate(srcs)
    flat = np.concatenate([flat, np.zeros((len(flat), 1), np.float32)], axis=1)
    off = np.concatenate([[0], np.cumsum([len(s) for s in srcs])]).astype(np.uint64)
    sset = gpu_ctx.upload_scans(flat, off)
    idx = [gpu_ctx.search_index(t) for t in (t1, t2, t3)]
    order = [(idx[1], 1), (idx[0], 0), (idx[2], 2), (idx[2], 3), (idx[0], 0)]
    live = gpu_ctx.pool_live()
    got, gt = gpu_ctx.icp_align([(i, (sset, k)) for i, k in order], trace=True, max_iterations=40)
    assert gpu_ctx.pool_live() == live
    want, wt = gpu_ctx.icp_align([(i, srcs[k]) for i, k in order], trace=True, max_iterations=40)
    assert got.tobytes() == want.tobytes() and gt.tobytes() == wt.tobytes()
    assert got["converged"].tolist() == [1, 1, 1, 0, 1] and got["iterations"][3] == 0
    # a keyframe outside the set is refused
    res = np.zeros(1, got.dtype)
    th = (C.c_void_p * 1)(idx[0].h)
    kf = np.array([4], np.uint32)
    assert gpu_ctx.lib.ltm_icp_align_scanset(gpu_ctx.h, 1, th, sset.h, kf.ctypes.data, None, None, res.ctypes.data, None) == -1
    assert gpu_ctx.pool_live() == live
    for i in idx:
        i.close()
    sset.free()


# -------------------------------------------------------------------------------------------------------------- end to end
def _affines_of(ltm, poses16):
    """the 6-D poses of a synthetic session (planar: x, y, z, yaw) as float affines"""
    P = poses16.reshape(-1, 4, 4)
    p6 = np.stack([P[:, 0, 3], P[:, 1, 3], P[:, 2, 3], np.zeros(len(P)), np.zeros(len(P)), np.arctan2(P[:, 1, 0], P[:, 0, 0])], axis=1)
    return ltm.pose6d_to_affine3f(p6.astype(np.float32))


def _old_submap(ctx, scans, key, search_num, affines, leaf):
    """one gridded submap from calls the library had before: keyframe clouds down, numpy float transform, up as a one-keyframe scan set, voxel_grid_scanset"""
    n_kf = scans.n_kf
    parts = []
    for k in range(max(key - search_num, 0), min(key + search_num, n_kf - 1) + 1):
        c = ctx.scan_of_keyframe(scans, k)
        parts.append(ref.transform(c.download().reshape(-1, 4), affines[k]))
        c.free()
    cat = np.concatenate(parts)
    one = ctx.upload_scans(cat, np.array([0, len(cat)], np.uint64))
    grid = ctx.voxel_grid_scanset(one, leaf)
    out = ctx.scan_of_keyframe(grid, 0)
    one.free()
    grid.free()
    return out


def test_verify_loops_end_to_end(gpu_ctx, ltm):
    from tools import synth
    A = synth.to_numpy(synth.make_session(1, 8, "small"))
    B = synth.to_numpy(synth.make_session(2, 8, "small"))
    ta, sa = _affines_of(ltm, A["poses"]), _affines_of(ltm, B["poses"])
    tscans, sscans = gpu_ctx.upload_scans(A["scans"], A["offsets"]), gpu_ctx.upload_scans(B["scans"], B["offsets"])
    pairs = [(k, k) for k in range(8)] + [(3, 5)]      # target key 3 twice: its submap and index are made once
    icp = dict(max_iterations=30)
    live = gpu_ctx.pool_live()
    res, accept = gpu_ctx.verify_loops(tscans, sscans, pairs, ta, sa, search_num=2, leaf=0.3, **icp)
    assert gpu_ctx.pool_live() == live
    want = np.zeros(len(pairs), ltm.ICP_RESULT)
    for i, (tk, sk) in enumerate(pairs):
        tsub, ssub = _old_submap(gpu_ctx, tscans, tk, 2, ta, 0.3), _old_submap(gpu_ctx, sscans, sk, 0, sa, 0.3)
        with gpu_ctx.search_index(tsub) as idx:
            want[i] = gpu_ctx.icp_align([(idx, ssub)], **icp)[0]
        tsub.free()
        ssub.free()
    assert res.tobytes() == want.tobytes()
    want_accept = (want["converged"] != 0) & (want["fitness"] <= 0.5)
    assert (accept == want_accept).all()
    assert (res["iterations"] > 0).all() and (res["n_corr"] > 1000).all()
    # batches cut by the point budget give what one batch gives (a budget of one point: every pair alone)
    for budget in (1, 150000):
        res2, accept2 = gpu_ctx.verify_loops(tscans, sscans, pairs, ta, sa, search_num=2, leaf=0.3, max_batch_points=budget, **icp)
        assert res2.tobytes() == res.tobytes() and (accept2 == accept).all()
    # the LocalCoord form: no affines at all
    res3, _ = gpu_ctx.verify_loops(tscans, sscans, pairs[:2], search_num=2, leaf=0.3, **icp)
    assert (res3["iterations"] > 0).all()
    assert gpu_ctx.pool_live() == live
    tscans.free()
    sscans.free()
