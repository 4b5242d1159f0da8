"""The lifetime rule of the pointer handles, once per handle type, at the smallest shapes that take every branch: records of 0, 1 and
about 300 points, the last with a few non-finite ones.  Every refusal asked for here is an argument error that the library answers before it looks
inside the handle (include/ltm.h: a freed handle, one of another type, of another context or of a lane is LTM_E_INVALID), or a normal free."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 300
K = 5
# the C type behind every kind of handle made here, and the next C type in a ring: a live handle of THAT type is offered to this type's _info
RING = ("search", "search_result", "sc", "clusters", "planes", "outliers", "fpfh")
KINDS = {"index": "search", "index_batch": "search", "radius_result": "search_result", "scan_contexts": "sc", "clusters": "clusters",
         "planes_scans": "planes", "planes_cloud": "planes", "outliers_statistical": "outliers", "outliers_radius": "outliers", "fpfh": "fpfh"}


def _points(seed):
    """~300 points: a noisy ground plane and two blobs above it, so that planes, clusters and filters all find something"""
    rng = np.random.default_rng(seed)
    ground = np.c_[rng.uniform(-4.0, 4.0, (200, 2)), rng.normal(0.0, 0.01, 200)]
    blobs = np.concatenate([rng.normal((1.0, 1.0, 1.0), 0.05, (60, 3)), rng.normal((-2.0, 0.5, 1.5), 0.05, (N - 260, 3))])
    return np.c_[np.concatenate([ground, blobs]), np.zeros(N)].astype(np.float32)


def _info(lib, kind, ctx_h, h):
    fn = getattr(lib, f"ltm_{kind}_info")
    return fn(ctx_h, h, *([None] * (len(fn.argtypes) - 2)))


def _free(lib, kind, ctx_h, h):
    return getattr(lib, f"ltm_{kind}_free")(ctx_h, h)


class World:
    """a fresh context with the inputs uploaded once; make(what) builds one kind of handle from them and returns its raw pointers"""

    def __init__(self, ltm):
        self.ctx = ltm.Context(vfov=50.0, hfov=360.0, device=0)
        self.lib = self.ctx.lib
        last = _points(1)
        last[[7, 150, 299], :3] = [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf]]
        one = np.array([[1.0, 2.0, 3.0, 0.0]], np.float32)
        self.scan_points, self.scan_offsets = np.concatenate([one, last]), [0, 0, 1, 1 + N]
        self.scans = self.ctx.upload_scans(self.scan_points, self.scan_offsets)
        self.cloud = self.ctx.upload(_points(2))
        # what the derived sets are computed from: the batched indices of the scan set and the index of the cloud, all with normals
        self.indices = self.ctx.search_index_batch(self.scans) + [self.ctx.search_index(self.cloud)]
        self.ctx.estimate_normals(self.indices, K)
        self.kept = []

    def make(self, what):
        ctx = self.ctx
        if what == "index":
            made = [ctx.search_index(self.cloud)]
        elif what == "index_batch":
            made = ctx.search_index_batch(self.scans)
            ctx.estimate_normals(made, K)      # their shared normals block goes with them as well
        elif what == "radius_result":
            res = C.c_void_p()
            assert self.lib.ltm_radius_search(ctx.h, self.indices[-1].h, self.cloud.h, 0.3, 0, C.byref(res)) == 0
            return [res.value]
        elif what == "scan_contexts":
            made = [ctx.scan_contexts(self.scans)]
        elif what == "clusters":
            made = ctx.cluster(self.indices, 0.3)
        elif what == "planes_scans":
            made = [ctx.segment_planes(self.scans, 0.05)]
        elif what == "planes_cloud":
            made = [ctx.segment_plane(self.cloud, 0.05)]
        elif what == "outliers_statistical":
            made = [ctx.statistical_outliers(self.indices, 4, 1.0)]
        elif what == "outliers_radius":
            made = [ctx.radius_outliers(self.indices, 0.3, 2)]
        else:
            assert what == "fpfh"
            made = [ctx.fpfh(self.indices, K)]
        hs = [m.h for m in made]
        for m in made:
            m.h = None      # the test frees the raw pointers itself (or leaves them to ltm_destroy)
        return hs

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def world(ltm):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (there is no CPU fallback)")
    w = World(ltm)
    w.lane = w.ctx.lane()
    w.live = {KINDS[what]: w.make(what)[0] for what in ("index", "radius_result", "scan_contexts", "clusters", "planes_cloud", "outliers_radius", "fpfh")}
    yield w
    w.lane.close()
    w.close()      # ltm_destroy releases w.live


@pytest.mark.parametrize("what", list(KINDS))
def test_free_refusals_and_pool_balance(world, what):
    ctx, lib, kind = world.ctx, world.lib, KINDS[what]
    ctx.synchronize()
    before = ctx.pool_live()
    hs = world.make(what)
    h = hs[0]
    assert ctx.pool_live()[0] > before[0]
    assert _info(lib, kind, ctx.h, h) == 0
    # (b) a live handle of another type is not in this type's list
    other = world.live[RING[(RING.index(kind) + 1) % len(RING)]]
    assert _info(lib, kind, ctx.h, other) == -1, "a handle of another type was taken"
    # (c) a lane is another context; the refusals leave the handle as it was
    assert _info(lib, kind, world.lane.h, h) == -1
    assert _free(lib, kind, world.lane.h, h) == -1
    assert _info(lib, kind, ctx.h, h) == 0, "the handle no longer works on its own context"
    # (a) freed: no handle any more, and everything it held is back in the pool
    for x in hs:
        assert _free(lib, kind, ctx.h, x) == 0
    assert _info(lib, kind, ctx.h, h) == -1
    assert _free(lib, kind, ctx.h, h) == -1, "a freed handle was freed again"
    ctx.synchronize()
    assert ctx.pool_live() == before, "blocks of the freed handle are still handed out"


def test_counters_start_at_zero_count_and_reset(ltm):
    """(d) zeros before the first call of the feature on a fresh context, counting after, zeros after reset.  The first counter of every block is looked
    at: finite_points for the outlier filters and FPFH, point_hypothesis_tests for the planes, pairs_tested for the clusters (host-side sums)"""
    w = World(ltm)
    ctx = w.ctx
    try:
        for stats, whats in ((ctx.cluster_stats, ["clusters"]), (ctx.plane_stats, ["planes_scans", "planes_cloud"]),
                             (ctx.outlier_stats, ["outliers_statistical", "outliers_radius"]), (ctx.fpfh_stats, ["fpfh"])):
            zeros = stats()
            first = next(iter(zeros))
            assert first in ("pairs_tested", "point_hypothesis_tests", "finite_points")
            assert not any(zeros.values()), f"{first}: counters before the first call: {zeros}"
            assert not any(stats(reset=True).values()), "a reset before the first call"
            for what in whats:
                w.kept += w.make(what)      # left open: ltm_destroy releases them
            got = stats(reset=True)
            assert got[first] > 0, got
            assert not any(stats().values()), "counters after reset=True"
    finally:
        w.close()


def test_destroy_releases_every_open_handle_in_order(ltm):
    w = World(ltm)
    lane = w.ctx.lane()
    for what in KINDS:
        w.kept += w.make(what)
    for x in w.indices:
        x.h = None      # the indices the sets were computed from stay open as well
    theirs = lane.search_index(_points(3))
    theirs.h = None
    lane.close()
    w.close()
    # the process goes on, and a second fresh context works with a balanced pool
    ctx = ltm.Context(vfov=50.0, hfov=360.0, device=0)
    try:
        cloud = ctx.upload(_points(4))
        ctx.synchronize()
        before = ctx.pool_live()
        index = ctx.search_index(cloud)
        assert index.info() == (N, N)
        index.close()
        ctx.synchronize()
        assert ctx.pool_live() == before
    finally:
        ctx.close()


def _download(s):
    pts, off = s.download()
    return pts.view(np.uint32).tolist(), off.tolist()


def test_split_with_one_side_wanted(world, ltm):
    """FlagSplit::hand_over's "one side wanted" branch at the two call sites of ltm_api_knn.cpp: ltm_knn_partition with either output null gives the
    bytes of the full call's other side, ltm_preclean keeps one half by definition; the pool is balanced once the returned sets are freed"""
    ctx, lib = world.ctx, world.lib
    poses = ctx.poses(np.tile(np.eye(4), (3, 1, 1)))
    ctx.synchronize()
    before = ctx.pool_live()
    both = ctx.knn_partition(world.cloud, world.scans, poses, 2, 0.05)
    want = [_download(s) for s in both]
    assert want[0][1][-1] + want[1][1][-1] == 1 + N and want[0][1][-1] > 0 and want[1][1][-1] > 0, "both sides of the split should have points"
    for s in both:
        s.free()
    for side in (0, 1):
        out = C.c_uint64()
        args = [None, None]
        args[side] = C.byref(out)
        assert lib.ltm_knn_partition(ctx.h, world.cloud.h, world.scans.h, poses.h, 0, 3, 2, 0.05, *args) == 0
        got = ltm.ScanSet(ctx, out.value)
        assert _download(got) == want[side], f"side {side} alone differs from the full call"
        got.free()
        ctx.synchronize()
        assert ctx.pool_live() == before, f"side {side} alone left blocks handed out"
    kept = ctx.preclean(world.scans, 1.5)
    assert kept.offsets().tolist()[0] == 0 and 0 < kept.info()[1] < 1 + N
    kept.free()
    ctx.synchronize()
    assert ctx.pool_live() == before
