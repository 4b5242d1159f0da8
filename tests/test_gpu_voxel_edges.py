"""The voxel-centroid grid (ltm_voxel_centroid and its _batch / _shard / _box / _scanset forms) on the edge cases of tests/voxel_cases.py, against the oracle:
clouds bitwise and by point count, no tolerance anywhere.  Two contexts: the default one (fused head/scan/starts kernel, identity speculation) and one created
with LTM_VOXEL_FUSED_TAIL=0 LTM_VOXEL_IDENTITY=0 (the four-kernel tail, no speculation).  tests/test_voxel_cases_cpu.py shows on the host that the oracle and an
independent numpy restatement agree on every one of these fixtures and that every fixture holds the property it is named for."""
import os

import numpy as np
import pytest

import voxel_cases as vc
from conftest import assert_clouds_equal

pytestmark = pytest.mark.gpu

TAGS = ("default", "plain")
PLAIN_ENV = dict(LTM_VOXEL_FUSED_TAIL=0, LTM_VOXEL_IDENTITY=0)


def _ctx_with(ltm, **env):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (there is no CPU fallback)")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return ltm.Context(vfov=50.0, hfov=360.0, device=0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.fixture(scope="module")
def ctxs(ltm):
    """{"default": the library as it runs, "plain": four-kernel tail and no identity speculation}"""
    out = {"default": _ctx_with(ltm), "plain": _ctx_with(ltm, **PLAIN_ENV)}
    yield out
    for c in out.values():
        c.close()


def _grid(ctx, pts, leaf):
    return ctx.voxel_centroid(ctx.upload(pts), leaf).download()


# ------------------------------------------------------------------------------------------------- lattice edges
@pytest.mark.parametrize("leaf", vc.LEAVES)
@pytest.mark.parametrize("tag", TAGS)
def test_lattice_edge_clouds_equal_the_oracle(ctxs, tag, leaf):
    ctx = ctxs[tag]
    for index, (label, pts) in enumerate(vc.lattice_cases(leaf)):
        assert_clouds_equal(_grid(ctx, pts, leaf), vc.expected("lattice", leaf, index), f"{tag}: {label}")


@pytest.mark.parametrize("leaf", vc.LEAVES)
@pytest.mark.parametrize("tag", TAGS)
def test_lattice_edge_cloud_through_batch_shards_and_box(ctxs, tag, leaf):
    ctx = ctxs[tag]
    label, pts = vc.lattice_forms_case(leaf)
    index = [lb for lb, _ in vc.lattice_cases(leaf)].index(label)
    want = vc.expected("lattice", leaf, index)
    other_label, other = vc.lattice_cases(leaf)[0]
    g, g_other = ctx.upload(pts), ctx.upload(other)
    outs = ctx.voxel_centroid_batch([g, g_other, g], [leaf] * 3)
    assert_clouds_equal(outs[0].download(), want, f"{tag}: {label}: batch job 0")
    assert_clouds_equal(outs[1].download(), vc.expected("lattice", leaf, 0), f"{tag}: {other_label}: batch job 1")
    assert_clouds_equal(outs[2].download(), want, f"{tag}: {label}: batch job 2")
    parts = [ctx.voxel_centroid_shard(g, leaf, r, 3).download() for r in range(3)]
    assert_clouds_equal(np.concatenate(parts), want, f"{tag}: {label}: three shards")
    mn, mx = ctx.bbox(g)
    assert (mn == pts[:, :3].min(0)).all() and (mx == pts[:, :3].max(0)).all()
    assert_clouds_equal(ctx.voxel_centroid_box(g, mn, mx, leaf).download(), want, f"{tag}: {label}: box")


# ------------------------------------------------------------------------------------------------- segment edges
@pytest.mark.parametrize("name", sorted(vc.SEGMENT_BUILDERS))
def test_segment_edge_clouds_equal_the_oracle_in_both_contexts(ctxs, name):
    """one voxel_centroid call per cloud and context (the two look-back cases are the largest inputs of the file)"""
    for index, (label, pts) in enumerate(vc.segment_cases(name)):
        want = vc.expected("segments", name, index)
        got = {tag: _grid(ctxs[tag], pts, vc.SEG_LEAF) for tag in TAGS}
        for tag in TAGS:
            assert_clouds_equal(got[tag], want, f"{tag}: {label}")
        assert_clouds_equal(got["default"], got["plain"], f"{label}: fused tail against the four-kernel tail")


@pytest.mark.parametrize("tag", TAGS)
def test_tile_edge_and_straddle_sizes_in_one_batch(ctxs, tag):
    ctx = ctxs[tag]
    jobs = [(name, index, label, pts) for name in ("tile_edge", "straddle") for index, (label, pts) in enumerate(vc.segment_cases(name))]
    assert sorted(len(j[3]) for j in jobs) == sorted(list(vc.TILE_EDGE_N) + [12402])
    outs = ctx.voxel_centroid_batch([ctx.upload(j[3]) for j in jobs], [vc.SEG_LEAF] * len(jobs))
    for (name, index, label, _), out in zip(jobs, outs):
        assert_clouds_equal(out.download(), vc.expected("segments", name, index), f"{tag}: batch job {label}")


@pytest.mark.parametrize("name", sorted(vc.UNPACKED_COUNTS))
def test_unpacked_segment_edge_clouds_equal_the_oracle_in_both_contexts(ctxs, name):
    (label, pts), = vc.unpacked_cases(name)
    want = vc.expected("unpacked", name, 0)
    for tag in TAGS:
        assert_clouds_equal(_grid(ctxs[tag], pts, vc.UNPACKED_LEAF), want, f"{tag}: {label}")


# ------------------------------------------------------------------------------------------------- stale frames
def _write_in_place(ctx, cloud, rows):
    """overwrites a device cloud through the zero-copy view that removerter.cloud_to_tensor hands out; the cloud keeps whatever frame it carries"""
    import torch
    from ltmapper_amd.removerter import _DeviceArray
    ctx.synchronize()
    view = torch.as_tensor(_DeviceArray(cloud.device_ptr(), (len(cloud), 4), "<f4"), device=f"cuda:{ctx.device}")
    assert tuple(view.shape) == rows.shape
    view.copy_(torch.from_numpy(np.array(rows, dtype=np.float32)))
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def stale_base(ctxs):
    """the base cloud gridded on the device: its own grid, carrying the frame"""
    ctx = ctxs["default"]
    g = vc.stale_base()[0]
    ctx.voxel_stats(reset=True)
    base = ctx.voxel_centroid(ctx.upload(g), vc.STALE_LEAF)
    assert ctx.voxel_stats() == (1, 0), "an uploaded cloud carries no frame"
    assert_clouds_equal(base.download(), g, "the base is its own grid")
    return base, g


@pytest.mark.parametrize("index", range(2 * len(vc.STALE_ROWS) + 4 + 3))
def test_a_cloud_written_in_place_is_regridded_unless_it_still_is_its_own_grid(ctxs, orc, stale_base, index):
    ctx = ctxs["default"]
    base, g = stale_base
    m = vc.stale_mutations()[index]
    want = orc.voxel_centroid(m.cloud, vc.STALE_LEAF)
    assert_clouds_equal(want, m.expected, f"{m.label}: the oracle on the mutated array")
    stale, untouched = base.clone(), base.clone()           # clones keep the frame
    _write_in_place(ctx, stale, m.cloud)
    assert_clouds_equal(stale.download(), m.cloud, f"{m.label}: the write")
    ctx.voxel_stats(reset=True)
    got = ctx.voxel_centroid(stale, vc.STALE_LEAF)
    stats = ctx.voxel_stats()
    assert_clouds_equal(got.download(), want, f"{m.label}: single")
    assert stats == (1, 1 if m.identity else 0), f"{m.label}: (grids, identity hits) = {stats}"
    ctx.voxel_stats(reset=True)
    b_stale, b_untouched = ctx.voxel_centroid_batch([stale, untouched], [vc.STALE_LEAF] * 2)
    stats = ctx.voxel_stats()
    assert_clouds_equal(b_stale.download(), want, f"{m.label}: batch, the mutated job")
    assert_clouds_equal(b_untouched.download(), g, f"{m.label}: batch, the untouched clone")
    assert stats == (2, 2 if m.identity else 1), f"{m.label}: batch (grids, identity hits) = {stats}"


def test_the_frame_travels_with_a_cloud_lent_or_given_to_a_lane(ctxs, stale_base):
    ctx = ctxs["default"]
    base, g = stale_base
    lane = ctx.lane()
    try:
        ctx.fence(lane)
        view = ctx.lend(base, lane)
        lane.voxel_stats(reset=True)
        assert_clouds_equal(lane.voxel_centroid(view, vc.STALE_LEAF).download(), g, "lent: re-grid on the lane")
        assert lane.voxel_stats() == (1, 1), "lent: an identity hit"
        view.free()
        moved = ctx.give(base.clone(), lane)
        lane.voxel_stats(reset=True)
        assert_clouds_equal(lane.voxel_centroid(moved, vc.STALE_LEAF).download(), g, "given: re-grid on the lane")
        assert lane.voxel_stats() == (1, 1), "given: an identity hit"
        lane.voxel_stats(reset=True)
        assert len(lane.voxel_centroid(moved, 0.4)) < len(g)
        assert lane.voxel_stats() == (1, 0), "another leaf than the frame's: no identity hit"
        moved.free()
        lane.synchronize()
    finally:
        lane.close()


# ------------------------------------------------------------------------------------------------- scan sets
@pytest.mark.parametrize("tag", TAGS)
def test_scan_set_of_mixed_depths_repeated_clouds_and_empty_keyframes(ctxs, orc, tag):
    ctx = ctxs[tag]
    kfs = vc.scanset_case()
    off = np.cumsum([0] + [len(k) for k in kfs]).astype(np.uint64)
    got_pts, got_off = ctx.voxel_centroid_scanset(ctx.upload_scans(np.concatenate(kfs), off), vc.SCANSET_LEAF).download()
    assert len(got_off) == len(kfs) + 1
    at = 0
    for k, pts in enumerate(kfs):
        want = orc.voxel_centroid(pts, vc.SCANSET_LEAF) if len(pts) else np.zeros((0, 4), np.float32)
        assert (int(got_off[k]), int(got_off[k + 1])) == (at, at + len(want)), f"{tag}: offsets of keyframe {k}"
        assert_clouds_equal(got_pts[at:at + len(want)], want, f"{tag}: keyframe {k}")
        at += len(want)
    assert at == len(got_pts)
