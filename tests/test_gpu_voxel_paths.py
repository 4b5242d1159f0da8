"""The voxel-centroid entry points (single, batch, shard, box) are one pipeline (csrc/ltm_api_voxel.cpp: VoxelJob, voxel_plan, voxel_centroid_jobs) and
the two scan-set grids share their tail (scanset_centroids).  These cases walk every branch of that pipeline at the smallest shapes that reach it:
the key/index-pair sort of a job whose code does not fit beside the index, a batch that mixes empty, identity, packed and unpacked jobs, the frame an
output does or does not carry, the clean-up after a job that throws, what the profile counts, and a ragged scan set through both scan-set grids."""
import os

import numpy as np
import pytest

from conftest import assert_clouds_equal

pytestmark = pytest.mark.gpu

WIDE_LEAF = 0.001


@pytest.fixture(scope="module")
def wide(ltm, orc):
    """1000 points in a 600 m cube at leaf 1 mm: octree depth 20 and every axis spans both halves of every level, so all 60 code bits are kept; with
    10 index bits the pair does not fit one 64-bit word: morton_keys, sort_pairs_u64, voxel_centroids (and compact_pairs in a shard) run"""
    rng = np.random.default_rng(2025)
    p = np.c_[rng.uniform(-300, 300, (1000, 3)), rng.uniform(0, 255, 1000)].astype(np.float32)
    bits, _, depth, _ = ltm.voxel_key_bits(p[:, :3].min(0), p[:, :3].max(0), WIDE_LEAF)
    assert (bits, depth) == (60, 20) and bits + 10 > 64
    return p, orc.voxel_centroid(p, WIDE_LEAF)


@pytest.fixture(scope="module")
def cube(orc):
    """3000 points in a 20 m cube: packed at leaf 0.05; its grid at 0.05 is the input of the identity jobs"""
    rng = np.random.default_rng(7)
    p = np.c_[rng.uniform(-10, 10, (3000, 3)), rng.uniform(0, 255, 3000)].astype(np.float32)
    return p, orc.voxel_centroid(p, 0.05)


def test_unpacked_job_through_every_entry_point(gpu_ctx, wide):
    p, want = wide
    g = gpu_ctx.upload(p)
    assert_clouds_equal(gpu_ctx.voxel_centroid(g, WIDE_LEAF).download(), want, "single")
    for k, out in enumerate(gpu_ctx.voxel_centroid_batch([g, g], [WIDE_LEAF, WIDE_LEAF])):
        assert_clouds_equal(out.download(), want, f"batch job {k}")
    parts = [gpu_ctx.voxel_centroid_shard(g, WIDE_LEAF, r, 3).download() for r in range(3)]
    assert all(len(q) for q in parts)
    assert_clouds_equal(np.concatenate(parts), want, "three shards")
    mn, mx = gpu_ctx.bbox(g)
    assert_clouds_equal(gpu_ctx.voxel_centroid_box(g, mn, mx, WIDE_LEAF).download(), want, "box")


def test_mixed_batch_equals_the_one_job_calls_and_the_oracle(gpu_ctx, ltm, orc, wide, cube):
    p_wide, _ = wide
    p_cube, grid_cube = cube
    one = np.array([[1, 2, 3, 4]], np.float32)
    gridded = gpu_ctx.voxel_centroid(gpu_ctx.upload(p_cube), 0.05)
    assert_clouds_equal(gridded.download(), grid_cube, "the grid the identity jobs start from")
    jobs = [(np.zeros((0, 4), np.float32), 0.05), (one, 0.05), (np.repeat(one, 1000, axis=0), 0.05), (p_cube, 0.05), (p_wide, WIDE_LEAF),
            (gridded, 0.05), (gridded, 0.4)]
    clouds = [c if isinstance(c, ltm.Cloud) else gpu_ctx.upload(c) for c, _ in jobs]
    leafs = [leaf for _, leaf in jobs]
    gpu_ctx.voxel_stats(reset=True)
    outs = gpu_ctx.voxel_centroid_batch(clouds, leafs)
    assert gpu_ctx.voxel_stats() == (6, 1), "six non-empty jobs, one of them the identity"
    for k, (c, leaf) in enumerate(zip(clouds, leafs)):
        got = outs[k].download()
        assert_clouds_equal(got, gpu_ctx.voxel_centroid(c, leaf).download(), f"job {k}: batch against single")
        assert_clouds_equal(got, orc.voxel_centroid(c.download(), leaf), f"job {k}: batch against the oracle")
    assert len(outs[0]) == 0 and len(outs[5]) == len(gridded)
    # only empty and identity jobs: nothing is sorted, no count is read
    gpu_ctx.voxel_stats(reset=True)
    outs = gpu_ctx.voxel_centroid_batch([clouds[0], gridded, clouds[0], gridded], [0.05] * 4)
    assert gpu_ctx.voxel_stats() == (2, 2)
    assert [len(o) for o in outs] == [0, len(gridded), 0, len(gridded)]
    for k in (1, 3):
        assert_clouds_equal(outs[k].download(), grid_cube, f"identity-only batch, job {k}")


def test_single_and_batch_outputs_carry_their_frame_shard_and_box_outputs_do_not(gpu_ctx, cube):
    p, want = cube
    g = gpu_ctx.upload(p)
    mn, mx = gpu_ctx.bbox(g)
    outs = {"single": gpu_ctx.voxel_centroid(g, 0.05), "batch": gpu_ctx.voxel_centroid_batch([g], [0.05])[0],
            "shard": gpu_ctx.voxel_centroid_shard(g, 0.05, 0, 1), "box": gpu_ctx.voxel_centroid_box(g, mn, mx, 0.05)}
    for what, out in outs.items():
        assert_clouds_equal(out.download(), want, what)
        gpu_ctx.voxel_stats(reset=True)
        again = gpu_ctx.voxel_centroid(out, 0.05)
        assert gpu_ctx.voxel_stats() == (1, 1 if what in ("single", "batch") else 0), what
        assert_clouds_equal(again.download(), want, f"{what}: re-grid at the same leaf")


def test_a_job_that_throws_returns_the_outputs_of_the_jobs_before_it(gpu_ctx, ltm, wide, cube):
    p_wide, _ = wide
    p_cube, grid_cube = cube
    gridded = gpu_ctx.voxel_centroid(gpu_ctx.upload(p_cube), 0.05)      # an identity job: its output is allocated while the batch is planned
    g_wide = gpu_ctx.upload(p_wide)
    before = gpu_ctx.pool_live()
    with pytest.raises(ltm.LtmError) as e:
        gpu_ctx.voxel_centroid_batch([gridded, g_wide], [0.05, 1e-5])    # 600 m / 1e-5 m: depth 26
    assert e.value.code == -4, "LTM_E_UNSUPPORTED"
    assert gpu_ctx.pool_live() == before
    assert_clouds_equal(gpu_ctx.voxel_centroid(gridded, 0.05).download(), grid_cube, "the context after the throw")
    with pytest.raises(ltm.LtmError) as e:
        gpu_ctx.voxel_centroid(g_wide, 1e-5)
    assert e.value.code == -4 and gpu_ctx.pool_live() == before


def test_profile_counts_one_voxel_launch_per_call(gpu_ctx, cube):
    p, _ = cube
    clouds = [gpu_ctx.upload(p[:n]) for n in (3000, 1, 500)]
    gpu_ctx.profile_enable(True)
    try:
        gpu_ctx.profile_reset()
        gpu_ctx.voxel_centroid_batch(clouds, [0.05, 0.05, 0.4])
        batch = gpu_ctx.profile_read()["voxel"]
        gpu_ctx.profile_reset()
        gpu_ctx.voxel_centroid(clouds[2], 0.05)
        single = gpu_ctx.profile_read()["voxel"]
    finally:
        gpu_ctx.profile_enable(False)
    assert (batch["launches"], batch["units"]) == (1, 3501.0)
    assert (single["launches"], single["units"]) == (1, 500.0)


def test_ragged_scan_set_through_both_scan_set_grids(gpu_ctx, orc):
    """keyframes of 0, 700, 0, 1, 900 (one voxel) and 0 points: empty first, middle and last keyframes, a one-point keyframe and a keyframe that is one
    segment, through the shared tail of ltm_voxel_centroid_scanset and ltm_voxel_grid_scanset (both orders)"""
    rng = np.random.default_rng(19)
    spot = np.c_[np.tile(np.float32([2.5, -1.25, 0.75]), (900, 1)), rng.uniform(0, 255, 900)]
    kfs = [np.zeros((0, 4)), np.c_[rng.uniform(-5, 5, (700, 3)), rng.uniform(0, 255, 700)], np.zeros((0, 4)),
           np.c_[rng.uniform(-1, 1, (1, 3)), [7.0]], spot, np.zeros((0, 4))]
    kfs = [k.astype(np.float32) for k in kfs]
    off = np.cumsum([0] + [len(k) for k in kfs]).astype(np.uint64)
    scans = gpu_ctx.upload_scans(np.concatenate(kfs), off)

    def check(got, want_of, what):
        g_pts, g_off = got.download()
        at = 0
        for k, pts in enumerate(kfs):
            want = want_of(pts)
            assert (int(g_off[k]), int(g_off[k + 1])) == (at, at + len(want)), f"{what}: offsets of keyframe {k}"
            assert_clouds_equal(g_pts[at:at + len(want)], want, f"{what}: keyframe {k}")
            at += len(want)
        assert at == len(g_pts)

    check(gpu_ctx.voxel_centroid_scanset(scans, 0.5), lambda pts: orc.voxel_centroid(pts, 0.5), "octree grid")
    assert len(orc.voxel_centroid(kfs[4], 0.5)) == 1 and len(orc.voxel_grid(kfs[4], 0.5, stable=True)) == 1
    old = os.environ.get("LTM_VOXELGRID_ORDER")
    try:
        for order in ("pcl", "input"):
            os.environ["LTM_VOXELGRID_ORDER"] = order
            check(gpu_ctx.voxel_grid_scanset(scans, 0.5), lambda pts: orc.voxel_grid(pts, 0.5, stable=(order == "input")), f"VoxelGrid, {order} order")
    finally:
        if old is None:
            del os.environ["LTM_VOXELGRID_ORDER"]
        else:
            os.environ["LTM_VOXELGRID_ORDER"] = old
