"""The fixtures of tests/voxel_cases.py mean something (no GPU needed): on every one of them the oracle's voxel grid and the module's numpy restatement
of it -- two independent statements of the same grid -- agree bit for bit, every case holds the property it is named for (the builders assert it from the
restatement's head positions; what can be said from outside is asserted again here), and the library's host arithmetic (ltm_debug_voxel_key_bits) derives the
restatement's depth and lattice origin from every fixture's box.  When tests/test_gpu_voxel_edges.py fails, this is what makes the device the odd one out."""
import math

import numpy as np
import pytest

import voxel_cases as vc
from conftest import assert_clouds_equal

F32 = np.float32


def _agree(orc, ltm, pts, leaf, what):
    """oracle == restatement (bits and counts); the library's frame of the cloud's box is the restatement's; returns the restatement and the kept key bits"""
    r = vc.restate(pts, leaf)
    assert_clouds_equal(orc.voxel_centroid(pts, leaf), r.centroids, f"{what}: oracle against the restatement")
    bits, _, depth, origin = ltm.voxel_key_bits(pts[:, :3].min(0), pts[:, :3].max(0), leaf)
    assert depth == r.frame.depth and (origin == r.frame.lo).all(), f"{what}: the library's frame {depth} {origin} against {r.frame}"
    return r, bits


def _near_a_face(pts, frame):
    """how many points change voxel when moved by one float on some axis on which the box has an extent"""
    p = pts[:, :3]
    key = lambda a: np.floor((a.astype(np.float64) - frame.lo) / frame.res)      # noqa: E731
    moved = (key(np.nextafter(p, F32(-np.inf))) != key(p)) | (key(np.nextafter(p, F32(np.inf))) != key(p))
    return int(moved[:, p.min(0) < p.max(0)].any(axis=1).sum())


@pytest.mark.parametrize("leaf", vc.LEAVES)
def test_lattice_edge_clouds(orc, ltm, leaf):
    cases = vc.lattice_cases(leaf)
    assert len(cases) == len(vc.CENTRES) * len(vc.EXTENTS) + 5 * len(vc.SWITCH_DEPTHS) and len({label for label, _ in cases}) == len(cases)
    for k, (label, pts) in enumerate(cases):
        assert pts.dtype == F32 and len(pts) <= 2100 and np.isfinite(pts).all()
        r, _ = _agree(orc, ltm, pts, leaf, label)
        assert _near_a_face(pts, r.frame) >= len(pts) // 4, f"{label}: points on or beside a voxel face"      # the rest were clipped onto the box
        assert 1 < len(r.heads) < len(pts), f"{label}: voxels of one point and of several"
        if k < len(vc.CENTRES) * len(vc.EXTENTS):
            centre, extent = vc.CENTRES[k // len(vc.EXTENTS)], vc.EXTENTS[k % len(vc.EXTENTS)]
            mn, mx = pts[:, :3].min(0), pts[:, :3].max(0)
            side = (1 << r.frame.depth) * r.frame.res
            for d in range(3):
                assert abs(float(mn[d]) - (centre - extent[d] / 2)) <= abs(centre) * 1e-7 + 1e-6
                if extent[d] == 0.0:          # a plane or a line: this axis has no extent and is centred by half the cube
                    assert mn[d] == mx[d] and abs((float(mn[d]) - r.frame.lo[d]) - side / 2) < 1e-3
            has_neg_zero = bool((pts[:, :3].view(np.uint32) == 0x80000000).any())
            assert has_neg_zero == (centre == 0.0), f"{label}: the -0.0 coordinate"
    depths = {label: vc.frame_of(pts, leaf).depth for label, pts in cases}
    for d in vc.SWITCH_DEPTHS:
        assert (depths[f"leaf{leaf}-depth{d}-last-float"], depths[f"leaf{leaf}-depth{d + 1}-first-float"]) == (d, d + 1)
        assert all(f"leaf{leaf}-switch{d}-{tag}" in depths for tag in ("minus", "exact", "plus"))
    label, pts = vc.lattice_forms_case(leaf)
    assert "centre-123.456-extent3" in label
    mn, mx = pts[:, :3].min(0), pts[:, :3].max(0)
    assert_clouds_equal(orc.voxel_centroid_box(pts, mn, mx, leaf), vc.restate(pts, leaf, box=(mn, mx)).centroids, f"{label}: box form")


@pytest.mark.parametrize("name", sorted(vc.SEGMENT_BUILDERS))
def test_segment_edge_clouds(orc, ltm, name):
    for label, pts in vc.segment_cases(name):           # the builder has asserted the head positions the case is named for
        assert len(pts) <= 140_000
        r, bits = _agree(orc, ltm, pts, vc.SEG_LEAF, label)
        assert_clouds_equal(vc.expected("segments", name, [lb for lb, _ in vc.segment_cases(name)].index(label)), r.centroids, label)
        assert bits + max(1, math.ceil(math.log2(len(pts)))) <= 64, f"{label}: code and index share one word (the packed kernels)"
        k = vc.keys_of(pts, r.frame)
        assert (k[:, :2] == k[0, :2]).all(), f"{label}: a line parallel to z"
    if name == "tile_edge":
        assert [len(p) for _, p in vc.segment_cases(name)] == list(vc.TILE_EDGE_N)


@pytest.mark.parametrize("name", sorted(vc.UNPACKED_COUNTS))
def test_unpacked_segment_edge_clouds(orc, ltm, name):
    (label, pts), = vc.unpacked_cases(name)
    r, bits = _agree(orc, ltm, pts, vc.UNPACKED_LEAF, label)
    assert r.frame.depth == 20 and bits == 60 and bits + math.ceil(math.log2(len(pts))) > 64
    assert (r.heads == np.r_[0, np.cumsum(vc.UNPACKED_COUNTS[name])[:-1]]).all()


def test_stale_frame_mutations(orc, ltm):
    g, ia, ca, ib, cb = vc.stale_base()
    assert len(g) == vc.STALE_N == 3000
    r, _ = _agree(orc, ltm, g, vc.STALE_LEAF, "the base")
    assert_clouds_equal(r.centroids, g, "the base is its own grid")
    assert (ia % 64, ib % 64) == (0, 63) and g[ia, ca].view(np.uint32) == 0 and g[ib, cb].view(np.uint32) == 0
    muts = vc.stale_mutations()
    labels = [m.label for m in muts]
    assert len(set(labels)) == len(labels) == 2 * len(vc.STALE_ROWS) + 4 + 3
    for i in vc.STALE_ROWS:
        assert f"swap({i})" in labels and f"dup({i})" in labels
    for m in muts:
        assert_clouds_equal(orc.voxel_centroid(m.cloud, vc.STALE_LEAF), m.expected, f"{m.label}: oracle")
        assert vc.same_frame(vc.frame_of(m.cloud, vc.STALE_LEAF), r.frame), m.label
        assert m.identity == m.label.startswith("benign")
        if not m.identity:
            assert m.cloud.shape != m.expected.shape or (m.cloud.view(np.uint32) != m.expected.view(np.uint32)).any(), f"{m.label}: a copy would pass"
        if m.label.startswith("swap") or m.label.startswith("negzero"):
            assert len(m.expected) == 3000
        if m.label.startswith("dup"):
            assert len(m.expected) == 2999


def test_scan_set_keyframes(orc, ltm):
    kfs = vc.scanset_case()
    sizes = [len(k) for k in kfs]
    assert sizes[0] == sizes[-1] == 0 and sizes.count(0) == 5 and sizes.count(2048) == 5
    depths = []
    for k, pts in enumerate(kfs):
        if len(pts):
            r, _ = _agree(orc, ltm, pts, vc.SCANSET_LEAF, f"keyframe {k}")
            depths.append(r.frame.depth)
    assert depths[:2] == [3, 15]
    assert kfs[4] is kfs[5] is kfs[6] and kfs[9] is kfs[10] and len(vc.restate(kfs[9], vc.SCANSET_LEAF).heads) == 1
