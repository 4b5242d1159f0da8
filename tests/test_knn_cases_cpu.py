"""The edge cases of tests/knn_cases.py mean something (no GPU needed): for every case the oracle's brute-force search and its kd-tree search --
two independent references -- give the same flags, both classes are populated, and the case reaches the branch it is named for as far as the
host's restatement of KnnIndex::build's grid frame can tell."""
import math

import numpy as np
import pytest

import knn_cases as kc

# cases that are one-class on purpose, or too small for a share to mean anything
SHARE_EXEMPT = {"bucketless": "every query coexists: the undecided count must be the bucket-less cells alone",
                "exact_threshold": "one query per variant, known answers checked below"}


def _both(orc, name, index):
    target, scans, off, poses, inv, k, thr = kc.cases(name)[index][1]
    brute, loc = kc.expected(name, index)
    tree, loc2 = orc.knn_labels(target, scans, off, poses, inv, kc.I4, k, thr, use_kdtree=True)
    return brute, tree, loc, loc2


@pytest.mark.parametrize("name", sorted(kc.BUILDERS))
def test_two_references_agree_and_both_classes_are_populated(orc, name):
    for index, (label, case) in enumerate(kc.cases(name)):
        target, scans, off, poses, inv, k, thr = case
        assert target.dtype == np.float32 and scans.dtype == np.float32 and off.dtype == np.uint64 and int(off[-1]) == len(scans)
        assert poses.shape == inv.shape == (len(off) - 1, 16)
        assert len(scans) * max(len(target), 1) <= 2e8, f"{label}: brute force too expensive"
        brute, tree, loc, loc2 = _both(orc, name, index)
        assert (brute == tree).all(), f"{label}: brute force and kd-tree disagree on {int((brute != tree).sum())} of {brute.size} queries"
        assert (np.nan_to_num(loc, nan=7.0).view(np.uint32) == np.nan_to_num(loc2, nan=7.0).view(np.uint32)).all()
        share = float(brute.mean()) if brute.size else 0.0
        if name == "bucketless":
            assert share == 1.0, f"{label}: share {share}"
        elif name == "small_targets":
            assert 0.1 <= share <= 0.9, f"{label}: coexist share {share}"       # holds for every (Mt, k), k > Mt included
        elif name not in SHARE_EXEMPT:
            assert 0.1 <= share <= 0.9, f"{label}: coexist share {share}"
        if label in kc.EXACT_THRESHOLD_EXPECT:
            assert int(brute[0]) == kc.EXACT_THRESHOLD_EXPECT[label], label
    if name == "exact_threshold":
        assert sum(1 for label, _ in kc.cases(name) if label in kc.EXACT_THRESHOLD_EXPECT) == 16


def test_exact_threshold_values_are_exact_in_float():
    q = np.float32(0.25)
    assert q * q == np.float32(0.0625) and float(q) ** 2 == 0.0625
    lo = np.nextafter(q, np.float32(0))
    assert lo * lo < np.float32(0.0625)
    assert np.float32(np.float64(q * q) + np.float64(q * q)) / np.float32(2) == np.float32(0.0625)
    t = np.float32(0.1)
    assert not (np.float32(np.float64(t * t) + np.float64(t * t)) / np.float32(2) < np.float32(0.01)), "the 0.1 / 0.1 / 0.01 case must be 'diff' (strict <)"


def test_unsorted_queue_case_overflows_the_sorted_queue_key():
    (label, (target, scans, off, _, _, k, thr)), = kc.cases("unsorted_queue")
    cell, n, _ = kc.grid_frame(target, k, thr)
    assert cell == math.sqrt(k * thr) * 1.001 and min(n) > 190_000
    key_bits, idx_bits = math.ceil(math.log2(n[0] * n[1] * n[2])), math.ceil(math.log2(len(scans)))
    assert key_bits + idx_bits > 64, (key_bits, idx_bits)
    assert kc.queue_bits(target, k, thr, len(scans)) == (key_bits, idx_bits) == (53, 12)
    assert len(off) - 1 == 3 and len(target) > 64


def test_clamped_cell_case_takes_the_clamp():
    (label, (target, scans, off, _, _, k, thr)), = kc.cases("clamped_cell")
    ext = float((target[:, :3].max(0).astype(np.float64) - target[:, :3].min(0).astype(np.float64)).max())
    assert ext / 1e6 > math.sqrt(k * thr) * 1.001
    cell, n, _ = kc.grid_frame(target, k, thr)
    assert cell == ext / 1e6 and max(n) < 2 ** 20 and max(n) > 999_000
    kb, ib = kc.queue_bits(target, k, thr, len(scans))
    assert kb == 60 and kb + ib > 64


def test_every_other_case_fits_the_sorted_queue():
    for name in sorted(kc.BUILDERS):
        if name in ("unsorted_queue", "clamped_cell"):
            continue
        for label, (target, scans, off, _, _, k, thr) in kc.cases(name):
            if len(target) > 64 and len(scans):
                kb, ib = kc.queue_bits(target, k, thr, len(scans))
                assert kb + ib <= 64, label


def _cell_counts(target, k, thr):
    cell, n, origin = kc.grid_frame(target, k, thr)
    c = kc.cells_of(target, cell, origin)
    # the box's maximum lies in cell n-2; its minimum lies one cell edge above the origin, i.e. in cell 1 or -- where the product with the
    # reciprocal rounds down -- at the very top of cell 0
    assert (c >= 0).all() and (c <= np.array(n) - 2).all(), "target points occupy cells 0 .. n-2"
    _, counts = np.unique(c, axis=0, return_counts=True)
    return counts


def test_crowded_and_thin_case_has_cells_above_nine_and_below_k():
    for label, (target, _, _, _, _, k, thr) in kc.cases("crowded_and_thin_cells"):
        counts = _cell_counts(target, k, thr)
        assert (counts > 9).any() and (counts >= 100).any(), label          # more than a bucket's nine: the evenly-spread sample
        assert (counts < k).any(), label
        assert len(np.unique(target[:, :3], axis=0)) < len(target), f"{label}: no duplicated target points"


def test_bucketless_case_has_one_site_per_cell():
    (label, (target, scans, _, _, _, k, thr)), = kc.cases("bucketless")
    counts = _cell_counts(target, k, thr)
    assert len(counts) == 8192 == len(scans) and (counts == 2).all()
    s = np.unique(target[:, :3].astype(np.float64), axis=0)
    from scipy.spatial import cKDTree
    d, _ = cKDTree(s).query(s, 2)
    assert d[:, 1].min() >= 1.0


def test_straddle_case_reaches_all_26_neighbour_cells_the_rim_and_the_outside(orc):
    for index, (label, (target, scans, off, poses, inv, k, thr)) in enumerate(kc.cases("straddle")):
        cell, n, origin = kc.grid_frame(target, k, thr)
        assert abs(cell - 0.25 * 1.001) < 1e-6
        flags, _ = kc.expected("straddle", index)
        qc = kc.cells_of(scans, cell, origin)          # identity poses: scan point == global point
        # the neighbour that decides a coexist query lies within sqrt(k thr) of it: find the cell of the farthest of its k nearest
        t64 = target[:, :3].astype(np.float64)
        tc = kc.cells_of(target, cell, origin)
        from scipy.spatial import cKDTree
        _, nn = cKDTree(t64).query(scans[:, :3].astype(np.float64), k)
        kth = nn if k == 1 else nn[:, k - 1]
        offs = {tuple(o) for o in (tc[kth] - qc)[flags == 1]}
        assert {tuple(int(v) for v in d) for d in kc.DIRS26} <= offs, f"{label}: neighbour cells never decisive: {sorted(set(map(tuple, kc.DIRS26.astype(int))) - offs)}"
        if k == 1:
            nn_arr = np.array(n)
            rim = ((qc == 0) | (qc == nn_arr - 1)).any(axis=1) & (qc >= 0).all(axis=1) & (qc < nn_arr).all(axis=1)
            outside = ((qc < 0) | (qc >= nn_arr)).any(axis=1)
            assert rim.sum() >= 20 and outside.sum() >= 20, (int(rim.sum()), int(outside.sum()))
            assert (flags[rim] == 1).any(), "no coexist query in a rim cell"
            assert (flags[outside] == 0).all()


def test_far_and_outside_case_leaves_the_grid(orc):
    (label, (target, scans, off, poses, inv, k, thr)), _ = kc.cases("far_and_outside")
    cell, n, origin = kc.grid_frame(target, k, thr)
    qc = kc.cells_of(kc.global_points(kc.cases("far_and_outside")[0][1]), cell, origin)
    nn = np.array(n)
    out = ((qc < -1) | (qc > nn)).any(axis=1)
    a, b, c = [slice(int(off[j]), int(off[j + 1])) for j in range(3)]
    assert not out[a].any() and 0.2 < out[b].mean() < 0.8 and out[c].all()
    flags, _ = kc.expected("far_and_outside", 0)
    assert flags[a].mean() > 0.1 and flags[c].sum() == 0
    t2 = kc.cases("far_and_outside")[1][1][0]
    assert np.abs(t2[:, :2]).min() > 9.9e4 and np.spacing(np.float32(1e5)) > 0.0078


def test_small_targets_cover_the_brute_force_boundary():
    labels = [label for label, _ in kc.cases("small_targets")]
    assert len(labels) == len(kc.SMALL_MT) * len(kc.SMALL_K) == 54
    for label, (target, scans, *_rest) in kc.cases("small_targets"):
        assert len(scans) == 500 and f"Mt{len(target)}-" in label


def test_ragged_and_many_keyframes_shapes():
    (_, (target, scans, off, poses, _, _, _)), = kc.cases("ragged_ranges")
    assert list(np.diff(off.astype(np.int64))) == kc.RAGGED_SIZES
    for _, (target, scans, off, poses, inv, k, thr) in kc.cases("many_keyframes"):
        sizes = np.diff(off.astype(np.int64))
        assert len(sizes) == 65537 + 300 and set(np.unique(sizes)) == {0, 1, 2}
        assert sizes[65535:].sum() > 100, "keyframes of the second launch must hold points"
        assert len(np.unique(poses[:, [3, 7, 11]], axis=0)) > 65000


def test_nonfinite_case_marks_rows_the_oracle_calls_diff(orc):
    for index, (label, case) in enumerate(kc.cases("nonfinite_queries")):
        g = kc.global_points(case)
        bad = ~np.isfinite(g[:, :3]).all(axis=1)
        raw = case[1]
        spoilt = (~np.isfinite(raw[:, :3]) | (raw[:, :3] == np.float32(3e38))).any(axis=1)
        assert spoilt.sum() == 48 and not spoilt[600:].any() and not bad[~spoilt].any(), label
        assert 36 <= bad.sum() <= 48, label                 # a 3e38 may stay finite through the pose; its squared distance does not
        flags, _ = kc.expected("nonfinite_queries", index)
        assert (flags[spoilt] == 0).all(), label
        assert np.isnan(raw[:, :3]).any() and np.isposinf(raw[:, :3]).any() and np.isneginf(raw[:, :3]).any() and (raw[:, :3] == np.float32(3e38)).any()
