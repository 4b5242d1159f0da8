"""The band plan of the LDS scan-image kernel (ltm_debug_scan_bands; make_scan_bands in ltm_k_projection.hip): for every shape the bands are disjoint,
ordered and cover rows 0 .. rows - 1, a band's bytes fit the budget, and shape sets that cannot be served are reported as such.  No GPU."""
import numpy as np
import pytest

MAX_SHAPES = 8          # kMaxScanShapes
LOT = ([125, 119, 100, 95, 75, 71], [900, 855, 720, 684, 540, 513])


def _check_plan(ltm, rows, cols):
    nb, row0, nbytes, budget = ltm.scan_bands(rows, cols)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if nb == 0:
        return 0, budget
    assert row0.shape == (nb + 1, len(rows)) and nbytes.shape == (nb,)
    r0 = row0.astype(np.int64)
    assert (r0[0] == 0).all() and (r0[nb] == rows).all(), "the bands of a shape start at row 0 and end at its last row"
    assert (np.diff(r0, axis=0) >= 0).all(), "ordered, disjoint (band b ends where band b + 1 starts)"
    px = (np.diff(r0, axis=0) * cols[None, :]).sum(axis=1) * 4
    assert (nbytes.astype(np.int64) >= px).all(), "a band's bytes hold its pixels"
    assert (nbytes <= budget).all(), "a band's bytes fit the budget"
    return nb, budget


def test_lot_shapes(ltm):
    nb, budget = _check_plan(ltm, *LOT)
    assert 0 < budget <= 160 * 1024
    total = sum(r * c * 4 for r, c in zip(*LOT))
    assert nb >= -(-total // budget), "fewer bands cannot hold the images"
    assert nb <= 2 * -(-total // budget), "and the plan is not far from that many"


def test_one_by_one_and_single_band(ltm):
    assert _check_plan(ltm, [1], [1])[0] == 1
    assert _check_plan(ltm, [25], [180])[0] == 1                      # 18 KB: one band
    assert _check_plan(ltm, [1, 71], [1, 513])[0] >= 1
    nb, _ = _check_plan(ltm, [125], [900])                            # 450 KB
    assert nb >= 3
    assert _check_plan(ltm, [1] * MAX_SHAPES, [1] * MAX_SHAPES)[0] == 1


def test_random_shape_sets(ltm):
    rng = np.random.default_rng(20250)
    served = 0
    for _ in range(300):
        n = int(rng.integers(1, MAX_SHAPES + 1))
        rows = rng.integers(1, 401, n)
        cols = rng.integers(1, 9001, n) if rng.random() < 0.5 else rng.integers(1, 1200, n)
        nb, budget = _check_plan(ltm, rows, cols)
        one_row_each = int(((cols + 3 + 3) // 4 * 4 * 4).sum())       # band 0 of a plan with as many bands as rows: one row of every shape
        if nb == 0:
            assert one_row_each > budget or int(rows.max()) > 4096, f"rows {rows} cols {cols}: a plan exists"
        else:
            served += 1
    assert served > 100


def test_unservable_sets(ltm):
    _, _, _, budget = ltm.scan_bands([1], [1])
    wide = budget // 4 + 1
    assert ltm.scan_bands([3], [wide])[0] == 0, "one row wider than the budget"
    assert ltm.scan_bands([3, 5], [wide // 2, wide // 2 + 8])[0] == 0, "one row of all shapes together wider than the budget"
    assert ltm.scan_bands([2] * (MAX_SHAPES + 1), [2] * (MAX_SHAPES + 1))[0] == 0, "more shapes than a launch takes"
    assert ltm.scan_bands([0], [10])[0] == 0 and ltm.scan_bands([10], [0])[0] == 0, "a shape without pixels"
    assert ltm.scan_bands([], [])[0] == 0
    assert _check_plan(ltm, [3], [budget // 4 - 3])[0] == 3, "the widest row that fits: one row per band"


@pytest.mark.parametrize("rows,cols", [([400] * 8, [9000] * 8), ([400], [9000]), ([7, 400, 1], [9000, 3, 1])])
def test_edge_sizes(ltm, rows, cols):
    _check_plan(ltm, rows, cols)
