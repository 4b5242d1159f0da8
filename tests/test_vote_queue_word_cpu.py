"""The survivor queue word of the range-culled vote kernel carries a pixel as a linear index in 18 bits (ltm_kernels_common.h: tile in run 4 bits | group 4 |
lane 6 | pixel 18, all ones = pixel not certain).  The drain takes row and column back out of it with a multiply-high by a host-made constant, and only
shapes whose pixels fit the field take the fast path.  Read through ltm_debug_vote_queue_word: the quotient must be numpy's integer division for every
pixel of the shapes the vote runs at and of the shapes on either side of the field's limit, and the predicate must be rows * cols <= 2^18 - 1.
No device needed."""
import numpy as np
import pytest

HFOV = 360.0
PX_BITS = 18
NPX_LIMIT = (1 << PX_BITS) - 1          # the largest pixel index, npx - 1, must stay below the all-ones value
# With vfov 50 and hfov 360: rows = round(50 alpha), cols = round(360 alpha).  262143 / 191 = 1372.47, so 191 x 1372 = 262052 is the largest image of this
# field of view that fits (190 rows end at alpha < 3.81, i.e. at 190 x 1372 = 260680) and 191 x 1373 = 262243 is the first that does not.
ALPHA_FITS = float(np.float32(1372.0 / 360.0))
ALPHA_TOO_LARGE = float(np.float32(1373.0 / 360.0))
# (vfov, alpha, rows, cols, on the fast path)
SHAPES = [
    (50.0, 2.5, 125, 900, True), (50.0, 2.0, 100, 720, True), (50.0, 1.5, 75, 540, True),           # the three resolutions of the vote
    (50.0, float(np.float32(0.95 * 2.5)), 119, 855, True), (50.0, 3.0, 150, 1080, True),           # an odd shape; the reprojection's resolution
    (90.0, 2.5, 225, 900, True), (90.0, 1.5, 135, 540, True),                                       # no steep-elevation clamp
    (50.0, ALPHA_FITS, 191, 1372, True), (50.0, ALPHA_TOO_LARGE, 191, 1373, False),                 # either side of the field's limit
    (50.0, 6.0, 300, 2160, False), (90.0, 3.0, 270, 1080, False),
]


@pytest.mark.parametrize("vfov,alpha,rows,cols,fast", SHAPES)
def test_row_and_column_of_every_pixel(ltm, vfov, alpha, rows, cols, fast):
    npx = rows * cols
    px = np.arange(npx, dtype=np.uint32)
    u, row, col = ltm.vote_queue_word(vfov, HFOV, alpha, px)
    assert (u["rows"], u["cols"], u["npx"]) == (rows, cols, npx)
    assert u["px_bits"] == PX_BITS and u["npx_limit"] == NPX_LIMIT
    assert bool(u["fast_path"]) == fast == (npx <= NPX_LIMIT)
    assert (row == px // cols).all() and (col == px % cols).all(), f"{rows} x {cols}: {(row != px // cols).sum()} rows differ from integer division"
    # the constant is made as the run mapping's: floor(2^(26 + s) / cols) + 1 with 2^s >= cols > 2^(s - 1)
    s = u["px_shift"]
    assert (1 << s) >= cols and (s == 0 or (1 << (s - 1)) < cols)
    assert u["px_magic"] == (1 << (26 + s)) // cols + 1


def test_the_limit_is_where_the_arithmetic_says(ltm):
    fits, _, _ = ltm.vote_queue_word(50.0, HFOV, ALPHA_FITS)
    over, _, _ = ltm.vote_queue_word(50.0, HFOV, ALPHA_TOO_LARGE)
    assert fits["npx"] == 262052 <= NPX_LIMIT < 262243 == over["npx"]
    assert fits["fast_path"] == 1 and over["fast_path"] == 0
    assert fits["npx"] - 1 < NPX_LIMIT, "the all-ones pixel value stays free for 'not certain'"
    # no shape of this field of view between the two: the next smaller image has 190 rows
    for a in np.linspace(3.78, 3.85, 700):
        u, _, _ = ltm.vote_queue_word(50.0, HFOV, float(np.float32(a)))
        assert bool(u["fast_path"]) == (u["npx"] <= NPX_LIMIT)
        assert u["npx"] <= fits["npx"] or u["npx"] >= over["npx"]


@pytest.mark.parametrize("cols", [4, 63, 64, 65, 540, 900, 1372, 1373, 2048, 2049, 4097])
def test_quotient_is_exact_over_the_whole_pixel_field(ltm, cols):
    """every value the 18-bit field can hold, and the rest of the quotient's domain (px < 2^26) at random, for divisors an image never has too"""
    alpha = float(np.float32(cols / 360.0))
    u, _, _ = ltm.vote_queue_word(50.0, HFOV, alpha)
    assert u["cols"] == cols, "the construction of alpha"
    rng = np.random.default_rng(cols)
    px = np.concatenate([np.arange(1 << PX_BITS, dtype=np.uint32), rng.integers(0, 1 << 26, 1 << 16).astype(np.uint32),
                         np.array([(1 << 26) - 1, (1 << 26) - cols, ((1 << 26) // cols) * cols - 1], dtype=np.uint32)])
    _, row, col = ltm.vote_queue_word(50.0, HFOV, alpha, px)
    assert (row == px // cols).all() and (col == px % cols).all()


def test_arguments_are_checked(ltm):
    with pytest.raises(ltm.LtmError):
        ltm.vote_queue_word(50.0, HFOV, 0.0)
    with pytest.raises(ltm.LtmError):
        ltm.vote_queue_word(50.0, HFOV, 2.5, np.array([1 << 26], dtype=np.uint32))
