"""The argument behind ltm_reproject_twin, restated in numpy; no GPU.

A map image holds per pixel the minimum of the words (range bits << 32 | point index) of the map's points.  Map A = S + A_only, where S are the points
that a second map B holds too, bit for bit.  Both maps list their points in the octree order of one frame, so the index of a shared point in A and its
index in B both increase with its index in S.  Then image(A) = min(relabel(image(S), S -> A), image(A_only)): the winner among the shared points of a pixel
-- ties on equal range bits included -- is the same point whichever of the three index sets the words carry.  The second test is the premise: what the
join calls shared (equal bits) pairs up in order on clouds gridded by the CPU oracle's voxel grid."""
import numpy as np

EMPTY = np.uint64(0x461C4000) << np.uint64(32)      # kFlagNoPOINT = 10000.0f, index 0: the fill word of an image


def _image(px, rng_bits, idx, npx):
    """min over the points of (range bits << 32 | index) per pixel, the empty word where no point falls"""
    img = np.full(npx, EMPTY, np.uint64)
    np.minimum.at(img, px, (rng_bits.astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64))
    return img


def _relabel(img, table):
    out = img.copy()
    hit = img != EMPTY
    out[hit] = (img[hit] & np.uint64(0xFFFFFFFF00000000)) | table[(img[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)].astype(np.uint64)
    return out


def test_relabel_then_min_equals_direct_min():
    rng = np.random.default_rng(7)
    npx = 300
    for trial in range(40):
        n_a, n_b = int(rng.integers(1, 900)), int(rng.integers(1, 900))
        n_s = int(rng.integers(0, min(n_a, n_b) + 1))
        s2a, s2b = np.sort(rng.choice(n_a, n_s, replace=False)), np.sort(rng.choice(n_b, n_s, replace=False))      # increasing, like octree order
        # few distinct ranges (among them the empty range itself) and few pixels: ties between shared points, between only-points, and across
        ranges = np.array([0x41200000, 0x41200001, 0x41A00000, 0x461C4000, 0x47000000], np.uint32)
        px = {m: rng.integers(0, npx, n) for m, n in (("a", n_a), ("b", n_b))}
        rb = {m: ranges[rng.integers(0, len(ranges), n)] for m, n in (("a", n_a), ("b", n_b))}
        px["b"][s2b], rb["b"][s2b] = px["a"][s2a], rb["a"][s2a]      # a shared point is ONE point: same pixel and range in both maps
        img_s = _image(px["a"][s2a], rb["a"][s2a], np.arange(n_s), npx)
        for m, n, table in (("a", n_a, s2a), ("b", n_b, s2b)):
            only = np.setdiff1d(np.arange(n), table)
            direct = _image(px[m], rb[m], np.arange(n), npx)
            twin = np.minimum(_relabel(img_s, table), _image(px[m][only], rb[m][only], only, npx))
            assert (twin == direct).all(), f"trial {trial}, map {m}: {np.count_nonzero(twin != direct)} pixels differ"


def test_relabel_needs_increasing_tables():
    """the counter-example that the order check of the join is there for: two shared points tie, and a table that swaps them changes the winner"""
    px, rb = np.array([0, 0]), np.array([0x41200000, 0x41200000], np.uint32)
    img_s = _image(px, rb, np.arange(2), 1)
    swapped = np.array([5, 3])
    direct = _image(px, rb, swapped, 1)
    assert _relabel(img_s, swapped)[0] != direct[0]
    assert _relabel(img_s, np.array([3, 5]))[0] == _image(px, rb, np.array([3, 5]), 1)[0]


def test_shared_points_of_two_grids_pair_up_in_order(orc):
    rng = np.random.default_rng(3)
    corners = np.array([[-30, -30, -5, 0], [30, 30, 5, 0]], np.float32)      # both clouds' bounding box, so both grids use one octree frame
    U = np.concatenate([corners, np.c_[rng.uniform(-25, 25, (6000, 2)), rng.uniform(-4, 4, 6000), rng.uniform(0, 100, 6000)].astype(np.float32)])
    P1 = np.c_[rng.uniform(-25, 25, (300, 2)), rng.uniform(-4, 4, 300), rng.uniform(0, 100, 300)].astype(np.float32)
    P1[:40, :3] = U[100:140, :3] + np.float32(0.004)      # some fall into voxels of U: those centroids move in the map that holds them
    A, B = orc.voxel_centroid(np.concatenate([U, P1]), 0.05), orc.voxel_centroid(np.concatenate([U, P1[::2]]), 0.05)
    key_b = {r.tobytes(): j for j, r in enumerate(B)}
    assert len(key_b) == len(B)      # one point per voxel: no two equal
    s2a = np.array([i for i, r in enumerate(A) if r.tobytes() in key_b])
    s2b = np.array([key_b[A[i].tobytes()] for i in s2a])
    assert 0.9 * len(A) < len(s2a) < min(len(A), len(B))
    assert (np.diff(s2a) > 0).all() and (np.diff(s2b) > 0).all(), "a shared point's indices in A and in B do not both increase along S"
    # -0.0 and +0.0 are different points for the join, as for the bitwise tests of the outputs
    assert np.float32(-0.0).tobytes() != np.float32(0.0).tobytes()
