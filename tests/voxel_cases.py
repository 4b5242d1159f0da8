"""TEST INFRASTRUCTURE: seeded edge cases of the voxel-centroid grid (ltm_voxel_centroid and its _batch / _shard / _box / _scanset forms) and a numpy
restatement of that grid.  Plain functions, no fixtures, no GPU.

The restatement (frame_of_box, restate) is written from the comment block above octree_frame_of_box in oracle/ltm_oracle.cpp and calls neither the oracle
nor the library: the frame from the box (float add of 512 FLT_EPSILON, depth, per-axis centring when over > FLT_EPSILON), keys in double, the Morton code
with x as the most significant bit of a triple, a stable order by code, float32 sums left to right in input order divided by float32(count).

Four families, each built to reach what realistic (uniformly random) clouds do not:
  lattice   points exactly on voxel faces and one float below / above them, 0 ... 100 km from the origin, boxes that are planes and lines (two axes centred
            by half the cube), extents around a depth switch, a -0.0 coordinate: the device's key arithmetic (octree_code, ltm_device_prims.h)
  segments  clouds whose sorted head positions are fixed by construction (segments_cloud on a line parallel to z, where Morton order is z order): heads on
            the wave (512) and tile (2048) edges of k_voxel_heads_starts, voxels longer than tiles, more than 64 tiles for its look-back, a long last voxel
            for the `n` bound of the centroid kernels; packed (z line, leaf 0.25) and unpacked (600 m cube, leaf 1 mm: key/index pairs)
  stale     a gridded cloud written in place (rows swapped, duplicated, a -0.0 written): what k_bbox_reduce_check must call a violation, and what it must not
  scanset   keyframes of depth 3 and 15 side by side, the same cloud in consecutive keyframes (equal Morton codes across a keyframe boundary), empty ones

Every builder asserts the property its case is named for, from the restatement's own head positions.  tests/test_voxel_cases_cpu.py shows on the host that the
oracle and the restatement agree bit for bit on every fixture; tests/test_gpu_voxel_edges.py runs them on the device against the oracle."""
import collections
import functools
import math

import numpy as np

F32 = np.float32
FLT_EPS = float(np.finfo(np.float32).eps)
EPS512 = F32(FLT_EPS) * F32(512.0)

Frame = collections.namedtuple("Frame", "lo res depth")                         # lattice origin (3 doubles), leaf as a double, octree depth
Restated = collections.namedtuple("Restated", "centroids frame codes heads")    # codes: sorted; heads: first sorted position of every voxel


def _orc():
    from oracle import oracle_py
    oracle_py.lib()
    return oracle_py


def _capi():
    import ltmapper_amd  # noqa: F401
    from ltmapper_amd import capi
    return capi


def _p4(xyz, rng):
    """(n, 3) float32 -> (n, 4) float32 with a seeded intensity column; the coordinates travel untouched (bit for bit)"""
    xyz = np.asarray(xyz)
    assert xyz.dtype == F32
    out = np.empty((xyz.shape[0], 4), F32)
    out[:, :3] = xyz
    out[:, 3] = rng.uniform(0, 255, xyz.shape[0])
    return out


def _ulps(x, k):
    """the float32 k representable steps above (k > 0) or below (k < 0) x"""
    x = F32(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


# ------------------------------------------------------------------------------------------------- the grid, restated
def frame_of_box(mn, mx, leaf):
    """the octree frame of a bounding box: defineBoundingBox + getKeyBitSize on an empty tree"""
    mn, mx = np.asarray(mn, dtype=F32), np.asarray(mx, dtype=F32)
    lo = mn.astype(np.float64)
    hi = (mx + EPS512).astype(F32).astype(np.float64)            # the add is a float add
    res = float(F32(leaf))
    cells = [math.ceil((hi[d] - lo[d] - FLT_EPS) / res) for d in range(3)]
    assert min(cells) >= 0
    depth = min(32, math.ceil(math.log2(max(max(cells), 2)) - FLT_EPS))
    side = float(1 << depth) * res
    for d in range(3):
        over = (side - (hi[d] - lo[d])) / 2.0
        if over > FLT_EPS:
            lo[d] -= over
    return Frame(lo, res, depth)


def frame_of(pts, leaf):
    p = np.asarray(pts, dtype=F32).reshape(-1, 4)
    return frame_of_box(p[:, :3].min(0), p[:, :3].max(0), leaf)


def same_frame(a, b):
    return bool((a.lo == b.lo).all()) and a.res == b.res and a.depth == b.depth


def keys_of(pts, frame):
    """(n, 3) integer keys, (unsigned)(((double)p - min) / res); every key must lie inside the cube (the grid's contract: finite points inside the box)"""
    p = np.asarray(pts, dtype=F32).reshape(-1, 4)
    q = (p[:, :3].astype(np.float64) - frame.lo) / frame.res
    assert (q >= 0).all() and (q < float(1 << frame.depth)).all(), "a key outside [0, 2^depth)"
    return q.astype(np.int64)


def morton(keys, depth):
    """x is the most significant bit of every level's triple"""
    k = np.asarray(keys).astype(np.uint64)
    code = np.zeros(len(k), np.uint64)
    for b in range(depth - 1, -1, -1):
        sh = np.uint64(b)
        one = np.uint64(1)
        code = (code << np.uint64(3)) | (((k[:, 0] >> sh) & one) << np.uint64(2)) | (((k[:, 1] >> sh) & one) << one) | ((k[:, 2] >> sh) & one)
    return code


def restate(pts, leaf, box=None):
    """the voxel centroids of `pts` (under the frame of `box` = (mn, mx) if given, of the cloud's own box otherwise)"""
    p = np.ascontiguousarray(pts, dtype=F32).reshape(-1, 4)
    assert len(p) and np.isfinite(p).all()
    frame = frame_of(p, leaf) if box is None else frame_of_box(box[0], box[1], leaf)
    code = morton(keys_of(p, frame), frame.depth)
    order = np.argsort(code, kind="stable")                       # input order inside a voxel
    sc, sp = code[order], p[order]
    heads = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
    counts = np.diff(np.r_[heads, len(p)])
    sums = np.zeros((len(heads), 4), F32)                         # 0 + x0 + x1 + ...: float32, left to right (cumsum accumulates sequentially)
    for v in np.flatnonzero(counts > 32):
        sums[v] = np.cumsum(np.vstack([np.zeros((1, 4), F32), sp[heads[v]:heads[v] + counts[v]]]), axis=0, dtype=F32)[-1]
    short = counts <= 32
    for r in range(32):
        sel = short & (counts > r)
        if not sel.any():
            break
        sums[sel] = sums[sel] + sp[heads[sel] + r]
    cent = sums / counts.astype(F32)[:, None]
    assert cent.dtype == F32
    return Restated(cent, frame, sc, heads)


@functools.lru_cache(maxsize=None)
def _oracle_cached(key):
    kind, name, index = key
    pts, leaf = cloud_of(kind, name, index)
    out = _orc().voxel_centroid(pts, leaf)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------- the builder
def segments_cloud(anchors, voxels, counts, rng, leaf, spread=(0.15, 0.85)):
    """The two anchor points (box corners, part of the cloud) fix the bounding box and so the frame; counts[j] further points go inside voxel voxels[j]
    of that frame, at frame_min + (k + u) * res with u well inside the part of the voxel that lies strictly inside the anchors' box (an axis on which
    the box has no extent takes the anchors' coordinate).  Input order is shuffled.  Asserted: every point has the key it was meant to have, lies
    strictly inside the box, and the finished cloud's frame is the anchors' frame."""
    a = np.asarray(anchors, dtype=F32).reshape(2, 3)
    assert (a[0] <= a[1]).all()
    frame = frame_of_box(a[0], a[1], leaf)
    vox = np.asarray(voxels, dtype=np.int64).reshape(-1, 3)
    counts = np.asarray(counts, dtype=np.int64)
    assert len(vox) == len(counts) and (counts >= 0).all()
    k = np.repeat(vox, counts, axis=0)
    n = len(k)
    xyz = np.empty((n, 3), F32)
    a64 = a.astype(np.float64)
    for d in range(3):
        if a[0, d] == a[1, d]:
            xyz[:, d] = a[0, d]
            continue
        lo = np.maximum(frame.lo[d] + k[:, d] * frame.res, a64[0, d])
        hi = np.minimum(frame.lo[d] + (k[:, d] + 1) * frame.res, a64[1, d])
        assert (hi - lo > 0.25 * frame.res).all(), "a voxel with too little room inside the box"
        u = rng.uniform(spread[0], spread[1], n)                 # well inside: float rounding (far below 0.15 of the room) cannot move the point out
        xyz[:, d] = (lo + u * (hi - lo)).astype(F32)
        assert ((xyz[:, d] > a[0, d]) & (xyz[:, d] < a[1, d])).all(), "a point not strictly inside the anchors' box"
    pts = np.concatenate([a, xyz])
    pts = _p4(pts[rng.permutation(len(pts))], rng)
    assert same_frame(frame_of(pts, leaf), frame)
    got = keys_of(np.c_[xyz, np.zeros(n, F32)], frame)
    assert (got == k).all(), "a point outside the voxel it was placed in"
    return pts, frame


# ------------------------------------------------------------------------------------------------- lattice edges
LEAVES = (0.05, 0.1, 0.4, 0.25, 1.0)                      # the first three are not representable
CENTRES = (0.0, -123.456, 1.0e4, -1.0e5)
EXTENTS = ((6.3, 6.3, 6.3), (12.8, 0.0, 0.0), (25.6, 25.6, 0.0), (3.17, 40.0, 1.0))
SWITCH_DEPTHS = (1, 4, 10)
LATTICE_FORMS_EXTENT = 3                                  # the cloud per leaf that also goes through batch, shards and box: centre -123.456, extent (3.17, 40, 1)


def _face_cloud(mn, mx, leaf, n_faces, rng, neg_zero=False):
    """both box corners; points whose coordinates are voxel faces float32(frame_min + k res) of the box's own frame; each one's neighbour one float down
    and one float up on all axes, and one with a direction of its own per axis; everything clipped into the box"""
    mn, mx = np.asarray(mn, dtype=F32), np.asarray(mx, dtype=F32)
    f = frame_of_box(mn, mx, leaf)
    corners = np.stack([mn, mx])
    klo, khi = keys_of(np.c_[corners, np.zeros(2, F32)], f)
    k = np.stack([rng.integers(klo[d], khi[d] + 2, n_faces) for d in range(3)], axis=1)
    face = (f.lo + k * f.res).astype(F32)
    down, up = np.nextafter(face, F32(-np.inf)), np.nextafter(face, F32(np.inf))
    pick = rng.integers(0, 3, face.shape)
    mixed = np.where(pick == 0, down, np.where(pick == 1, face, up))
    xyz = np.clip(np.concatenate([face, down, up, mixed]), mn, mx).astype(F32)
    if neg_zero:
        assert mn[0] < 0 < mx[0]
        extra = xyz[:2].copy()
        extra[0, 0], extra[1, 0] = F32(-0.0), F32(0.0)        # -0.0 and +0.0 share a key; a voxel that sums only -0.0 still gives +0.0
        xyz = np.concatenate([xyz, extra])
    pts = _p4(np.concatenate([corners, xyz[rng.permutation(len(xyz))]]), rng)
    assert same_frame(frame_of(pts, leaf), f) and len(pts) <= 2100
    return pts


def _depth_of_top(e, top, leaf):
    return frame_of_box(np.array([F32(-0.5) * e, 0, 0], F32), np.array([top, 0, 0], F32), leaf).depth


def _switch_top(d, e, leaf):
    """the largest float32 `top` for which the box x = [-e / 2, top] still has octree depth d: the next float's has depth d + 1.  (Such a box from 0 would put
    its far corner on the cube's closed upper face where the 512 FLT_EPSILON are lost to rounding, at 1024 m and beyond -- key 2^depth, outside the
    grid's contract: PCL itself grows the tree there.)"""
    a, b = F32(0.4) * e, F32(0.51) * e
    assert _depth_of_top(e, a, leaf) == d and _depth_of_top(e, b, leaf) == d + 1
    ia, ib = int(a.view(np.int32)), int(b.view(np.int32))
    while ib - ia > 1:
        m = (ia + ib) // 2
        if _depth_of_top(e, np.int32(m).view(F32), leaf) > d:
            ib = m
        else:
            ia = m
    return np.int32(ia).view(F32)


@functools.lru_cache(maxsize=None)
def lattice_cases(leaf):
    """[(label, points)] of one leaf: 16 centre x extent clouds, and for d in SWITCH_DEPTHS the boxes whose longest extent is 2^d leaf minus one float,
    exactly, plus one float (x from -E/2 to E/2: both ends and their difference are exact), and the two consecutive floats between which the depth
    really switches from d to d + 1"""
    out = []
    li = LEAVES.index(leaf)
    for ci, c in enumerate(CENTRES):
        for ei, ext in enumerate(EXTENTS):
            rng = np.random.default_rng(10_000 + 100 * li + 10 * ci + ei)
            h = np.asarray(ext, dtype=np.float64) / 2
            mn, mx = (c - h).astype(F32), (c + h).astype(F32)
            out.append((f"leaf{leaf}-centre{c:g}-extent{ei}", _face_cloud(mn, mx, leaf, 500, rng, neg_zero=(c == 0.0))))
    for d in SWITCH_DEPTHS:
        rng = np.random.default_rng(20_000 + 100 * li + d)
        e = F32(2 ** d) * F32(leaf)
        assert float(e) == 2 ** d * float(F32(leaf))
        for tag, top in (("minus", _ulps(F32(0.5) * e, -1)), ("exact", F32(0.5) * e), ("plus", _ulps(F32(0.5) * e, 1))):
            mn = np.array([F32(-0.5) * e, 0, 0], F32)
            mx = np.array([top, F32(0.37) * e, 0], F32)
            if tag == "exact":
                assert float(mx[0]) - float(mn[0]) == float(e)
            out.append((f"leaf{leaf}-switch{d}-{tag}", _face_cloud(mn, mx, leaf, 150, rng)))
        last = _switch_top(d, e, leaf)
        for tag, top, depth in (("last", last, d), ("first", _ulps(last, 1), d + 1)):
            pts = _face_cloud(np.array([F32(-0.5) * e, 0, 0], F32), np.array([top, F32(0.37) * e, 0], F32), leaf, 150, rng)
            assert frame_of(pts, leaf).depth == depth, f"leaf {leaf}: the depth does not switch between the two floats"
            out.append((f"leaf{leaf}-depth{depth}-{tag}-float", pts))
    assert len(out) == 16 + 5 * len(SWITCH_DEPTHS)
    return out


def lattice_forms_case(leaf):
    """the one cloud per leaf that also runs through the batch, shard and box forms"""
    return lattice_cases(leaf)[1 * len(EXTENTS) + LATTICE_FORMS_EXTENT]


# ------------------------------------------------------------------------------------------------- segment edges (packed: a line parallel to z)
SEG_LEAF = 0.25
WAVE, TILE = 512, 2048                                    # k_voxel_heads_starts: keys per wave, keys per tile (256 threads x 8)
TILE_EDGE_N = (2047, 2048, 2049, 4097)
TILE_EDGE_HEADS = (2047, 2048, 2049, 4096)


def z_line(counts, rng, depth=None, x=1.5, y=-2.25):
    """a cloud on a line parallel to z whose sorted segments hold counts[0], counts[1], ... points: the first segment is the low anchor's voxel (key 0),
    the last the high anchor's (key 2^depth - 1), the others seeded voxels between them in z order.  Morton order on the line is z order, so the head
    positions are the running sums of `counts` (asserted from the restatement)."""
    counts = list(counts)
    m = len(counts)
    assert m >= 2 and min(counts) >= 1
    d = max(math.ceil(math.log2(m)), 1) if depth is None else depth
    top = (1 << d) - 1
    assert m <= top + 1
    half = ((1 << d) * SEG_LEAF - 0.3) / 2                  # 0.15 m of the cube left over at either end: the anchors sit 0.6 / 0.4 of the way through their voxels
    anchors = np.array([[x, y, -half], [x, y, half]], F32)
    frame = frame_of_box(anchors[0], anchors[1], SEG_LEAF)
    assert frame.depth == d
    kxy = keys_of(np.c_[anchors[:1], np.zeros(1, F32)], frame)[0, :2]
    kz = np.r_[0, np.sort(rng.permutation(np.arange(1, top))[:m - 2]), top]
    vox = np.c_[np.tile(kxy, (m, 1)), kz]
    extra = np.array(counts)
    extra[0] -= 1
    extra[-1] -= 1                                           # the anchors are points of the first and the last segment
    pts, _ = segments_cloud(anchors, vox, extra, rng, SEG_LEAF)
    r = restate(pts, SEG_LEAF)
    assert same_frame(r.frame, frame) and len(pts) == sum(counts)
    assert (r.heads == np.r_[0, np.cumsum(counts)[:-1]]).all(), "head positions are not the running sums of the counts"
    return pts, r


def _has_heads(r, at):
    return all(int(h) in set(r.heads.tolist()) for h in at)


def _no_head_in(r, a, b):
    """no head at sorted positions [a, b)"""
    return not ((r.heads >= a) & (r.heads < b)).any()


def _seg_wave_edge(rng):
    pts, r = z_line([511, 1, 1, 511, 300], rng)
    assert _has_heads(r, (511, 512, 513, 1024)) and len(pts) == 1324
    return [("wave_edge", pts)]


def _tile_edge_counts(n):
    """heads at every one of 2047, 2048, 2049, 4096 that the cloud is long enough for; the last voxel is one point (a head at n - 1)"""
    return {2047: [2046, 1], 2048: [2047, 1], 2049: [2047, 1, 1], 4097: [2047, 1, 1, 2047, 1]}[n]


def _seg_tile_edge(rng):
    out = []
    for n in TILE_EDGE_N:
        pts, r = z_line(_tile_edge_counts(n), rng)
        assert len(pts) == n and _has_heads(r, [h for h in TILE_EDGE_HEADS if h < n] + [n - 1])
        out.append((f"tile_edge-n{n}", pts))
    return out


def _seg_straddle(rng):
    pts, r = z_line([1500, 1101, 3600, 6200, 1], rng)
    assert r.heads.tolist() == [0, 1500, 2601, 6201, 12401]
    assert _no_head_in(r, 1501, 2601) and _no_head_in(r, 2602, 6201)           # one voxel over positions 1500 ... 2600 (across 2048), one over 2601 ... 6200
    assert _no_head_in(r, 2 * TILE, 3 * TILE) and _no_head_in(r, 4 * TILE, 6 * TILE)      # whole tiles without a head: one, then two in a row
    return [("straddle", pts)]


def _seg_one_voxel_3_tiles(rng):
    pts, r = z_line([1, 4097, 1], rng)
    assert r.heads.tolist() == [0, 1, 4098] and 4097 > 2 * TILE
    return [("one_voxel_3_tiles", pts)]


def _seg_all_single_2049(rng):
    pts, r = z_line([1] * 2049, rng)
    assert len(pts) == 2049 and (r.heads == np.arange(2049)).all()
    return [("all_single_2049", pts)]


def _seg_long_last(rng):
    pts, r = z_line([1, 5, 40, 3000], rng)
    assert len(pts) - int(r.heads[-1]) == 3000
    return [("long_last", pts)]


def _seg_lookback_sparse(rng):
    pts, r = z_line([28000] * 5, rng)
    tiles = -(-len(pts) // TILE)
    headless = sum(_no_head_in(r, t * TILE, (t + 1) * TILE) for t in range(tiles))
    assert len(pts) == 140_000 and tiles > 64 and headless == tiles - 5
    return [("lookback_sparse", pts)]


def _seg_lookback_dense(rng):
    pts, r = z_line([1] * 140_000, rng, depth=18)
    assert r.frame.depth == 18 and (r.heads == np.arange(140_000)).all()
    z = np.abs(pts[:, 2]).max()
    assert 30_000 < z < 35_000 and float(np.spacing(F32(z))) < SEG_LEAF / 50       # float spacing at the far end stays far below the leaf
    return [("lookback_dense", pts)]


SEGMENT_BUILDERS = {"wave_edge": _seg_wave_edge, "tile_edge": _seg_tile_edge, "straddle": _seg_straddle, "one_voxel_3_tiles": _seg_one_voxel_3_tiles,
                    "all_single_2049": _seg_all_single_2049, "long_last": _seg_long_last, "lookback_sparse": _seg_lookback_sparse,
                    "lookback_dense": _seg_lookback_dense}
LOOKBACK = ("lookback_sparse", "lookback_dense")


@functools.lru_cache(maxsize=None)
def segment_cases(name):
    """[(label, points)] of one segment-edge case, built once per process; leaf SEG_LEAF"""
    out = SEGMENT_BUILDERS[name](np.random.default_rng(3000 + sorted(SEGMENT_BUILDERS).index(name)))
    assert all(len(p) <= 140_000 for _, p in out)
    return out


# ------------------------------------------------------------------------------------------------- segment edges (unpacked: key / index pairs)
UNPACKED_LEAF = 0.001
UNPACKED_COUNTS = {"tile_edge": [1, 2046, 1, 1, 2047, 1],       # heads at 0, 1, 2047, 2048, 2049, 4096; n = 4097
                   "long_last": [1, 5, 40, 3000]}


def _mid_voxel_anchors(leaf):
    """the corners of a 600 m cube, moved outwards by a few floats until both sit near the middle of their voxels (so that the first and the last voxel
    have room for further points inside the box)"""
    best = None
    a0, a1 = F32(-300.0), F32(300.0)
    for _ in range(80):          # one float more on the high corner moves both corners' places in their voxels, by the same amount in opposite directions
        f = frame_of_box([a0] * 3, [a1] * 3, leaf)
        u = [((float(a) - f.lo[0]) / f.res) % 1.0 for a in (a0, a1)]
        score = max(abs(u[0] - 0.5), abs(u[1] - 0.5))
        if best is None or score < best[0]:
            best = (score, a1)
        a1 = np.nextafter(a1, F32(np.inf))
    assert best[0] < 0.1
    return np.array([[a0] * 3, [best[1]] * 3], F32)


@functools.lru_cache(maxsize=None)
def unpacked_cases(name):
    """the same head positions with voxels taken at random in a 600 m cube at leaf 1 mm (depth 20, all 60 code bits kept): counts assigned in code order,
    the corners' voxels first and last (the Morton code is monotone in every key).  Code bits + index bits exceed 64, so morton_keys, sort_pairs_u64 and
    k_voxel_centroids run instead of the packed kernels."""
    rng = np.random.default_rng(4000 + sorted(UNPACKED_COUNTS).index(name))
    counts = np.array(UNPACKED_COUNTS[name])
    anchors = _mid_voxel_anchors(UNPACKED_LEAF)
    frame = frame_of_box(anchors[0], anchors[1], UNPACKED_LEAF)
    klo, khi = keys_of(np.c_[anchors, np.zeros(2, F32)], frame)
    mid = rng.integers(klo + 2, khi - 1, (len(counts) - 2, 3))
    mid = mid[np.argsort(morton(mid, frame.depth), kind="stable")]
    vox = np.concatenate([klo[None], mid, khi[None]])
    assert len(np.unique(morton(vox, frame.depth))) == len(vox)
    extra = counts.copy()
    extra[0] -= 1
    extra[-1] -= 1
    pts, _ = segments_cloud(anchors, vox, extra, rng, UNPACKED_LEAF, spread=(0.3, 0.7))       # within 0.2 mm of the voxel centre
    r = restate(pts, UNPACKED_LEAF)
    assert (r.heads == np.r_[0, np.cumsum(counts)[:-1]]).all()
    if name == "tile_edge":
        assert len(pts) == 4097 and _has_heads(r, TILE_EDGE_HEADS)
    else:
        assert len(pts) - int(r.heads[-1]) == 3000
    bits, _, depth, _ = _capi().voxel_key_bits(pts[:, :3].min(0), pts[:, :3].max(0), UNPACKED_LEAF)
    index_bits = max(1, math.ceil(math.log2(len(pts))))
    assert depth == 20 and bits + index_bits > 64, "the pair fits one word: the packed kernels would run"
    return [(f"unpacked-{name}", pts)]


# ------------------------------------------------------------------------------------------------- stale frames
STALE_LEAF = 0.05
STALE_N = 3000      # k_bbox_reduce_check on 3000 points: 6 blocks of 256, a second trip from i = 1536, and a ragged last 256-chunk
STALE_ROWS = (1, 64, 256, 1536, STALE_N - 1)
Mutation = collections.namedtuple("Mutation", "label cloud expected identity")


@functools.lru_cache(maxsize=None)
def stale_base():
    """(g, lane-0 row, its zero coordinate, lane-63 row, its zero coordinate): g is an order-preserving subset (all extremal rows kept, so the frame is the
    same) of the oracle's grid of uniform points in a 20 m cube, 3000 rows long, whose row `lane-0 row` (a multiple of 64) holds a +0.0 in one
    coordinate and whose row `lane-63 row` (63 mod 64) holds one in another.  g is its own grid: every row alone in its voxel, rows in code order."""
    rng = np.random.default_rng(8)      # a seed under which no row that a mutation touches is an extremum (asserted in stale_mutations)
    p = np.c_[rng.uniform(-10, 10, (3300, 3)), rng.uniform(1, 255, 3300)].astype(F32)
    first = _orc().voxel_centroid(p, STALE_LEAF)

    def source_of(row):      # the input point that is alone in the voxel of this row (rows near 600 and 1800: room on either side for the trimming below)
        k = np.flatnonzero((p.view(np.uint32) == first[row].view(np.uint32)).all(axis=1))
        assert len(k) == 1
        return int(k[0])

    k0, k1 = source_of(600), source_of(1800)
    p[:, 0] -= p[k0, 0]                                      # x - x: +0.0; the shift moves the whole cloud, box and lattice with it
    p[:, 1] -= p[k1, 1]
    full = _orc().voxel_centroid(p, STALE_LEAF)
    zero = lambda c: np.flatnonzero(full[:, c].view(np.uint32) == 0)      # noqa: E731
    assert len(zero(0)) == 1 and len(zero(1)) == 1
    (ra, ca), (rb, cb) = sorted([(int(zero(0)[0]), 0), (int(zero(1)[0]), 1)])
    keep = np.ones(len(full), bool)
    fixed = {ra, rb} | {int(full[:, d].argmin()) for d in range(3)} | {int(full[:, d].argmax()) for d in range(3)}

    def drop(rows, how_many):
        rows = np.array([r for r in rows if r not in fixed and keep[r]][:how_many], dtype=np.int64)
        assert len(rows) == how_many
        keep[rows] = False

    assert 64 < ra and ra + 200 < rb and rb + 64 < len(full)
    drop(range(0, ra), ra % 64)                              # the first zero row lands on a multiple of 64
    drop(range(ra + 1, rb), ((rb - ra % 64) - 63) % 64)      # the second on 63 mod 64
    drop(range(len(full) - 1, rb, -1), int(keep.sum()) - STALE_N)
    g = np.ascontiguousarray(full[keep])
    ia, ib = int(keep[:ra].sum()), int(keep[:rb].sum())
    assert len(g) == STALE_N and ia % 64 == 0 and ib % 64 == 63
    assert g[ia, ca].view(np.uint32) == 0 and g[ib, cb].view(np.uint32) == 0
    g.setflags(write=False)
    return g, ia, ca, ib, cb


@functools.lru_cache(maxsize=None)
def stale_mutations():
    """[Mutation(label, mutated copy of g, what its grid must be, whether the grid is the identity)].  Asserted for every one: no extremal row is touched
    and the frame is g's; the restatement gives `expected`; and, unless the grid is the identity, the mutated array is not `expected` (a plain copy of
    the input cannot pass)."""
    g, ia, ca, ib, cb = stale_base()
    n = len(g)
    assert n == STALE_N == 3000 and -(-n // 512) == 6 and 6 * 256 == 1536 and n % 256 != 0
    base = restate(g, STALE_LEAF)
    assert (base.centroids.view(np.uint32) == g.view(np.uint32)).all() and (base.heads == np.arange(n)).all(), "g is not its own grid"
    extremal = {int(g[:, d].argmin()) for d in range(3)} | {int(g[:, d].argmax()) for d in range(3)}
    out = []

    def add(label, m, touched, expected, identity=False):
        assert not (set(touched) & extremal), f"{label}: touches an extremal row"
        assert same_frame(frame_of(m, STALE_LEAF), base.frame), f"{label}: the frame moved"
        r = restate(m, STALE_LEAF)
        assert r.centroids.shape == expected.shape and (r.centroids.view(np.uint32) == expected.view(np.uint32)).all(), f"{label}: restatement"
        same = m.shape == expected.shape and bool((m.view(np.uint32) == expected.view(np.uint32)).all())
        assert same == identity, f"{label}: a plain copy of the input would {'not ' if identity else ''}pass"
        m.setflags(write=False)
        expected.setflags(write=False)
        out.append(Mutation(label, m, expected, identity))

    for i in STALE_ROWS:
        assert i not in (ia, ib) and i - 1 not in (ia, ib)
        m = g.copy()
        m[[i - 1, i]] = m[[i, i - 1]]
        add(f"swap({i})", m, (i - 1, i), g.copy())                           # code[i] < code[i - 1]
        m = g.copy()
        m[i] = m[i - 1]
        add(f"dup({i})", m, (i,), np.delete(g, i, axis=0))                   # code[i] == code[i - 1]; (0 + x + x) / 2 == x
    wi = {0: 2048, 63: 2111}                                                 # the intensity rows: lane 0 and lane 63 of a wave of the second trip
    assert wi[0] % 64 == 0 and wi[63] % 64 == 63
    for lane, i, c in ((0, ia, ca), (63, ib, cb)):
        m = g.copy()
        m[i, c] = F32(-0.0)
        add(f"negzero({i},{c})-lane{lane}-coordinate", m, (), g.copy())      # -0.0 == +0.0: no extremum moves; 0 + -0.0 = +0.0
        m = g.copy()
        m[wi[lane], 3] = F32(-0.0)
        e = g.copy()
        e[wi[lane], 3] = F32(0.0)
        add(f"negzero({wi[lane]},3)-lane{lane}-intensity", m, (), e)
    for i in (64, 1536, n - 1):
        m = g.copy()
        m[i, 3] = F32(77.25)
        assert m[i, 3] != g[i, 3]
        add(f"benign({i})", m, (), m.copy(), identity=True)
    return out


# ------------------------------------------------------------------------------------------------- scan sets
SCANSET_LEAF = 0.25


@functools.lru_cache(maxsize=None)
def scanset_case():
    """[keyframe clouds]: a keyframe of octree depth 3 next to one of depth 15; one 2048-point cloud in three consecutive keyframes and a 2048-point
    one-voxel cloud in two (the Morton code of a keyframe's last voxel equals the code of the next keyframe's first: only the keyframe id tells them
    apart); empty keyframes first, last and between"""
    rng = np.random.default_rng(5000)
    cloud = lambda n, side, at=0.0: np.c_[rng.uniform(-side / 2, side / 2, (n, 3)) + at, rng.uniform(0, 255, n)].astype(F32)      # noqa: E731
    empty = np.zeros((0, 4), F32)
    a, b, x = cloud(500, 1.7, 3.0), cloud(700, 5000.0, -900.0), cloud(2048, 3.0, -40.0)
    y = _p4(np.tile(F32([2.5, -1.25, 0.75]), (2048, 1)), rng)
    assert frame_of(a, SCANSET_LEAF).depth == 3 and frame_of(b, SCANSET_LEAF).depth == 15
    assert len(restate(y, SCANSET_LEAF).heads) == 1
    kfs = [empty, a, b, empty, x, x, x, empty, empty, y, y, empty]
    for k in kfs:
        k.setflags(write=False)
    return kfs


# ------------------------------------------------------------------------------------------------- access by name, and the oracle's answers
def cloud_of(kind, name, index):
    if kind == "lattice":
        return lattice_cases(name)[index][1], name
    if kind == "segments":
        return segment_cases(name)[index][1], SEG_LEAF
    if kind == "unpacked":
        return unpacked_cases(name)[index][1], UNPACKED_LEAF
    raise KeyError(kind)


def expected(kind, name, index):
    """the oracle's grid of one fixture, computed once per process and read-only"""
    return _oracle_cached((kind, name, index))
