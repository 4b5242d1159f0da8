"""include/ltm.h, sections "fpfh matches" and "initial alignment", restated in numpy.  Written from the header text; imports nothing of the library.
Matches: for every row of a source record its kc nearest rows of a target record in descriptor space, exhaustively.  The distance is an explicit float32
accumulation loop over the 33 bins (elementwise numpy only, one rounding per operation: no np.dot / einsum / BLAS, which may fuse or reorder), the order a stable sort by distance over the
target rows in their own order, so that ties keep the smaller row first.  The device and this file agree by construction.

    distances(source, target)         (ns, nt) float32: acc = 0; for b in 0..32: e = s[b] - t[b]; acc = acc + e * e
    match(target, source, kc)         (ns, kc) int32 target rows and (ns, kc) float32 distances; unused slots (-1, +inf)

Alignment: pcl::SampleConsensusPrerejective as the header states it.  The hypotheses are plain Python floats (IEEE doubles, one rounding per operation, no
fused multiply-add), the inlier test scipy's cKDTree.query_ball_point at a slightly enlarged radius followed by the exact float32 d2 on the candidates.

    mix(seed, h, j)                   the 32-bit hash of the draws
    draws(seed, h, n_rows, kk)        the three source rows, and given their filled slot counts the three slots
    source_order(points)              the finite points' positions in the index's own order: stable by Morton code under the cloud's own frame
    hypothesis(...)                   (state, T) of one hypothesis, state one of VALID, COINCIDENT, NO_POINT, NO_MATCH, PREREJECTED, DEGENERATE
    align(target, source, match_idx, inlier_distance, ...)   dict: found, best, consensus, n_valid, n_prerejected, n_eval, T (4, 4), hyp_valid, hyp_counts,
                                      states (per hypothesis)
"""
import math

import numpy as np

SIZE, MIN_KC, MAX_KC = 33, 1, 16


def distances(source, target):
    s = np.ascontiguousarray(source, dtype=np.float32).reshape(-1, SIZE)
    t = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, SIZE)
    acc = np.zeros((len(s), len(t)), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(SIZE):
            e = s[:, b][:, None] - t[:, b][None, :]
            acc = acc + e * e
    assert acc.dtype == np.float32
    return acc


def match(target, source, kc):
    """A target row with a NaN component is not eligible, a source row with one has no matches, a candidate whose distance is NaN (two infinities met) is not
    listed; the rest ascending by (distance, target row), the first kc of them"""
    if not MIN_KC <= kc <= MAX_KC:
        raise ValueError("need 1 <= kc <= 16")
    s = np.ascontiguousarray(source, dtype=np.float32).reshape(-1, SIZE)
    t = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, SIZE)
    idx = np.full((len(s), kc), -1, np.int32)
    dist = np.full((len(s), kc), np.inf, np.float32)
    eligible = np.flatnonzero(~np.isnan(t).any(axis=1))
    rows = np.flatnonzero(~np.isnan(s).any(axis=1))
    chunk = max(1, (1 << 22) // max(len(eligible), 1))
    for a in range(0, len(rows), chunk):
        r = rows[a:a + chunk]
        d = distances(s[r], t[eligible])
        for j, row in enumerate(r):
            listable = np.flatnonzero(~np.isnan(d[j]))
            order = listable[np.argsort(d[j][listable], kind="stable")][:kc]      # eligible is ascending: stable = ties to the smaller row
            idx[row, :len(order)] = eligible[order]
            dist[row, :len(order)] = d[j][order]
    return idx, dist


# ------------------------------------------------------------------------------------------------------------------ initial alignment
VALID, COINCIDENT, NO_POINT, NO_MATCH, PREREJECTED, DEGENERATE = range(6)
MAX_ITERATIONS = 16384
M32 = 0xFFFFFFFF


def mix(seed, h, j):
    """murmur3's finaliser over seed + 0x9E3779B9 (6 h + j + 1), modulo 2^32"""
    x = (seed + 0x9E3779B9 * (6 * h + j + 1)) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def draws(seed, h, n_rows, kk=None):
    """s_j = (mix_j n_rows) >> 32; with kk = the filled slots of those three rows also m_j = (mix_{3+j} kk_j) >> 32"""
    s = [(mix(seed, h, j) * n_rows) >> 32 for j in range(3)]
    if kk is None:
        return s
    return s, [(mix(seed, h, 3 + j) * kk[j]) >> 32 for j in range(3)]


def _morton(q):
    code = np.zeros(len(q), np.uint64)
    for b in range(20, -1, -1):
        sh, one = np.uint64(b), np.uint64(1)
        code = (code << np.uint64(3)) | (((q[:, 0] >> sh) & one) << np.uint64(2)) | (((q[:, 1] >> sh) & one) << one) | ((q[:, 2] >> sh) & one)
    return code


def source_order(points):
    """positions (into `points`) of the finite points in the index's own order: origin = the box's minimum, scale = 2097151 / the largest extent (0 for a
    point), q = floor(((double)v - o) * scale) clamped to [0, 2097151] per axis, codes interleaved with x most significant, a stable sort"""
    p = _xyz(points)
    fin = np.flatnonzero(np.isfinite(p).all(axis=1))
    if not len(fin):
        return fin
    f = p[fin]
    mn, mx = f.min(axis=0).astype(np.float64), f.max(axis=0).astype(np.float64)
    ext = float((mx - mn).max())
    scale = 2097151.0 / ext if ext > 0.0 else 0.0
    q = np.clip(np.floor((f.astype(np.float64) - mn) * scale), 0.0, 2097151.0).astype(np.uint64)
    return fin[np.argsort(_morton(q), kind="stable")]


def _xyz(points):
    """(n, 3) or (n, 4) points -> float32 xyz"""
    a = np.asarray(points, np.float32)
    return np.zeros((0, 3), np.float32) if a.size == 0 else np.ascontiguousarray(a.reshape(len(a), -1)[:, :3])


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _frame(a):
    """(e1, e2, e3), centroid of the triangle a[0], a[1], a[2] (lists of Python floats); None where a squared length is 0 or not finite"""
    u = _sub(a[1], a[0])
    uu = _dot(u, u)
    n = _cross(u, _sub(a[2], a[0]))
    nn = _dot(n, n)
    if not (uu > 0.0 and nn > 0.0 and math.isfinite(uu) and math.isfinite(nn)):
        return None
    lu, ln = math.sqrt(uu), math.sqrt(nn)
    e1, e3 = [v / lu for v in u], [v / ln for v in n]
    return (e1, _cross(e3, e1), e3), [((a[0][d] + a[1][d]) + a[2][d]) / 3.0 for d in range(3)]


def hypothesis(seed, h, source, target, match_idx, similarity_threshold):
    """source, target: (n, 3) float32 in ORIGINAL order; match_idx: (n_source, kc) int32"""
    n = len(source)
    if n < 3:
        return COINCIDENT, None
    s = draws(seed, h, n)
    if len(set(s)) < 3:
        return COINCIDENT, None
    kk = [int((match_idx[r] >= 0).sum()) for r in s]
    state = VALID
    for j in range(3):
        if not np.isfinite(source[s[j]]).all():
            state = NO_POINT
        elif kk[j] == 0:
            state = NO_MATCH
        if state != VALID:
            return state, None
    _, m = draws(seed, h, n, kk)
    t = [int(match_idx[s[j], m[j]]) for j in range(3)]
    if len(set(t)) < 3:
        return COINCIDENT, None
    if not all(np.isfinite(target[r]).all() for r in t):
        return NO_POINT, None
    a = [[float(v) for v in source[r]] for r in s]
    b = [[float(v) for v in target[r]] for r in t]
    thr2 = similarity_threshold * similarity_threshold
    for i, k in ((0, 1), (1, 2), (2, 0)):
        da, db = _sub(a[i], a[k]), _sub(b[i], b[k])
        ls, lt = _dot(da, da), _dot(db, db)
        if not (min(ls, lt) >= thr2 * max(ls, lt)):
            return PREREJECTED, None
    fs, ft = _frame(a), _frame(b)
    if fs is None or ft is None:
        return DEGENERATE, None
    (f, cs), (g, ct) = fs, ft
    T = np.eye(4)
    for r in range(3):
        for c in range(3):
            T[r, c] = (g[0][r] * f[0][c] + g[1][r] * f[1][c]) + g[2][r] * f[2][c]
        T[r, 3] = ct[r] - ((float(T[r, 0]) * cs[0] + float(T[r, 1]) * cs[1]) + float(T[r, 2]) * cs[2])
    return VALID, T


def transform_to_float(T, pts):
    """step 1 of "icp": x' = ((T00 x + T01 y) + T02 z) + T03 in double, rounded to float"""
    p = pts.astype(np.float64)
    out = np.empty((len(p), 3), np.float64)
    for r in range(3):
        out[:, r] = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]
    with np.errstate(over="ignore"):
        return out.astype(np.float32)


def count_inliers(tree, target_finite, queries, inlier_distance):
    """queries (n, 3) float32; a query is an inlier iff some target point has float32 ((dx*dx)+dy*dy)+dz*dz, as a double, <= inlier_distance^2"""
    ok = np.isfinite(queries).all(axis=1)
    q = queries[ok]
    if not len(q) or not len(target_finite):
        return 0
    r2 = inlier_distance * inlier_distance
    lists = tree.query_ball_point(q.astype(np.float64), inlier_distance * (1.0 + 1e-4) + 1e-5)
    lens = np.fromiter((len(x) for x in lists), np.int64, len(lists))
    if not lens.sum():
        return 0
    qi = np.repeat(np.arange(len(q)), lens)
    ti = np.fromiter((j for x in lists for j in x), np.int64, int(lens.sum()))
    d = q[qi] - target_finite[ti]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == np.float32
    hit = d2.astype(np.float64) <= r2
    return int(len(np.unique(qi[hit])))


def align(target, source, match_idx, inlier_distance, max_iterations=1000, seed=0, similarity_threshold=0.9, inlier_fraction=0.25, eval_stride=1, order=None):
    """order: the source index's own order (positions of its finite points), source_order(source) if None"""
    from scipy.spatial import cKDTree
    target, source = _xyz(target), _xyz(source)
    match_idx = np.asarray(match_idx, np.int32).reshape(len(source), -1) if len(source) else np.zeros((0, 1), np.int32)
    if not (1 <= max_iterations <= MAX_ITERATIONS and 0.0 <= similarity_threshold < 1.0 and inlier_distance > 0.0 and math.isfinite(inlier_distance)
            and 0.0 <= inlier_fraction <= 1.0 and eval_stride >= 1):
        raise ValueError("parameters outside the domain")
    order = source_order(source) if order is None else np.asarray(order)
    voters = source[order[::eval_stride]]
    tf = target[np.isfinite(target).all(axis=1)]
    tree = cKDTree(tf.astype(np.float64)) if len(tf) else None
    H = max_iterations
    states = np.empty(H, np.int32)
    counts = np.zeros(H, np.uint32)
    Ts = [None] * H
    for h in range(H):
        states[h], Ts[h] = hypothesis(seed, h, source, target, match_idx, similarity_threshold)
        if states[h] == VALID and tree is not None and len(voters):
            counts[h] = count_inliers(tree, tf, transform_to_float(Ts[h], voters), inlier_distance)
    valid = states == VALID
    res = dict(hyp_valid=valid.astype(np.uint8), hyp_counts=counts, states=states, n_valid=int(valid.sum()), n_prerejected=int((states == PREREJECTED).sum()),
               n_eval=len(voters), best=-1, consensus=0, found=0, T=np.full((4, 4), np.nan))
    if valid.any():
        key = np.where(valid, counts.astype(np.int64), -1)
        best = int(np.argmax(key))      # the first occurrence of the maximum: ties to the smaller h
        res.update(best=best, consensus=int(counts[best]), T=Ts[best])
        res["found"] = int(float(res["consensus"]) >= inlier_fraction * float(res["n_eval"]) and res["consensus"] >= 3)
    return res
