"""include/ltm.h, section "fpfh", restated in numpy: Fast Point Feature Histograms (Rusu et al.; pcl::FPFHEstimation with setKSearch) of one cloud with
given normals, as this library takes PCL 1.10 to compute them.  Written from the header text; imports nothing of the library.  Neighbourhoods are brute-force
float32 L2_Simple in a stable order (ties to the smaller index); everything after them is float64 with one rounding per operation: elementwise numpy only,
no np.dot / einsum / BLAS, which may fuse or reorder.  The device and this file agree by construction.

    neighbours(pts, kk)               (m, kk) indices and (m, kk) float32 d2 of the kk nearest points of every point of `pts` (m, 3) float32
    bin_unit(f)                       the bin of alpha / phi
    bin_theta(y, x)                   the bin of theta = atan2(y, x) by sign tests against THETA_TABLE
    bin_theta_atan2(y, x)             PCL's floor(11 (atan2(y, x) + pi) / (2 pi)), clamped: what bin_theta stands for
    pair_bins(p, n_p, q, n_q)         (skipped, alpha bin, phi bin, theta bin) of pairs, all arrays of the same length
    fpfh(points, normals, k)          dict: descriptors float32 (n, 33), spfh_counts uint8 (n, 33), n_target, n_finite, pairs_skipped, neighbours (n, kk)
"""
import numpy as np

BINS, SIZE, MIN_K, MAX_K = 11, 33, 2, 64
# (c_j, s_j) of boundary theta_j = -pi + 2 pi j / 11, j = 1 .. 10: the copy of lt-mapper_amd/csrc/ltm_fpfh_bins.h
THETA_TABLE = (
    (-0.8412535328311811, -0.5406408174555978),
    (-0.4154150130018863, -0.9096319953545184),
    (0.14231483827328512, -0.9898214418809327),
    (0.6548607339452851, -0.7557495743542583),
    (0.9594929736144975, -0.2817325568414295),
    (0.9594929736144975, 0.2817325568414295),
    (0.6548607339452851, 0.7557495743542583),
    (0.14231483827328512, 0.9898214418809327),
    (-0.41541501300188616, 0.9096319953545186),
    (-0.8412535328311813, 0.5406408174555974),
)


def neighbours(pts, kk):
    """((dx*dx)+dy*dy)+dz*dz in float32, dx = query - target, ascending, a stable sort so that equal distances keep the smaller index first"""
    m = len(pts)
    nb = np.empty((m, kk), np.int64)
    d2 = np.empty((m, kk), np.float32)
    chunk = max(1, (1 << 22) // max(m, 1))
    x, y, z = pts[:, 0][None, :], pts[:, 1][None, :], pts[:, 2][None, :]
    for a in range(0, m, chunk):
        q = pts[a:a + chunk]
        with np.errstate(over="ignore"):
            dx, dy, dz = q[:, 0:1] - x, q[:, 1:2] - y, q[:, 2:3] - z
            d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        order = np.argsort(d, axis=1, kind="stable")[:, :kk]
        nb[a:a + chunk] = order
        d2[a:a + chunk] = np.take_along_axis(d, order, axis=1)
    return nb, d2


def bin_unit(f):
    t = 11.0 * ((np.asarray(f, np.float64) + 1.0) * 0.5)
    return np.clip(np.floor(t), 0.0, 10.0).astype(np.int64)


def bin_theta(y, x):
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    upper = ~np.signbit(y)
    b = np.zeros(y.shape, np.int64)
    for j, (c, s) in enumerate(THETA_TABLE, start=1):
        side = (c * y - s * x) >= 0.0
        b += ((upper | side) if j <= 5 else (upper & side)).astype(np.int64)
    return np.where((x == 0.0) & (y == 0.0), 5, b)


def bin_theta_atan2(y, x):
    t = np.arctan2(np.asarray(y, np.float64), np.asarray(x, np.float64))
    return np.clip(np.floor(11.0 * (t + np.pi) / (2.0 * np.pi)), 0.0, 10.0).astype(np.int64)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def pair_bins(p, n_p, q, n_q):
    """computePairFeatures of (p, q) with normals (n_p, n_q), all (m, 3) float64; a skipped pair's bins are meaningless"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = q - p
        f4 = np.sqrt(_dot(d, d))
        a1 = _dot(n_p, d) / f4
        a2 = _dot(n_q, d) / f4
        swap = np.abs(a1) < np.abs(a2)
        u = np.where(swap[:, None], n_q, n_p)
        other = np.where(swap[:, None], n_p, n_q)
        d = np.where(swap[:, None], -d, d)
        phi = np.where(swap, -a2, a1)
        v = _cross(d, u)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[:, None]
        w = _cross(u, v)
        alpha = _dot(v, other)
        y, x = _dot(w, other), _dot(u, other)
        skipped = (f4 == 0.0) | (vn == 0.0) | ~np.isfinite(n_q).all(axis=1)
        return skipped, bin_unit(alpha), bin_unit(phi), bin_theta(y, x)


def _rows3(a):
    """the first three columns of an (n, 3) or (n, 4) array, float32"""
    a = np.asarray(a, np.float32)
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1] if a.ndim == 2 else 3)[:, :3])


def fpfh(points, normals, k):
    if not MIN_K <= int(k) <= MAX_K:
        raise ValueError("k must be in [2, 64]")
    points, normals = _rows3(points), _rows3(normals)
    assert points.dtype == np.float32 and normals.dtype == np.float32 and len(points) == len(normals)
    n = len(points)
    fin = np.isfinite(points).all(axis=1)
    where = np.flatnonzero(fin)
    pts, nrm = points[fin], normals[fin].astype(np.float64)
    m = len(pts)
    kk = min(int(k), m)
    res = dict(descriptors=np.full((n, SIZE), np.nan, np.float32), spfh_counts=np.zeros((n, SIZE), np.uint8), n_target=n, n_finite=m, pairs_skipped=0,
               neighbours=np.full((n, kk), -1, np.int64))
    if m == 0:
        return res
    nb, d2 = neighbours(pts, kk)
    valid = np.isfinite(nrm).all(axis=1)      # a point whose normal is not finite: no counts, a NaN row
    p64 = pts.astype(np.float64)
    counts = np.zeros((m, SIZE), np.int64)
    rows = np.arange(m)
    skipped_total = 0
    for j in range(kk):
        qj = nb[:, j]
        skipped, ba, bp, bt = pair_bins(p64, nrm, p64[qj], nrm[qj])
        pair = valid & (qj != rows)
        skipped_total += int((pair & skipped).sum())
        use = np.flatnonzero(pair & ~skipped)
        np.add.at(counts, (use, ba[use]), 1)
        np.add.at(counts, (use, BINS + bp[use]), 1)
        np.add.at(counts, (use, 2 * BINS + bt[use]), 1)
    assert counts.max(initial=0) <= 63
    # weightPointSPFHSignature: S_b = sum over the neighbourhood in list order of (1 / d2) count_q[b], skipping d2 == 0
    S = np.zeros((m, SIZE))
    c64 = counts.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):      # d2 == 0: w is inf and the term is not used
        for j in range(kk):
            w = 1.0 / d2[:, j].astype(np.float64)
            term = w[:, None] * c64[nb[:, j]]
            S = np.where((d2[:, j] != 0.0)[:, None], S + term, S)
    desc = np.zeros((m, SIZE))
    for g in range(3):
        T = np.zeros(m)
        for b in range(BINS):
            T = T + S[:, g * BINS + b]
        with np.errstate(invalid="ignore", divide="ignore"):
            scaled = 100.0 * S[:, g * BINS:(g + 1) * BINS] / T[:, None]
        desc[:, g * BINS:(g + 1) * BINS] = np.where((T == 0.0)[:, None], 0.0, scaled)
    desc = desc.astype(np.float32)
    desc[~valid] = np.nan
    res["descriptors"][where] = desc
    res["spfh_counts"][where] = counts.astype(np.uint8)
    res["pairs_skipped"] = skipped_total
    res["neighbours"][where] = where[nb]
    return res
