"""include/ltm.h, section "outlier filters", restated in numpy: statistical and radius outlier removal over one cloud, as this library takes PCL 1.10's
StatisticalOutlierRemoval / RadiusOutlierRemoval to do.  Written from the header text.  Distances are brute-force float32 L2_Simple (numpy rounds every
float32 operation once and fuses nothing), the square roots, the divide and the record statistics are float64 in the header's order, the sums have the
header's fixed shape written out: the device and this file agree by construction.

    d2_rows(xyz, rows)                         float32 [len(rows), n_finite]: squared distances of some finite points to all finite points
    fixed_sum(values)                          the double sum in the fixed shape of "clusters"
    sor_distances(points, mean_k)              float32 [n]: d_i in original order, 0 for non-finite points
    sor_statistics(dist, n_finite, stddev_mul, clamp=True)   (mean, stddev, threshold, variance before the clamp)
    statistical(points, mean_k, stddev_mul)    everything, as a dict
    radius(points, radius, min_neighbors)      everything, as a dict
    statistical_large / radius_large           the same through scipy.spatial.cKDTree candidates, for inputs too large for brute force (the bench tool)
"""
import math

import numpy as np

CHUNK, GROUP = 256, 64
MAX_MEAN_K = 63
SOR_DEFAULTS = dict(mean_k=1, stddev_mul=0.0)          # PCL's constructor
ROR_DEFAULTS = dict(radius=0.0, min_neighbors=1)       # the radius must be set
_ROWS = 1024                                           # query rows per block of the brute-force distance matrix


def _xyz(points):
    p = np.asarray(points, dtype=np.float32)
    return p.reshape(-1, p.shape[-1] if p.ndim == 2 else 4)[:, :3]


def finite_mask(points):
    return np.isfinite(_xyz(points)).all(axis=1)


def d2_rows(xyz, rows):
    """((dx*dx)+dy*dy)+dz*dz in float32, one rounding per operation, dx = query - target"""
    q = xyz[rows]
    dx = q[:, None, 0] - xyz[None, :, 0]
    dy = q[:, None, 1] - xyz[None, :, 1]
    dz = q[:, None, 2] - xyz[None, :, 2]
    r = dx * dx
    r = r + dy * dy
    r = r + dz * dz
    assert r.dtype == np.float32
    return r


def _tree(a, first):
    """rows of `a` summed by the binary tree that adds entries `first` apart, then first / 2, ... 1"""
    s = first
    while s:
        a = a[:, :s] + a[:, s:2 * s]
        s //= 2
    return a[:, 0]


def fixed_sum(values):
    """chunks of 256 consecutive entries, the last padded with zeros, each by a tree (128 apart first); the chunk sums 64 at a time, the last group padded
    with zeros, each by a tree (32 apart first); the group sums added in order to 0.0"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    n_chunks = -(-len(v) // CHUNK)
    padded = np.zeros(n_chunks * CHUNK)
    padded[:len(v)] = v
    chunk_sums = _tree(padded.reshape(n_chunks, CHUNK), CHUNK // 2) if n_chunks else np.zeros(0)
    n_groups = -(-n_chunks // GROUP)
    padded = np.zeros(n_groups * GROUP)
    padded[:n_chunks] = chunk_sums
    group_sums = _tree(padded.reshape(n_groups, GROUP), GROUP // 2) if n_groups else np.zeros(0)
    total = 0.0
    for g in group_sums.tolist():
        total = total + g
    return total


def _distance_from_sorted_d2(d2_sorted, mean_k):
    """rows of ascending d2 (the first is the point itself) -> (float)(sum of double sqrt past the first / mean_k), the terms added in ascending order"""
    terms = np.sqrt(d2_sorted[:, 1:].astype(np.float64))
    s = np.zeros(len(d2_sorted))
    for j in range(terms.shape[1]):
        s = s + terms[:, j]
    return (s / float(mean_k)).astype(np.float32)


def sor_distances(points, mean_k):
    assert 1 <= int(mean_k) <= MAX_MEAN_K
    xyz = _xyz(points)
    fin = np.flatnonzero(finite_mask(points))
    f = xyz[fin]
    kk = min(int(mean_k) + 1, len(f))
    out = np.zeros(len(xyz), np.float32)
    for a in range(0, len(f), _ROWS):
        rows = np.arange(a, min(a + _ROWS, len(f)))
        d2 = d2_rows(f, rows)
        nearest = np.sort(np.partition(d2, kk - 1, axis=1)[:, :kk], axis=1)      # the kk smallest d2 of every row, ascending
        out[fin[rows]] = _distance_from_sorted_d2(nearest, mean_k)
    return out


def sor_statistics(dist, n_finite, stddev_mul, clamp=True):
    d = np.asarray(dist, dtype=np.float32).astype(np.float64)
    total, sq_total = fixed_sum(d), fixed_sum(d * d)
    n = float(n_finite)
    mean = stddev = variance = 0.0
    if n_finite >= 1:
        mean = total / n
    if n_finite >= 2:
        variance = (sq_total - (total * total) / n) / (n - 1.0)
        stddev = math.sqrt(variance if variance > 0.0 else 0.0) if clamp else (math.sqrt(variance) if variance >= 0.0 else math.nan)
    threshold = mean + float(stddev_mul) * stddev if n_finite else 0.0
    return mean, stddev, threshold, variance


def _sor_result(points, dist, stddev_mul):
    fin = finite_mask(points)
    mean, stddev, threshold, variance = sor_statistics(dist, int(fin.sum()), stddev_mul)
    labels = (fin & (dist.astype(np.float64) <= threshold)).astype(np.uint8)
    return dict(distances=dist, labels=labels, n_target=len(fin), n_finite=int(fin.sum()), n_kept=int(labels.sum()), mean=mean, stddev=stddev,
                threshold=threshold, variance_unclamped=variance)


def statistical(points, mean_k, stddev_mul):
    assert math.isfinite(float(stddev_mul))
    return _sor_result(points, sor_distances(points, mean_k), stddev_mul)


def sor_labels(points, dist, threshold):
    """the label expression at given distances and a given threshold"""
    return (finite_mask(points) & (np.asarray(dist, np.float32).astype(np.float64) <= float(threshold))).astype(np.uint8)


def r2_of(radius):
    return np.float32(float(radius) * float(radius))


def _ror_result(points, neighbours, min_neighbors):
    fin = finite_mask(points)
    counts = np.minimum(neighbours, int(min_neighbors)).astype(np.uint32)
    labels = (fin & (counts == int(min_neighbors))).astype(np.uint8)
    return dict(counts=counts, labels=labels, n_target=len(fin), n_finite=int(fin.sum()), n_kept=int(labels.sum()))


def radius(points, radius, min_neighbors=1):
    assert math.isfinite(float(radius)) and float(radius) > 0.0 and int(min_neighbors) >= 1
    xyz = _xyz(points)
    fin = np.flatnonzero(finite_mask(points))
    f = xyz[fin]
    r2 = r2_of(radius)
    neighbours = np.zeros(len(xyz), np.int64)
    for a in range(0, len(f), _ROWS):
        rows = np.arange(a, min(a + _ROWS, len(f)))
        neighbours[fin[rows]] = (d2_rows(f, rows) < r2).sum(axis=1)      # strict, the point itself included
    return _ror_result(points, neighbours, min_neighbors)


# ------------------------------------------------------------------------------------------------ large inputs (tools/bench_outliers.py)
def statistical_large(points, mean_k, stddev_mul, slack=8):
    """`statistical` with the candidates from scipy's kd-tree: the mean_k + 1 + slack nearest in float64, their d2 recomputed in float32 L2_Simple and the
    smallest taken.  Exact unless more than `slack` float32 ties straddle the last neighbour, which the assertion below would catch."""
    from scipy.spatial import cKDTree
    xyz = _xyz(points)
    fin = np.flatnonzero(finite_mask(points))
    f = xyz[fin]
    kk = min(int(mean_k) + 1, len(f))
    out = np.zeros(len(xyz), np.float32)
    if len(f):
        kq = min(kk + slack, len(f))
        _, nb = cKDTree(f.astype(np.float64)).query(f.astype(np.float64), k=kq)
        nb = nb.reshape(len(f), kq)
        d = f[:, None, :] - f[nb]
        d2 = d[:, :, 0] * d[:, :, 0]
        d2 = d2 + d[:, :, 1] * d[:, :, 1]
        d2 = d2 + d[:, :, 2] * d[:, :, 2]
        d2 = np.sort(d2, axis=1)
        assert kq == len(f) or (d2[:, kk - 1] < d2[:, kq - 1]).all() or kq == kk, "float32 ties beyond the slack: raise it"
        out[fin] = _distance_from_sorted_d2(d2[:, :kk], mean_k)
    return _sor_result(points, out, stddev_mul)


def radius_large(points, radius, min_neighbors=1):
    """`radius` with the candidates from scipy's kd-tree at a slightly larger float64 radius, the float32 relation applied to them"""
    from scipy.spatial import cKDTree
    xyz = _xyz(points)
    fin = np.flatnonzero(finite_mask(points))
    f = xyz[fin]
    r2 = r2_of(radius)
    neighbours = np.zeros(len(xyz), np.int64)
    if len(f):
        tree = cKDTree(f.astype(np.float64))
        cand = tree.query_ball_point(f.astype(np.float64), float(radius) * (1.0 + 1e-5) + 1e-12)
        for i, c in enumerate(cand):
            c = np.asarray(c, dtype=np.int64)
            d = f[i][None, :] - f[c]
            d2 = d[:, 0] * d[:, 0]
            d2 = d2 + d[:, 1] * d[:, 1]
            d2 = d2 + d[:, 2] * d[:, 2]
            neighbours[fin[i]] = int((d2 < r2).sum())
    return _ror_result(points, neighbours, min_neighbors)
