"""Restatement of include/ltm.h, section "clusters" (pcl::EuclideanClusterExtraction as this library understands it), with scipy: the GPU tests compare
ltm_search_cluster against this for equality.

Candidate pairs come from a k-d tree at tolerance * (1 + 1e-5): the float32 distance of the library is within 3e-7 relative of the exact one
(ltm_k_search.hip), so no pair with float d2 < r2 lies outside that radius.  The candidates are then filtered by the float32 expression itself,
((dx*dx)+dy*dy)+dz*dz evaluated with numpy float32 operations in that order, against r2 = float32(float64(tolerance)^2), strict <.
Where squares underflow the float distance can also lie 1.5 * 2^-149 BELOW the exact one (each of the three squares loses up to half a denormal spacing:
three squares below 2^-150 give d2 = 0 for a pair 1.2e-22 apart), and r2 itself is rounded to a denormal, up by half a spacing at the most: the squared
candidate radius is enlarged by 2^-147, which is nothing at any tolerance above 1e-19."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


UNDERFLOW_SLACK = 2.0 ** -147      # added to the squared candidate radius: see above


def r2_of(tolerance):
    return np.float32(np.float64(tolerance) * np.float64(tolerance))


def d2_float32(a, b):
    """FLANN's L2_Simple in float32 between the rows of a and b (float32 [n, 3])"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    dx, dy, dz = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1], a[:, 2] - b[:, 2]
    return ((dx * dx) + dy * dy) + dz * dz


def ordered_key(f):
    """the order-preserving float32 -> uint32 key of the library's boxes (-0.0 below +0.0)"""
    u = np.asarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _xyz(points):
    p = np.asarray(points, np.float32)
    return (p if p.ndim == 2 else p.reshape(-1, 3))[:, :3]


def edges(points, tolerance):
    """(i, j) pairs of finite points adjacent under the library's relation, original indices, i < j"""
    p = _xyz(points)
    fin = np.flatnonzero(np.isfinite(p).all(axis=1))
    if len(fin) < 2:
        return np.zeros((0, 2), np.int64), fin
    q = p[fin]
    with np.errstate(over="ignore", invalid="ignore"):
        reach = float(tolerance) * (1.0 + 1e-5)
        cand = cKDTree(q.astype(np.float64)).query_pairs(float(np.sqrt(reach * reach + UNDERFLOW_SLACK)), output_type="ndarray")
        if len(cand) == 0:
            return np.zeros((0, 2), np.int64), fin
        keep = d2_float32(q[cand[:, 0]], q[cand[:, 1]]) < r2_of(tolerance)
    return fin[cand[keep]].astype(np.int64), fin


def from_components(points, comp_of_point, min_size=1, max_size=None):
    """filter, canonical order and per-cluster values from a component id per point (-1: not a vertex).  Returns a dict: labels int32 [n], sizes uint32,
    first int32, offsets uint64 [nc + 1], idx int32, boxes float32 [nc, 6], centroids float64 [nc, 3]."""
    p = _xyz(points)
    n = len(p)
    comp = np.asarray(comp_of_point, np.int64)
    vert = np.flatnonzero(comp >= 0)
    uniq, inv, cnt = np.unique(comp[vert], return_inverse=True, return_counts=True)
    first = np.full(len(uniq), n, np.int64)
    np.minimum.at(first, inv, vert)
    ok = cnt >= int(min_size)
    if max_size:
        ok &= cnt <= int(max_size)
    kept = np.flatnonzero(ok)
    kept = kept[np.lexsort((first[kept], -cnt[kept]))]      # size descending, then lowest original index
    number = np.full(len(uniq), -1, np.int64)
    number[kept] = np.arange(len(kept))
    labels = np.full(n, -1, np.int32)
    labels[vert] = number[inv]
    nc = len(kept)
    sizes = cnt[kept].astype(np.uint32)
    offsets = np.zeros(nc + 1, np.uint64)
    offsets[1:] = np.cumsum(sizes, dtype=np.uint64)
    member = np.flatnonzero(labels >= 0)
    idx = member[np.argsort(labels[member], kind="stable")].astype(np.int32)      # ascending original index inside a cluster
    boxes = np.zeros((nc, 6), np.float32)
    cent = np.zeros((nc, 3), np.float64)
    for c in range(nc):
        q = p[idx[int(offsets[c]):int(offsets[c + 1])]]
        k = ordered_key(q)
        boxes[c, :3] = q[k.argmin(axis=0), np.arange(3)]
        boxes[c, 3:] = q[k.argmax(axis=0), np.arange(3)]
        cent[c] = q.astype(np.float64).mean(axis=0)
    return dict(labels=labels, sizes=sizes, first=first[kept].astype(np.int32), offsets=offsets, idx=idx, boxes=boxes, centroids=cent)


def cluster(points, tolerance, min_size=1, max_size=None):
    """the clusters of `points` ((n, 3) or (n, 4) float32) as ltm_search_cluster gives them"""
    p = _xyz(points)
    n = len(p)
    e, fin = edges(p, tolerance)
    comp = np.full(n, -1, np.int64)
    if len(fin):
        g = coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(n, n))
        _, lab = connected_components(g, directed=False)
        comp[fin] = lab[fin]
    return from_components(p, comp, min_size, max_size)
