"""Normals of a cloud as include/ltm.h ("normals") states them, restated in numpy: what the tests hold ltm_search_estimate_normals against.  Written
from the header text; imports nothing of the library.  Brute-force float32 neighbours in a stable order (L2_Simple, ties to the smaller target index),
moments in double about the point itself, summed in neighbourhood order, np.linalg.eigh.

    r = estimate(target_xyz, k, viewpoint=(0, 0, 0))
    r: dict with normals (n, 4) float32 -- (nx, ny, nz, curvature) in the target's order, NaN rows for non-finite points and for fewer than 3 neighbours --
       normals64 (n, 4) the same before the rounding to float, eigenvalues (n, 3) ascending, gap (n,) = (l1 - l0) / l2 (0 where l2 is 0), and
       neighbours (n, kk) the neighbourhoods as target indices (-1 rows for non-finite points)."""
import numpy as np


def neighbours(pts, kk):
    """(m, kk) indices of the kk nearest points of every point among `pts` (m, 3) float32 itself: ((dx*dx)+dy*dy)+dz*dz in float32, ascending, a stable
    sort so that equal distances keep the smaller index first"""
    m = len(pts)
    out = np.empty((m, kk), np.int64)
    chunk = max(1, (1 << 22) // max(m, 1))
    x, y, z = pts[:, 0][None, :], pts[:, 1][None, :], pts[:, 2][None, :]
    for a in range(0, m, chunk):
        q = pts[a:a + chunk]
        with np.errstate(over="ignore"):
            dx, dy, dz = q[:, 0:1] - x, q[:, 1:2] - y, q[:, 2:3] - z
            d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        out[a:a + chunk] = np.argsort(d, axis=1, kind="stable")[:, :kk]
    return out


def canonical_sign(n):
    """the component of largest magnitude positive, the lower axis among equals"""
    big = np.argmax(np.abs(n), axis=1)      # the first maximum
    s = np.where(n[np.arange(len(n)), big] < 0.0, -1.0, 1.0)
    return n * s[:, None]


def estimate(target, k, viewpoint=(0.0, 0.0, 0.0)):
    if not 3 <= int(k) <= 64:
        raise ValueError("k must be in [3, 64]")
    target = np.asarray(target, dtype=np.float32)
    if target.ndim != 2:
        target = target.reshape(-1, 3)
    target = np.ascontiguousarray(target[:, :3])
    n = len(target)
    vp = np.asarray(viewpoint, dtype=np.float64).reshape(3)
    fin = np.isfinite(target).all(axis=1)
    where = np.flatnonzero(fin)
    pts = target[fin]
    m = len(pts)
    kk = min(int(k), m)
    res = dict(normals=np.full((n, 4), np.nan, np.float32), normals64=np.full((n, 4), np.nan), eigenvalues=np.full((n, 3), np.nan),
               gap=np.full(n, np.nan), neighbours=np.full((n, max(kk, 0)), -1, np.int64))
    if kk < 3:
        return res
    nb = neighbours(pts, kk)
    p = pts.astype(np.float64)
    s = np.zeros((m, 3))
    c = np.zeros((m, 3, 3))
    for j in range(kk):      # the neighbourhood's ascending (d2, index) order
        d = p[nb[:, j]] - p
        s += d
        c += d[:, :, None] * d[:, None, :]
    mean = s / kk
    cov = c / kk - mean[:, :, None] * mean[:, None, :]
    w, v = np.linalg.eigh(cov)      # ascending eigenvalues
    nrm = v[:, :, 0]
    nrm = nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]
    nrm = canonical_sign(nrm)
    to_vp = vp[None, :] - p
    dot = (to_vp[:, 0] * nrm[:, 0] + to_vp[:, 1] * nrm[:, 1]) + to_vp[:, 2] * nrm[:, 2]
    nrm = np.where((dot < 0.0)[:, None], -nrm, nrm)
    tr = w.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.where(tr > 0.0, np.maximum(w[:, 0], 0.0) / tr, 0.0)
        gap = np.where(w[:, 2] > 0.0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
    full = np.concatenate([nrm, curv[:, None]], axis=1)
    res["normals64"][where] = full
    res["normals"][where] = full.astype(np.float32)
    res["eigenvalues"][where] = w
    res["gap"][where] = gap
    res["neighbours"][where] = where[nb]
    res["view_dot"] = np.full(n, np.nan)
    res["view_dot"][where] = dot
    return res
