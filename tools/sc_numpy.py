"""numpy restatement of the reference's Scan Context (ltslam/src/Scancontext.cpp:23-36, :69-324; nanoflann.hpp:383-409), written from those lines
and from nothing else: it shares no code with the library.  float32 where the reference computes in float, float64 where it computes in double,
sums in the order of the reference's loops (np.cumsum adds sequentially).  Used by tests/test_gpu_scancontext.py as the expected result and by
tools/bench_scancontext.py as the one-thread CPU timing.  It is the tests' expected result: change it only where it misreads the reference, never
to follow the library."""
import numpy as np

F32, F64 = np.float32, np.float64
DEFAULTS = dict(lidar_height=2.0, num_ring=20, num_sector=60, max_radius=80.0, num_candidates=3, search_ratio=0.1, dist_thres=0.3)
INT_MIN = -(1 << 31)


def params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return p


def _cell(v, n):
    """max(min(n, int(ceil(v))), 1) with x86's int conversion: NaN / out of range -> INT_MIN"""
    c = np.ceil(v)
    ok = (c >= -2147483648.0) & (c < 2147483648.0)
    i = np.where(ok, np.where(ok, c, 0.0).astype(np.int64), INT_MIN)
    return np.maximum(np.minimum(n, i), 1)


def polar(pts):
    """(azim_range float32, azim_angle float32) of :171-172"""
    x, y = pts[:, 0].astype(F32), pts[:, 1].astype(F32)
    deg = 180.0 / np.pi
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y)
        t = np.full(len(x), np.nan, F64)
        m = (x >= 0) & (y >= 0)
        t[m] = deg * np.arctan((y[m] / x[m]).astype(F64))
        m = (x < 0) & (y >= 0)
        t[m] = 180.0 - deg * np.arctan((y[m] / (-x[m])).astype(F64))
        m = (x < 0) & (y < 0)
        t[m] = 180.0 + deg * np.arctan((y[m] / x[m]).astype(F64))
        m = (x >= 0) & (y < 0)
        t[m] = 360.0 - deg * np.arctan(((-y[m]) / x[m]).astype(F64))
    return r, t.astype(F32)


def bins(pts, p):
    """(keep mask, ring index, sector index), both 1-based (:175-179); non-finite points are left out"""
    r, theta = polar(pts)
    keep = np.isfinite(pts[:, :3]).all(axis=1) & ~(r.astype(F64) > p["max_radius"])
    with np.errstate(all="ignore"):
        ring = _cell(r.astype(F64) / p["max_radius"] * p["num_ring"], p["num_ring"])
        sector = _cell(theta.astype(F64) / 360.0 * p["num_sector"], p["num_sector"])
    return keep, ring, sector


def heights(pts, p):
    return (pts[:, 2].astype(F64) + p["lidar_height"]).astype(F32).astype(F64)


def descriptor(pts, p):
    """makeScancontext :151-195"""
    keep, ring, sector = bins(pts, p)
    desc = np.full((p["num_ring"], p["num_sector"]), -1000.0)
    np.maximum.at(desc, (ring[keep] - 1, sector[keep] - 1), heights(pts, p)[keep])
    desc[desc == -1000.0] = 0.0
    return desc


def descriptors(scans, offsets, p):
    return np.stack([descriptor(scans[int(offsets[k]):int(offsets[k + 1])], p) for k in range(len(offsets) - 1)]) if len(offsets) > 1 \
        else np.zeros((0, p["num_ring"], p["num_sector"]))


def _seq_sum(a, axis):
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def ring_key(desc):
    return (_seq_sum(desc, 1) / desc.shape[1]).astype(F32)


def sector_key(desc):
    return _seq_sum(desc, 0) / desc.shape[0]


def align_norms(vk1, vk2):
    """||vkey1 - circshift(vkey2, s)|| for every shift s (:93-113)"""
    S = len(vk1)
    c = np.arange(S)
    J = (c[None, :] - c[:, None]) % S                   # [s, c] -> column of vk2 under column c
    d = vk1[None, :] - vk2[J]
    return np.sqrt(_seq_sum(d * d, 1))


def shift_distances(sc1, sc2):
    """distDirectSC(sc1, circshift(sc2, s)) for every shift s (:69-90)"""
    R, S = sc1.shape
    n1, n2 = np.sqrt(_seq_sum(sc1 * sc1, 0)), np.sqrt(_seq_sum(sc2 * sc2, 0))
    D = np.zeros((S, S))
    for r in range(R):
        D = D + sc1[r][:, None] * sc2[r][None, :]       # D[c, j] = col c of sc1 . col j of sc2
    c = np.arange(S)
    J = (c[None, :] - c[:, None]) % S
    valid = ~((n1[None, :] == 0) | (n2[J] == 0))
    with np.errstate(all="ignore"):
        sim = np.where(valid, D[c[None, :], J] / (n1[None, :] * n2[J]), 0.0)
        return 1.0 - _seq_sum(sim, 1) / valid.sum(axis=1)


def first_min(values, order, start=10000000.0):
    best, arg = start, 0
    for s in order:
        if values[s] < best:
            best, arg = values[s], s
    return best, int(arg)


def search_space(a0, S, ratio):
    radius = int(np.floor(0.5 * ratio * S + 0.5))       # round() of a non-negative value
    space = {a0}
    for ii in range(1, min(radius, S) + 1):
        space.add((a0 + ii + S) % S)
        space.add((a0 - ii + S) % S)
    return sorted(space)


def distance(sc1, sc2, ratio, details=False):
    """distanceBtnScanContext :116-148 -> (dist, shift)"""
    S = sc1.shape[1]
    norms = align_norms(sector_key(sc1), sector_key(sc2))
    _, a0 = first_min(norms, range(S))
    space = search_space(a0, S, ratio)
    d = shift_distances(sc1, sc2)
    best, arg = first_min(d, space)
    if details:
        return best, arg, np.sort(norms), np.sort(d[space])
    return best, arg


def key_distances(q, keys):
    """nanoflann L2_Adaptor::evalMetric in float between key q and every row of keys"""
    q, keys = q.astype(F32), keys.astype(F32)
    res = np.zeros(len(keys), F32)
    R, d = len(q), 0
    with np.errstate(all="ignore"):
        while d + 3 < R:
            d0, d1, d2, d3 = (q[d + k] - keys[:, d + k] for k in range(4))
            res = res + (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3)
            d += 4
        while d < R:
            d0 = q[d] - keys[:, d]
            res = res + d0 * d0
            d += 1
    return res


def detect(db, queries, p):
    """detectLoopClosureIDBetweenSession :263-324 for every query -> dict of arrays"""
    n, S = len(queries), p["num_sector"]
    out = dict(loop_id=np.full(n, -1, np.int32), nn_idx=np.zeros(n, np.int32), min_dist=np.full(n, 10000000.0), nn_align=np.zeros(n, np.int32),
               yaw_diff_rad=np.zeros(n, F32))
    K = len(db) if p["num_candidates"] == 0 else min(p["num_candidates"], len(db))
    keys = np.stack([ring_key(d) for d in db]) if len(db) else np.zeros((0, p["num_ring"]), F32)
    for i, q in enumerate(queries):
        if K:
            kd = key_distances(ring_key(q), keys)
            cand = np.lexsort((np.arange(len(db)), kd))[:K]         # ascending (distance, index)
            best, align, idx = 10000000.0, 0, 0
            for j in cand:
                d, s = distance(q, db[j], p["search_ratio"])
                if d < best:
                    best, align, idx = d, s, int(j)
            out["min_dist"][i], out["nn_align"][i], out["nn_idx"][i] = best, align, idx
            if best < p["dist_thres"]:
                out["loop_id"][i] = idx
        degrees = F32(out["nn_align"][i] * (360.0 / S))               # deg2rad takes a float (:17-20)
        out["yaw_diff_rad"][i] = F32(F64(degrees) * np.pi / 180.0)
    return out
