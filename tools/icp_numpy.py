"""Point-to-point ICP as include/ltm.h ("icp") states it, restated in numpy: what the tests hold ltm_icp_align against.  Written from the header
text; imports nothing of the library.  Brute-force float32 nearest neighbours (FLANN's L2_Simple, the first minimum wins a tie, which is the smaller
target index), two-pass demeaned moments in double, np.linalg.svd.

    r = align(target_xyz, source_xyz, init=None, max_corr_dist=150.0, max_iterations=100, transformation_epsilon=1e-6,
              euclidean_fitness_epsilon=1e-6, order=None)
    r: dict with T (4, 4), fitness, last_mse, converged, iterations, state, n_corr, trace (max_iterations, 2)

`order` (a permutation of the finite source points, or None) only changes the order in which the sums over the correspondences run; the fixture condition
of the tests is that this does not change the discrete part of the result."""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)


def _f32(a):
    """(n, 3) or (n, 4) points -> float32 xyz"""
    a = np.asarray(a, dtype=np.float32)
    if a.ndim != 2:
        a = a.reshape(-1, 3)
    return np.ascontiguousarray(a[:, :3])


def transform_to_float(T, src):
    """step 1: x' = ((T00 x + T01 y) + T02 z) + T03 in double, rounded to float"""
    p = src.astype(np.float64)
    out = np.empty((len(p), 3), np.float64)
    for r in range(3):
        out[:, r] = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]
    with np.errstate(over="ignore"):
        return out.astype(np.float32)


def nearest(queries, target):
    """(index, d2 float32) of the nearest target point of every query: ((dx*dx)+dy*dy)+dz*dz in float32, first minimum"""
    chunk = max(1, (1 << 22) // max(len(target), 1))      # queries per block of the distance matrix
    idx = np.empty(len(queries), np.int64)
    d2 = np.empty(len(queries), np.float32)
    tx, ty, tz = target[:, 0][None, :], target[:, 1][None, :], target[:, 2][None, :]
    for a in range(0, len(queries), chunk):
        q = queries[a:a + chunk]
        with np.errstate(over="ignore"):
            dx, dy, dz = q[:, 0:1] - tx, q[:, 1:2] - ty, q[:, 2:3] - tz
            d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        j = np.argmin(d, axis=1)      # the first occurrence of the minimum
        idx[a:a + chunk] = j
        d2[a:a + chunk] = d[np.arange(len(q)), j]
    return idx, d2


def rigid_transform(p, q):
    """step 5: Umeyama without scale, p -> q, all in double"""
    n = len(p)
    pm, qm = p.sum(axis=0) / n, q.sum(axis=0) / n
    H = (p - pm).T @ (q - qm) / n
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(V @ U.T) >= 0.0 else -1.0])
    R = V @ D @ U.T
    return R, qm - R @ pm


def align(target, source, init=None, max_corr_dist=150.0, max_iterations=100, transformation_epsilon=1e-6, euclidean_fitness_epsilon=1e-6, order=None):
    target, source = _f32(target), _f32(source)
    target = target[np.isfinite(target).all(axis=1)]
    source = source[np.isfinite(source).all(axis=1)]
    if order is not None:
        order = np.asarray(order)
        assert sorted(order.tolist()) == list(range(len(source))), "order must be a permutation of the finite source points"
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    T[3] = (0.0, 0.0, 0.0, 1.0)
    res = dict(T=T, fitness=DBL_MAX, last_mse=DBL_MAX, converged=0, iterations=0, state=0, n_corr=0,
               trace=np.full((max(max_iterations, 0), 2), np.nan))
    if len(source) == 0 or len(target) == 0 or max_iterations < 1:
        return res
    max2 = max_corr_dist * max_corr_dist
    prev = DBL_MAX
    it = 0
    while True:
        q = transform_to_float(T, source)
        ok = np.isfinite(q).all(axis=1)
        idx, d2 = nearest(q[ok], target)
        keep = d2.astype(np.float64) <= max2
        p, t, dk = q[ok][keep].astype(np.float64), target[idx[keep]].astype(np.float64), d2[keep].astype(np.float64)
        if order is not None:
            sel = np.argsort(np.argsort(order)[np.flatnonzero(ok)[keep]], kind="stable")      # the kept pairs in the order `order` visits their points
            p, t, dk = p[sel], t[sel], dk[sel]
        n = len(p)
        mse = float(np.add.reduce(dk) / n) if n else DBL_MAX
        res["n_corr"], res["last_mse"] = n, mse
        res["trace"][it] = (n, mse if n else np.nan)
        if n < 3:
            res["state"], res["converged"] = 0, 0
            break
        R, tr = rigid_transform(p, t)
        Ti = np.eye(4)
        Ti[:3, :3], Ti[:3, 3] = R, tr
        T = Ti @ T
        it += 1
        state = -1
        dm = abs(mse - prev)
        if it >= max_iterations:
            state = 1
        elif 0.5 * (np.trace(R) - 1.0) >= 1.0 - transformation_epsilon and float(tr @ tr) <= transformation_epsilon:
            state = 2
        elif dm < 1e-12:
            state = 3
        elif dm / prev < euclidean_fitness_epsilon:
            state = 4
        if state >= 0:
            res["state"], res["converged"] = state, 1
            break
        prev = mse
    res["T"], res["iterations"] = T, it
    q = transform_to_float(T, source)
    q = q[np.isfinite(q).all(axis=1)]
    if len(q):
        _, d2 = nearest(q, target)
        res["fitness"] = float(d2.astype(np.float64).sum() / len(q))
    return res
