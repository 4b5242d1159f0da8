"""Point-to-plane ICP as include/ltm.h ("icp, point-to-plane") states it, restated in numpy: what the tests hold ltm_icp_align_plane against.  Written
from the header text; imports nothing of the library.  Steps 1-3, the stop tests, mse, fitness and the trace are those of tools/icp_numpy.py (whose helpers
are used); the estimate is the 6 x 6 linear system of the correspondences' rows [p x n, n], right side n . (q - p), about the corner of the target's
bounding box, solved by np.linalg.solve after the header's pivot test.

    r = align(target_xyz, normals, source_xyz, init=None, max_corr_dist=150.0, max_iterations=100, transformation_epsilon=1e-6,
              euclidean_fitness_epsilon=1e-6, order=None)
    normals: (n_target, 3 or 4) float32 in the target's order (tools/normals_numpy.py: estimate(...)["normals"])
    r: dict with T (4, 4), fitness, last_mse, converged, iterations, state (5: degenerate system), n_corr, trace (max_iterations, 2)

`order` (a permutation of the finite source points, or None) only changes the order in which the sums over the correspondences run."""
import numpy as np

from tools.icp_numpy import DBL_MAX, _f32, nearest, transform_to_float


def well_determined(ata):
    """the header's test: Cholesky without pivoting, every diagonal entry positive and every pivot d_j > 1e-12 (A^T A)_jj"""
    L = np.zeros((6, 6))
    for j in range(6):
        ajj = ata[j, j]
        d = ajj - float(L[j, :j] @ L[j, :j])
        if not ajj > 0.0 or not d > 1e-12 * ajj:
            return False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (ata[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    return True


def rotation(alpha, beta, gamma):
    """R = Rz(gamma) Ry(beta) Rx(alpha), entry by entry"""
    sa, ca, sb, cb, sg, cg = np.sin(alpha), np.cos(alpha), np.sin(beta), np.cos(beta), np.sin(gamma), np.cos(gamma)
    return np.array([[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca],
                     [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca],
                     [-sb, cb * sa, cb * ca]])


def plane_step(p, q, n, o):
    """(R, t) of one step from queries p, target points q and normals n (doubles), or None when the system is degenerate"""
    p, q = p - o, q - o
    a = np.concatenate([np.cross(p, n), n], axis=1)
    b = (n * (q - p)).sum(axis=1)
    ata, atb = a.T @ a, a.T @ b
    if not well_determined(ata):
        return None
    x = np.linalg.solve(ata, atb)
    if not np.isfinite(x).all():
        return None
    R = rotation(x[0], x[1], x[2])
    return R, x[3:] + o - R @ o


def align(target, normals, source, init=None, max_corr_dist=150.0, max_iterations=100, transformation_epsilon=1e-6, euclidean_fitness_epsilon=1e-6,
          order=None):
    target, source = _f32(target), _f32(source)
    normals = _f32(normals)
    assert len(normals) == len(target), "one normal per target point"
    fin = np.isfinite(target).all(axis=1)
    target, normals = target[fin], normals[fin]
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
    o = target.min(axis=0).astype(np.float64)      # the corner of the target's bounding box
    has_normal = np.isfinite(normals).all(axis=1)
    max2 = max_corr_dist * max_corr_dist
    prev = DBL_MAX
    it = 0
    while True:
        q = transform_to_float(T, source)
        ok = np.isfinite(q).all(axis=1)
        idx, d2 = nearest(q[ok], target)
        keep = (d2.astype(np.float64) <= max2) & has_normal[idx]
        p, t, nn, dk = q[ok][keep].astype(np.float64), target[idx[keep]].astype(np.float64), normals[idx[keep]].astype(np.float64), d2[keep].astype(np.float64)
        if order is not None:
            sel = np.argsort(np.argsort(order)[np.flatnonzero(ok)[keep]], kind="stable")
            p, t, nn, dk = p[sel], t[sel], nn[sel], dk[sel]
        n = len(p)
        mse = float(np.add.reduce(dk) / n) if n else DBL_MAX
        res["n_corr"], res["last_mse"] = n, mse
        res["trace"][it] = (n, mse if n else np.nan)
        if n < 3:
            res["state"], res["converged"] = 0, 0
            break
        step = plane_step(p, t, nn, o)
        if step is None:
            res["state"], res["converged"] = 5, 0
            break
        R, tr = step
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
