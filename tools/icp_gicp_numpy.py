"""Generalized (plane-to-plane) ICP as include/ltm.h ("icp, generalized") states it, restated in numpy: what the tests hold ltm_icp_align_gicp against.
Written from the header text; imports nothing of the library.  Steps 1-3, the stop tests, mse, fitness and the trace are those of tools/icp_numpy.py, the
pivot test and the rotation of the step those of tools/icp_plane_numpy.py (their helpers are used).  Per correspondence: m = R_T n_a,
S = 2I - (1 - epsilon)(n_b n_b^T + m m^T), M = adj(S) / det(S) from the header's six cofactors, A = [-[p]x, I], d = q - p about the corner of the target's
bounding box; the 6 x 6 system sum A^T M A x = sum A^T M d is solved by np.linalg.solve after the header's pivot test.

    r = align(target_xyz, target_normals, source_xyz, source_normals, init=None, gicp_epsilon=1e-3, max_corr_dist=150.0, max_iterations=100,
              transformation_epsilon=1e-6, euclidean_fitness_epsilon=1e-6, order=None, on_iteration=None)
    normals: (n, 3 or 4) float32 in the order of their cloud (tools/normals_numpy.py: estimate(...)["normals"])
    r: dict with T (4, 4), fitness, last_mse, converged, iterations, state (5: degenerate system), n_corr, trace (max_iterations, 2)

`order` (a permutation of the finite source points, or None) only changes the order in which the sums over the correspondences run.  on_iteration, if
given, is called with (indices of the kept finite source points, indices of their finite target points) of every iteration."""
import numpy as np

from tools.icp_numpy import DBL_MAX, _f32, nearest, transform_to_float
from tools.icp_plane_numpy import rotation, well_determined


def weights(nb, m, epsilon):
    """(n, 3, 3) M of the header's step 6 from target normals nb and turned source normals m (doubles): six cofactors and one determinant"""
    w = 1.0 - epsilon
    bx, by, bz = nb[:, 0], nb[:, 1], nb[:, 2]
    mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
    s00, s01, s02 = 2.0 - w * (bx * bx + mx * mx), -w * (bx * by + mx * my), -w * (bx * bz + mx * mz)
    s11, s12, s22 = 2.0 - w * (by * by + my * my), -w * (by * bz + my * mz), 2.0 - w * (bz * bz + mz * mz)
    c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
    c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 1.0 / ((s00 * c00 + s01 * c01) + s02 * c02)
        return np.stack([np.stack([c00 * r, c01 * r, c02 * r], 1), np.stack([c01 * r, c11 * r, c12 * r], 1), np.stack([c02 * r, c12 * r, c22 * r], 1)], 1)


def jacobians(p):
    """(n, 3, 6) A = [-[p]x, I]: A x = omega x p + t' for x = (omega, t')"""
    n = len(p)
    A = np.zeros((n, 3, 6))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    A[:, 0, 1], A[:, 0, 2] = z, -y
    A[:, 1, 0], A[:, 1, 2] = -z, x
    A[:, 2, 0], A[:, 2, 1] = y, -x
    A[:, 0, 3] = A[:, 1, 4] = A[:, 2, 5] = 1.0
    return A


def normal_equations(p, q, M):
    """(sum A^T M A, sum A^T M d) of correspondences p -> q (already about o), summed in the order given"""
    A, d = jacobians(p), q - p
    MA = M @ A
    H = np.add.reduce(np.swapaxes(A, 1, 2) @ MA, axis=0)
    g = np.add.reduce(np.einsum("nij,ni->nj", MA, d), axis=0)
    return H, g


def gicp_step(p, q, nb, m, o, epsilon):
    """(R, t) of one step from queries p, target points q, target normals nb and turned source normals m (doubles), or None when degenerate"""
    H, g = normal_equations(p - o, q - o, weights(nb, m, epsilon))
    if not np.isfinite(H).all() or not well_determined(H):
        return None
    x = np.linalg.solve(H, g)
    if not np.isfinite(x).all():
        return None
    R = rotation(x[0], x[1], x[2])
    return R, x[3:] + o - R @ o


def align(target, target_normals, source, source_normals, init=None, gicp_epsilon=1e-3, max_corr_dist=150.0, max_iterations=100,
          transformation_epsilon=1e-6, euclidean_fitness_epsilon=1e-6, order=None, on_iteration=None):
    assert np.isfinite(gicp_epsilon) and 0.0 < gicp_epsilon <= 1.0, "gicp_epsilon must be in (0, 1]"
    target, source = _f32(target), _f32(source)
    tn, sn = _f32(target_normals), _f32(source_normals)
    assert len(tn) == len(target) and len(sn) == len(source), "one normal per point"
    fin = np.isfinite(target).all(axis=1)
    target, tn = target[fin], tn[fin]
    fin = np.isfinite(source).all(axis=1)
    source, sn = source[fin], sn[fin]
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
    t_has, s_has = np.isfinite(tn).all(axis=1), np.isfinite(sn).all(axis=1)
    max2 = max_corr_dist * max_corr_dist
    prev = DBL_MAX
    it = 0
    while True:
        q = transform_to_float(T, source)
        ok = np.isfinite(q).all(axis=1)
        idx, d2 = nearest(q[ok], target)
        at = np.flatnonzero(ok)
        keep = (d2.astype(np.float64) <= max2) & t_has[idx] & s_has[at]
        at, idx, dk = at[keep], idx[keep], d2[keep].astype(np.float64)
        if order is not None:
            sel = np.argsort(np.argsort(order)[at], kind="stable")
            at, idx, dk = at[sel], idx[sel], dk[sel]
        if on_iteration is not None:
            on_iteration(at, idx)
        n = len(at)
        mse = float(np.add.reduce(dk) / n) if n else DBL_MAX
        res["n_corr"], res["last_mse"] = n, mse
        res["trace"][it] = (n, mse if n else np.nan)
        if n < 3:
            res["state"], res["converged"] = 0, 0
            break
        a = sn[at].astype(np.float64)
        m = np.stack([(T[r, 0] * a[:, 0] + T[r, 1] * a[:, 1]) + T[r, 2] * a[:, 2] for r in range(3)], 1)
        step = gicp_step(q[at].astype(np.float64), target[idx].astype(np.float64), tn[idx].astype(np.float64), m, o, gicp_epsilon)
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
