"""include/ltm.h, section "planes", restated in numpy: RANSAC plane segmentation of one record of points, as this library takes PCL 1.10's
SACSegmentation::segment (SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE, SAC_RANSAC) to do.  Written from the header text, vectorised over points; every
decisive expression uses + - x in float64 in the header's order, numpy does not fuse them, so the device and this file agree by construction on hypotheses,
counts, the best hypothesis and -- given coefficients -- on labels.  The refinement goes through the same moment shape and the same Jacobi iteration in
Python floats.

    params(...)                              the parameters as a dict
    hypotheses(points, params)               idx [H, 3], N [H, 3], p0 [H, 3], T [H], valid [H]
    counts(points, hyps)                     uint32 [H]
    best(counts, valid)                      (found, h, consensus, n_valid)
    unrefined(hyps, h, params)               (coeff [4], point [3])
    refine(points, hyps, h, consensus, params, perm=None)   (coeff [4], point [3], refined)
    labels(points, coeff, point, thr)        uint8 [n]
    segment(points, params)                  everything, as a dict
"""
import math

import numpy as np

MAX_ITERATIONS = 4096
CHUNK, GROUP = 256, 64
_M32 = np.uint64(0xffffffff)


def params(distance_threshold, max_iterations=128, axis=None, eps_angle=0.0, seed=0, refine=True):
    ax = (0.0, 0.0, 0.0) if axis is None else tuple(float(v) for v in axis)
    assert len(ax) == 3 and 1 <= int(max_iterations) <= MAX_ITERATIONS and float(distance_threshold) > 0.0
    return dict(distance_threshold=float(distance_threshold), max_iterations=int(max_iterations), axis=ax, eps_angle=float(eps_angle), seed=int(seed),
                refine=bool(refine))


def mix(seed, h, j):
    """the 32-bit hash of (seed, h, j), vectorised over h"""
    h = np.asarray(h, dtype=np.uint64)
    x = (np.uint64(seed) + np.uint64(0x9E3779B9) * (np.uint64(3) * h + np.uint64(j) + np.uint64(1))) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    x ^= x >> np.uint64(16)
    return x


def _xyz(points):
    p = np.asarray(points, dtype=np.float32)
    return p.reshape(-1, p.shape[-1] if p.ndim == 2 else 4)[:, :3]


def _constraint(p):
    """(has_axis, constrained, c2)"""
    ax = p["axis"]
    has_axis = any(v != 0.0 for v in ax)
    constrained = has_axis and p["eps_angle"] < 1.5707963267948966
    c = math.cos(p["eps_angle"]) if constrained else 0.0
    return has_axis, constrained, c * c


def hypotheses(points, p):
    xyz = _xyz(points)
    n, H = len(xyz), p["max_iterations"]
    h = np.arange(H, dtype=np.uint64)
    idx = np.stack([(mix(p["seed"], h, j) * np.uint64(n)) >> np.uint64(32) for j in range(3)], axis=1).astype(np.int64)
    valid = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    N, p0, T = np.zeros((H, 3)), np.zeros((H, 3)), np.zeros(H)
    if n:
        fin = np.isfinite(xyz).all(axis=1)
        valid &= fin[idx].all(axis=1)
    else:
        valid[:] = False
    v = np.flatnonzero(valid)
    if len(v):
        q = xyz.astype(np.float64)
        a, b, c = q[idx[v, 0]], q[idx[v, 1]], q[idx[v, 2]]
        u, w = b - a, c - a
        Nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        Ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        Nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        with np.errstate(over="ignore", invalid="ignore"):
            n2 = (Nx * Nx + Ny * Ny) + Nz * Nz
            ok = (n2 > 0.0) & np.isfinite(n2)
            _, constrained, c2 = _constraint(p)
            if constrained:
                ax = p["axis"]
                dot = (Nx * ax[0] + Ny * ax[1]) + Nz * ax[2]
                aa = (ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]
                ok &= dot * dot >= (c2 * n2) * aa
            thr = p["distance_threshold"]
            Tv = (thr * thr) * n2
        valid[v] = ok
        g = v[ok]
        N[g] = np.stack([Nx, Ny, Nz], axis=1)[ok]
        p0[g] = a[ok]
        T[g] = Tv[ok]
    return dict(idx=idx, N=N, p0=p0, T=T, valid=valid.astype(np.uint8))


def _inlier_matrix(q, fin, N, p0, T):
    """[hypotheses, points] of the inlier test"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = q[None, :, 0] - p0[:, None, 0]
        dy = q[None, :, 1] - p0[:, None, 1]
        dz = q[None, :, 2] - p0[:, None, 2]
        s = (N[:, None, 0] * dx + N[:, None, 1] * dy) + N[:, None, 2] * dz
        return (s * s < T[:, None]) & fin[None, :]


def counts(points, hyps):
    xyz = _xyz(points)
    H = len(hyps["T"])
    out = np.zeros(H, dtype=np.uint32)
    if not len(xyz):
        return out
    fin = np.isfinite(xyz).all(axis=1)
    q = np.where(fin[:, None], xyz, np.float32(0)).astype(np.float64)
    v = np.flatnonzero(hyps["valid"])
    step = max(1, (1 << 21) // max(len(xyz), 1))
    for a in range(0, len(v), step):
        g = v[a:a + step]
        out[g] = _inlier_matrix(q, fin, hyps["N"][g], hyps["p0"][g], hyps["T"][g]).sum(axis=1)
    return out


def best(cnt, valid):
    """(found, h, consensus, n_valid): the valid hypothesis with the largest count, ties to the smaller h"""
    v = np.flatnonzero(valid)
    if not len(v):
        return 0, -1, 0, 0
    h = int(v[np.argmax(cnt[v])])      # argmax returns the first of equals
    return 1, h, int(cnt[h]), len(v)


def _coefficients(n, c0, p):
    nx, ny, nz = (float(v) for v in n)
    big = nx
    if abs(ny) > abs(big):
        big = ny
    if abs(nz) > abs(big):
        big = nz
    flip = big < 0.0
    if _constraint(p)[0]:
        ax = p["axis"]
        dot = (nx * ax[0] + ny * ax[1]) + nz * ax[2]
        if dot > 0.0:
            flip = False
        elif dot < 0.0:
            flip = True
    if flip:
        nx, ny, nz = -nx, -ny, -nz
    d = -((nx * float(c0[0]) + ny * float(c0[1])) + nz * float(c0[2]))
    return np.array([nx, ny, nz, d]), np.array([float(v) for v in c0])


def unrefined(hyps, h, p):
    N, p0 = hyps["N"][h], hyps["p0"][h]
    ln = math.sqrt((float(N[0]) * float(N[0]) + float(N[1]) * float(N[1])) + float(N[2]) * float(N[2]))
    return _coefficients((float(N[0]) / ln, float(N[1]) / ln, float(N[2]) / ln), p0, p)


def fixed_shape_sum(rows):
    """rows [n, k] summed in the shape of "clusters": chunks of 256 by a tree (128 apart first), the chunk sums 64 at a time by a tree, groups in order"""
    rows = np.asarray(rows, dtype=np.float64)
    n, k = rows.shape
    nc = -(-n // CHUNK)
    a = np.zeros((nc * CHUNK, k))
    a[:n] = rows
    a = a.reshape(nc, CHUNK, k)
    s = CHUNK // 2
    while s:
        a[:, :s] = a[:, :s] + a[:, s:2 * s]
        s //= 2
    sums = a[:, 0]
    ng = -(-nc // GROUP)
    b = np.zeros((ng * GROUP, k))
    b[:nc] = sums
    b = b.reshape(ng, GROUP, k)
    s = GROUP // 2
    while s:
        b[:, :s] = b[:, :s] + b[:, s:2 * s]
        s //= 2
    total = np.zeros(k)
    for g in range(ng):
        total = total + b[g, 0]
    return total


def smallest_axis(s, c, n):
    """ltm_covariance.h in Python floats: (unit normal with the canonical sign, eigenvalues by axis, axis of the smallest)"""
    inv = 1.0 / float(n)
    mx, my, mz = s[0] * inv, s[1] * inv, s[2] * inv
    A = [[0.0] * 3 for _ in range(3)]
    A[0][0] = c[0] * inv - mx * mx; A[0][1] = c[1] * inv - mx * my; A[0][2] = c[2] * inv - mx * mz
    A[1][1] = c[3] * inv - my * my; A[1][2] = c[4] * inv - my * mz; A[2][2] = c[5] * inv - mz * mz
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2]
    V = [[1.0 if r == k else 0.0 for k in range(3)] for r in range(3)]
    for _ in range(30):
        rotated = False
        for i in range(2):
            for j in range(i + 1, 3):
                apq = A[i][j]
                if apq == 0.0 or abs(apq) <= 1.0e-17 * math.sqrt(abs(A[i][i] * A[j][j])):
                    continue
                rotated = True
                theta = (A[j][j] - A[i][i]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(1.0 + theta * theta))
                cs = 1.0 / math.sqrt(1.0 + t * t)
                sn = cs * t
                l = 3 - i - j
                aii, ajj, ail, ajl = A[i][i], A[j][j], A[i][l], A[j][l]
                A[i][i] = aii - t * apq; A[j][j] = ajj + t * apq
                A[i][j] = A[j][i] = 0.0
                A[i][l] = A[l][i] = cs * ail - sn * ajl
                A[j][l] = A[l][j] = sn * ail + cs * ajl
                for k in range(3):
                    vi, vj = V[k][i], V[k][j]
                    V[k][i] = cs * vi - sn * vj; V[k][j] = sn * vi + cs * vj
        if not rotated:
            break
    e = 0
    if A[1][1] < A[e][e]:
        e = 1
    if A[2][2] < A[e][e]:
        e = 2
    lam = [A[0][0], A[1][1], A[2][2]]
    nx, ny, nz = V[0][e], V[1][e], V[2][e]
    ln = math.sqrt((nx * nx + ny * ny) + nz * nz)
    nx, ny, nz = nx / ln, ny / ln, nz / ln
    big = nx
    if abs(ny) > abs(big):
        big = ny
    if abs(nz) > abs(big):
        big = nz
    if big < 0.0:
        nx, ny, nz = -nx, -ny, -nz
    return (nx, ny, nz), lam, e


def moment_rows(points, hyps, h):
    """[n, 9]: d and the six products of every point of the record, zeros where the point is no inlier of hypothesis h"""
    xyz = _xyz(points)
    fin = np.isfinite(xyz).all(axis=1)
    q = np.where(fin[:, None], xyz, np.float32(0)).astype(np.float64)
    inl = _inlier_matrix(q, fin, hyps["N"][h:h + 1], hyps["p0"][h:h + 1], hyps["T"][h:h + 1])[0]
    d = q - hyps["p0"][h][None, :]
    rows = np.stack([d[:, 0], d[:, 1], d[:, 2], d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                     d[:, 2] * d[:, 2]], axis=1)
    rows[~inl] = 0.0
    return rows


def refine(points, hyps, h, consensus, p, perm=None):
    """(coeff, point, refined).  perm: sum the moment rows in that order instead of the record's (how much the order of summation moves the result)"""
    base = unrefined(hyps, h, p)
    if consensus < 3:
        return base[0], base[1], 0
    rows = moment_rows(points, hyps, h)
    if perm is not None:
        rows = rows[perm]
    m = fixed_shape_sum(rows)
    (nx, ny, nz), lam, e = smallest_axis([float(v) for v in m[:3]], [float(v) for v in m[3:]], consensus)
    second = min(lam[k] for k in range(3) if k != e)
    if not (second > lam[e]) or not all(math.isfinite(v) for v in (nx, ny, nz)):
        return base[0], base[1], 0
    p0 = hyps["p0"][h]
    c0 = [float(p0[k]) + float(m[k]) / float(consensus) for k in range(3)]
    coeff, point = _coefficients((nx, ny, nz), c0, p)
    return coeff, point, 1


def labels(points, coeff, point, thr):
    xyz = _xyz(points)
    if not len(xyz):
        return np.zeros(0, dtype=np.uint8)
    fin = np.isfinite(xyz).all(axis=1)
    q = np.where(fin[:, None], xyz, np.float32(0)).astype(np.float64)
    a, b, c = float(coeff[0]), float(coeff[1]), float(coeff[2])
    with np.errstate(invalid="ignore", over="ignore"):
        ex, ey, ez = q[:, 0] - float(point[0]), q[:, 1] - float(point[1]), q[:, 2] - float(point[2])
        v = np.abs((a * ex + b * ey) + c * ez)
        return ((v < float(thr)) & fin).astype(np.uint8)


def segment(points, p):
    hyps = hypotheses(points, p)
    cnt = counts(points, hyps)
    found, h, consensus, n_valid = best(cnt, hyps["valid"])
    n = len(_xyz(points))
    if not found:
        coeff, point, refined = np.full(4, np.nan), np.full(3, np.nan), 0
        lab = np.zeros(n, dtype=np.uint8)
    else:
        if p["refine"]:
            coeff, point, refined = refine(points, hyps, h, consensus, p)
        else:
            (coeff, point), refined = unrefined(hyps, h, p), 0
        lab = labels(points, coeff, point, p["distance_threshold"])
    return dict(hyps=hyps, counts=cnt, valid=hyps["valid"], found=found, best=h, consensus=consensus, n_valid=n_valid, n_inliers=int(lab.sum()),
                refined=refined, coeff=coeff, point=point, labels=lab)
