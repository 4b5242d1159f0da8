"""The loop submaps as include/ltm.h ("loop submaps") states them, restated in numpy float32 with one rounding per operation: what the tests hold
ltm_pose6d_to_affine3f and ltm_submaps_assemble (without the grid, leaf = 0) against.  Written from the header text; imports nothing of the library.

    A = pose6d_to_affine3f(xyzrpy, cos=np.cos, sin=np.sin)     (n, 6) float32 -> (n, 3, 4) float32
    pts, offsets = assemble(scans, offsets, keys, search_num, affines=None)

cos / sin may be replaced (the tests pass the C library's cosf / sinf so that only the products and sums are under test)."""
import numpy as np

F = np.float32


def pose6d_to_affine3f(xyzrpy, cos=np.cos, sin=np.sin):
    """pcl::getTransformation(x, y, z, roll, pitch, yaw) in float (PCL 1.10 common/impl/eigen.hpp, as understood)"""
    p = np.ascontiguousarray(xyzrpy, dtype=F).reshape(-1, 6)
    x, y, z, roll, pitch, yaw = (p[:, i] for i in range(6))
    A, B = cos(yaw).astype(F), sin(yaw).astype(F)
    C, D = cos(pitch).astype(F), sin(pitch).astype(F)
    E, Fs = cos(roll).astype(F), sin(roll).astype(F)
    DE, DF = D * E, D * Fs
    out = np.empty((len(p), 3, 4), F)
    out[:, 0, 0] = A * C; out[:, 0, 1] = A * DF - B * E; out[:, 0, 2] = B * Fs + A * DE; out[:, 0, 3] = x
    out[:, 1, 0] = B * C; out[:, 1, 1] = A * E + B * DF; out[:, 1, 2] = B * DE - A * Fs; out[:, 1, 3] = y
    out[:, 2, 0] = -D;    out[:, 2, 1] = C * Fs;         out[:, 2, 2] = C * E;           out[:, 2, 3] = z
    return out


def transform(pts, affine):
    """transformPointCloud (utility.cpp:97-99): ((t00*x + t01*y) + t02*z) + t03 in float32, left to right; the intensity is copied"""
    pts = np.ascontiguousarray(pts, dtype=F).reshape(-1, 4)
    t = np.asarray(affine, dtype=F).reshape(3, 4)
    out = np.empty_like(pts)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            out[:, r] = ((t[r, 0] * pts[:, 0] + t[r, 1] * pts[:, 1]) + t[r, 2] * pts[:, 2]) + t[r, 3]
    out[:, 3] = pts[:, 3]
    return out


IDENTITY = np.eye(4, dtype=F)[:3]


def assemble(scans, offsets, keys, search_num, affines=None):
    """window w = keyframes keys[w] - search_num ... keys[w] + search_num inside [0, n_kf), ascending, each moved by its affine (None: the identity,
    still multiplied through).  Returns (points (n, 4) float32, offsets (n_windows + 1) uint64)."""
    scans = np.ascontiguousarray(scans, dtype=F).reshape(-1, 4)
    offsets = np.asarray(offsets, dtype=np.int64)
    n_kf = len(offsets) - 1
    parts, out_off = [], [0]
    for key in np.asarray(keys, dtype=np.int64):
        n = 0
        for k in range(max(int(key) - search_num, 0), min(int(key) + search_num, n_kf - 1) + 1):
            part = transform(scans[offsets[k]:offsets[k + 1]], IDENTITY if affines is None else affines[k])
            parts.append(part)
            n += len(part)
        out_off.append(out_off[-1] + n)
    pts = np.concatenate(parts) if parts else np.empty((0, 4), F)
    return pts, np.asarray(out_off, dtype=np.uint64)
