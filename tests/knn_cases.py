"""TEST INFRASTRUCTURE: seeded edge cases of the kNN change detection (ltm_knn_partition / ltm_knn_split_cloud), each built to reach one branch
of lt-mapper_amd/csrc/ltm_api_knn.cpp / ltm_k_knn.hip that realistic clouds do not reach.  Plain functions, no fixtures.

Every builder returns a list of (label, (target, scans, offsets, poses, inv, k, thr)): target (Mt, 4) float32 in the global frame, scans (P, 4)
float32 in the keyframes' local frames, offsets (n_kf + 1) uint64, poses / inv (n_kf, 16) float64 row-major.  tests/test_knn_cases_cpu.py shows on
the host that the cases mean something (two independent references agree, both classes are populated, the branch is reached);
tests/test_gpu_knn_edges.py runs them on the device.  Expected values come from the oracle's brute-force search and are computed once per
process (expected())."""
import functools
import math

import numpy as np

F32 = np.float32
I4 = np.eye(4)

# keyframe sub-ranges of the `ragged_ranges` case (sizes RAGGED_SIZES): empty ranges, empty keyframes at either end, one-point keyframes
RAGGED_SIZES = [0, 300, 0, 1, 257, 0, 900]
RAGGED_RANGES = [(0, 0), (1, 1), (0, 7), (1, 3), (2, 5), (6, 7), (3, 7)]
# a LiDAR -> base extrinsic that is not the identity (the B2L_IDENTITY = false kernels)
L2B = np.array([[0.0, -1.0, 0.0, 0.31], [1.0, 0.0, 0.0, -0.12], [0.0, 0.0, 1.0, 0.45], [0.0, 0.0, 0.0, 1.0]])

DIRS26 = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=np.float64)
UNIT26 = DIRS26 / np.linalg.norm(DIRS26, axis=1, keepdims=True)
STRADDLE_F = (0.98, 1.0 - 1e-5, 1.0, 1.0 + 1e-5, 1.02)


def _orc():
    from oracle import oracle_py
    oracle_py.lib()
    return oracle_py


def _p4(xyz, seed=0):
    """(n, 3) -> (n, 4) float32 with a seeded intensity column (it must travel through the partition untouched)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    out = np.empty((xyz.shape[0], 4), F32)
    out[:, :3] = xyz
    out[:, 3] = np.random.default_rng(1000 + seed).uniform(0, 255, xyz.shape[0])
    return out


def _pose(rng, t_scale=30.0):
    yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    T = np.eye(4)
    T[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T[:3, 3] = rng.uniform(-t_scale, t_scale, 3)
    return T


def _inv(poses):
    return _orc().inverse_poses(np.asarray(poses, dtype=np.float64).reshape(-1, 16))


def _identity_kf(queries, n_kf=1):
    """queries already in the global frame, cut into n_kf keyframes of identity pose (global point == scan point, bit for bit)"""
    q = np.ascontiguousarray(queries, dtype=F32).reshape(-1, 4)
    off = np.array([(len(q) * j) // n_kf for j in range(n_kf + 1)], dtype=np.uint64)
    poses = np.tile(np.eye(4).reshape(1, 16), (n_kf, 1))
    return q, off, poses, poses.copy()


def _to_local(global_q, sizes, poses, b2l=I4):
    """scan points whose global-frame image (pose * b2l * p, as the kNN stage moves them: quirk Q7) lands near `global_q` (up to float rounding)"""
    g = np.asarray(global_q, dtype=np.float64).reshape(-1, 4)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    assert int(off[-1]) == len(g)
    out = np.empty((len(g), 4), F32)
    for kf in range(len(sizes)):
        a, b = int(off[kf]), int(off[kf + 1])
        M = np.linalg.inv(np.asarray(poses[kf]).reshape(4, 4) @ np.asarray(b2l, dtype=np.float64))
        out[a:b, :3] = g[a:b, :3] @ M[:3, :3].T + M[:3, 3]
        out[a:b, 3] = g[a:b, 3]
    return out, off


def _case(target, scans, offsets, poses, inv, k, thr):
    return (np.ascontiguousarray(target, dtype=F32).reshape(-1, 4), np.ascontiguousarray(scans, dtype=F32).reshape(-1, 4),
            np.ascontiguousarray(offsets, dtype=np.uint64), np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16),
            np.ascontiguousarray(inv, dtype=np.float64).reshape(-1, 16), int(k), float(F32(thr)))


# ------------------------------------------------------------------------------------------------- the grid frame of KnnIndex::build, restated
def grid_frame(target, k, thr):
    """(cell, (nx, ny, nz), origin) as KnnIndex::build derives them for a target of more than 64 points"""
    t = np.asarray(target, dtype=F32).reshape(-1, 4)
    mn, mx = t[:, :3].min(0).astype(np.float64), t[:, :3].max(0).astype(np.float64)
    cell = math.sqrt(float(k) * float(F32(thr))) * (1.0 + 1e-3)
    ext = max(float((mx - mn).max()), 1e-3)
    cell = max(cell, ext / 1.0e6)
    origin = mn - cell
    n = tuple(int(math.floor((mx[d] - origin[d]) * (1.0 / cell))) + 2 for d in range(3))
    return cell, n, origin


def cells_of(points, cell, origin):
    p = np.asarray(points, dtype=F32).reshape(-1, 4)[:, :3].astype(np.float64)
    return np.floor((p - origin) * (1.0 / cell)).astype(np.int64)


def queue_bits(target, k, thr, n_queries):
    """(bits of the largest cell id, bits of the largest query index): the sorted phase-2 queue needs their sum <= 64"""
    _, n, _ = grid_frame(target, k, thr)
    b = 1
    while b < 64 and (1 << b) < n[0] * n[1] * n[2]:
        b += 1
    i = 1
    while i < 63 and (1 << i) < n_queries:
        i += 1
    return b, i


# ------------------------------------------------------------------------------------------------- cases
def straddle():
    """a jittered lattice of 12^3 sites at 0.75 m pitch.  k = 1, thr = 0.0625: every site gets one of the 26 directions and a query at
    f * sqrt(thr) along it for five f around 1, plus the float neighbours of the f = 1 query; the six extreme sites of the target's box get all
    26 directions and f = 1.5 on top (rim cells, just outside the grid).  k = 2, 3, 4, 6 (thr = 0.0625 / k, the same cell): k - 1 coincident points
    at the site and one at f * 0.25 m, queried from the site and its float neighbours, so that the k-th d2 sits around k * thr"""
    rng = np.random.default_rng(101)
    ijk = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 3)
    sites = (ijk * 0.75 + rng.uniform(-0.125, 0.125, ijk.shape)).astype(F32).astype(np.float64)      # the jitter spans one cell: every phase occurs
    n = len(sites)
    r = 0.25
    out = []
    # k = 1
    q = []
    d_of_site = np.arange(n) % 26
    for f in STRADDLE_F:
        q.append((sites + UNIT26[d_of_site] * (f * r)).astype(F32))
    q1 = q[2]
    q += [np.nextafter(q1, F32(np.inf)), np.nextafter(q1, F32(-np.inf))]
    extreme = sorted({int(sites[:, d].argmin()) for d in range(3)} | {int(sites[:, d].argmax()) for d in range(3)})
    for s in extreme:
        for f in STRADDLE_F + (1.5,):
            q.append((sites[s] + UNIT26 * (f * r)).astype(F32))
    q = _p4(np.concatenate(q), 1)
    out.append(("straddle-k1", _case(_p4(sites, 2), *_identity_kf(q, 3), 1, 0.0625)))
    # k >= 2
    for k in (2, 3, 4, 6):
        f_of_site = np.array(STRADDLE_F)[(np.arange(n) // 26) % 5]
        probe = sites + UNIT26[d_of_site] * (f_of_site * r)[:, None]
        target = np.concatenate([np.repeat(sites, k - 1, axis=0), probe])
        target = target[np.random.default_rng(102 + k).permutation(len(target))]
        s32 = sites.astype(F32)
        at_one = f_of_site == 1.0
        q = np.concatenate([s32, np.nextafter(s32[at_one], F32(np.inf)), np.nextafter(s32[at_one], F32(-np.inf)),
                            (sites + UNIT26[(d_of_site + 13) % 26] * 0.3).astype(F32)[::7]])      # the last ones: nothing near, all 27 cells walked
        out.append((f"straddle-k{k}", _case(_p4(target, 3), *_identity_kf(_p4(q, 4), 2), k, F32(0.0625) / F32(k))))
    return out


def exact_threshold():
    """one query at the origin, neighbours at distances whose float arithmetic is exact.  Every variant once bare (brute force inside the
    kernel) and once with 500 far points added (the hash grid).  EXACT_THRESHOLD_EXPECT holds the known answers of the bare variants"""
    lo = float(np.nextafter(F32(0.25), F32(0)))
    far = (np.random.default_rng(9).normal(0, 50.0, (500, 3)) + 100.0)
    far = far[np.linalg.norm(far, axis=1) > 20.0]
    variants = [
        ("d2-eq-thr-k1", [[0.25, 0, 0]], 1, 0.0625),                       # d2 == thr: strict <, "diff"
        ("d2-below-thr-k1", [[lo, 0, 0]], 1, 0.0625),
        ("mean-eq-thr-k2", [[0.25, 0, 0], [0, 0.25, 0]], 2, 0.0625),
        ("mean-below-thr-k2", [[lo, 0, 0], [0, lo, 0]], 2, 0.0625),
        ("kat-0.1-0.1-thr0.01", [[0.1, 0, 0], [0, 0.1, 0], [3, 3, 3]], 2, 0.01),
        ("kat-0.1-0.1-thr0.0101", [[0.1, 0, 0], [0, 0.1, 0], [3, 3, 3]], 2, 0.0101),
        ("kat-0.1-0.1-thr0.0099", [[0.1, 0, 0], [0, 0.1, 0], [3, 3, 3]], 2, 0.0099),
        ("k3-one-in-reach-coexist", [[0.25, 0, 0]], 3, 0.03),             # k clamped to 1, divisor 3: 0.0625 / 3 < 0.03
        ("k3-one-in-reach-diff", [[0.25, 0, 0]], 3, 0.02),
        ("duplicate-of-the-query-k2", [[0, 0, 0], [0, 0, 0], [1, 1, 1]], 2, 1e-6),      # d2 == 0 twice
    ]
    q = np.zeros((1, 4), F32)
    out = []
    for name, t, k, thr in variants:
        out.append((f"exact-{name}-bare", _case(_p4(t, 5), *_identity_kf(q), k, thr)))
        out.append((f"exact-{name}-grid", _case(_p4(np.concatenate([np.asarray(t, dtype=np.float64), far]), 5), *_identity_kf(q), k, thr)))
    return out


EXACT_THRESHOLD_EXPECT = {"exact-d2-eq-thr-k1-bare": 0, "exact-d2-below-thr-k1-bare": 1, "exact-mean-eq-thr-k2-bare": 0, "exact-mean-below-thr-k2-bare": 1,
                          "exact-kat-0.1-0.1-thr0.01-bare": 0, "exact-kat-0.1-0.1-thr0.0101-bare": 1, "exact-kat-0.1-0.1-thr0.0099-bare": 0,
                          "exact-k3-one-in-reach-coexist-bare": 1, "exact-k3-one-in-reach-diff-bare": 0, "exact-duplicate-of-the-query-k2-bare": 1,
                          # with the far points added k is no longer clamped: the 2nd and 3rd neighbours are tens of metres away
                          "exact-k3-one-in-reach-coexist-grid": 0, "exact-duplicate-of-the-query-k2-grid": 1, "exact-d2-eq-thr-k1-grid": 0,
                          "exact-d2-below-thr-k1-grid": 1, "exact-mean-eq-thr-k2-grid": 0, "exact-mean-below-thr-k2-grid": 1}


def _cube(seed, n=5000, side=200.0):
    return np.random.default_rng(seed).uniform(0.0, side, (n, 3)).astype(F32)


def unsorted_queue():
    """5000 points in a 200 m cube, k = 1, thr = 1e-6: ~2 * 10^5 cells per axis, 53 key bits + 12 index bits > 64, so phase 2 keeps its
    queue in scan order and finds every query's keyframe again (three keyframes, three poses)"""
    rng = np.random.default_rng(201)
    t = _cube(200)
    d = rng.normal(size=(4096, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    step = np.where(np.arange(4096) % 2 == 1, 0.3e-3, 3.0e-3)
    gq = np.concatenate([t[:4096].astype(np.float64) + d * step[:, None], np.zeros((4096, 1))], axis=1)
    gq[:, 3] = rng.uniform(0, 255, 4096)
    poses = [_pose(rng, 5.0) for _ in range(3)]
    scans, off = _to_local(gq, [1500, 1096, 1500], poses)
    poses = np.array(poses).reshape(3, 16)
    return [("unsorted_queue", _case(_p4(t, 6), scans, off, poses, _inv(poses), 1, 1e-6))]


def clamped_cell():
    """the same cube, k = 1, thr = 1e-9: sqrt(k thr) is below extent / 1e6, the cell edge is clamped, 10^6 cells per axis, 60-bit keys.
    Queries: target points moved by 1 ulp (odd index) or 40 ulp (even index) on every axis; identity poses keep them bit for bit"""
    t = _cube(200)
    q = t[:4096].copy()
    for _ in range(40):
        q[0::2] = np.nextafter(q[0::2], F32(np.inf))
    q[1::2] = np.nextafter(q[1::2], F32(np.inf))
    return [("clamped_cell", _case(_p4(t, 6), *_identity_kf(_p4(q, 7), 2), 1, 1e-9))]


def crowded_and_thin_cells():
    """k = 2 and 4, thr = 0.01: sites 1.5 m apart holding 1, k - 1, k, 9, 10 and 200 points inside a ball of 2 cm (every third of them an exact
    duplicate of another): cells with fewer than k points, with exactly the nine a bucket holds, with more (the evenly-spread sample), d2 == 0"""
    out = []
    for k in (2, 4):
        rng = np.random.default_rng(300 + k)
        ijk = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(6), indexing="ij"), -1).reshape(-1, 3)
        sites = ijk * 1.5 + rng.uniform(-0.2, 0.2, ijk.shape)
        counts = np.array([1, k - 1, k, 9, 10, 200])[np.arange(len(sites)) % 6]
        tgt, qry = [], []
        for s, c in zip(sites, counts):
            v = rng.normal(size=(c, 3))
            v *= (0.02 * rng.uniform(0, 1, (c, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
            p = (s + v).astype(F32)
            p[2::3] = p[1::3][:len(p[2::3])]      # exact duplicates
            tgt.append(p)
            u = rng.normal(size=(5, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            qry.append(np.concatenate([p[:1], s[None].astype(F32), (s + u * np.array([0.04, 0.08, 0.1, 0.15, 0.3])[:, None]).astype(F32)]))
        tgt = np.concatenate(tgt)
        tgt = tgt[rng.permutation(len(tgt))]
        out.append((f"crowded_and_thin_cells-k{k}", _case(_p4(tgt, 8), *_identity_kf(_p4(np.concatenate(qry), 9), 2), k, 0.01)))
    return out


def bucketless():
    """8192 sites more than 1 m apart, two identical points each, queried at the sites (k = 2, thr = 0.01): every occupied cell holds one site,
    every query whose cell has a bucket is decided by phase 1, so the undecided count is the number of cells that lost both places"""
    rng = np.random.default_rng(401)
    ijk = np.stack(np.meshgrid(np.arange(21), np.arange(21), np.arange(19), indexing="ij"), -1).reshape(-1, 3)
    sites = (ijk[rng.permutation(len(ijk))[:8192]] * 1.3 + rng.uniform(-0.1, 0.1, (8192, 3))).astype(F32)
    tgt = np.repeat(sites, 2, axis=0)
    tgt = tgt[rng.permutation(len(tgt))]
    return [("bucketless", _case(_p4(tgt, 10), *_identity_kf(_p4(sites, 11), 2), 2, 0.01))]


SMALL_MT = (1, 2, 3, 4, 5, 63, 64, 65, 66)
SMALL_K = (1, 2, 3, 4, 5, 16)


def small_targets():
    """Mt around the 64-point boundary between brute force inside the kernel and the hash grid, k from 1 to 16 (k > Mt included: k is clamped, the
    divisor is not; KT = 0 where Mt < k <= 4).  500 queries each; thr is the median of the queries' mean squared distance (numpy, float64), so
    both classes are populated"""
    out = []
    for Mt in SMALL_MT:
        rng = np.random.default_rng(500 + Mt)
        t = rng.uniform(0, 1.0, (Mt, 3)).astype(F32)
        d = rng.normal(size=(500, 3))
        d *= rng.uniform(0, 0.6, (500, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
        q = (t[rng.integers(0, Mt, 500)] + d).astype(F32)
        d2 = np.sort(((q[:, None, :].astype(np.float64) - t[None].astype(np.float64)) ** 2).sum(-1), axis=1)
        poses = np.array([_pose(rng, 2.0) for _ in range(2)])
        scans, off = _to_local(np.concatenate([q, np.zeros((500, 1), F32)], axis=1), [250, 250], poses)
        scans[:, 3] = rng.uniform(0, 255, 500)
        for k in SMALL_K:
            thr = float(np.median(d2[:, :min(k, Mt)].sum(1) / k))
            out.append((f"small_targets-Mt{Mt}-k{k}", _case(_p4(t, 12), scans, off, poses.reshape(2, 16), _inv(poses), k, thr)))
    return out


@functools.lru_cache(maxsize=None)
def small_pair_target():
    """the map of the suite's `small_pair` query session (0.05 m grid), and one thinned keyframe of that session with its pose: most of its points
    have their own voxel's centroid and a neighbour's within reach, so both classes are populated"""
    from tools import synth
    orc = _orc()
    Q = synth.to_numpy(synth.make_session(2, 6, "small"))
    target = orc.voxel_centroid(orc.merge_to_global(Q["scans"], Q["offsets"], Q["poses"], I4), 0.05)
    a, b = int(Q["offsets"][2]), int(Q["offsets"][3])
    return target, np.ascontiguousarray(Q["scans"][a:b][::16]), np.asarray(Q["poses"], dtype=np.float64).reshape(-1, 16)[2].reshape(4, 4)


def far_and_outside():
    """the small_pair map; one keyframe posed (a) inside the map, (b) half outside its box, (c) 10 km away (the sentinel cell -2); and (d) map
    and pose moved to coordinates of 1e5 m, where floats are 8 mm apart"""
    target, scan, pose = small_pair_target()
    mn, mx = target[:, :3].min(0), target[:, :3].max(0)
    pb, pc = pose.copy(), pose.copy()
    pb[0, 3] = float(mx[0])              # the sensor on the box's +x face: half of the scan beyond it
    pc[:3, 3] += 1.0e4
    poses = np.array([pose, pb, pc]).reshape(3, 16)
    scans = np.concatenate([scan] * 3)
    off = np.array([0, len(scan), 2 * len(scan), 3 * len(scan)], dtype=np.uint64)
    out = [("far_and_outside-abc", _case(target, scans, off, poses, _inv(poses), 2, 0.01))]
    shift = np.array([1.0e5, -1.0e5, 0.0])
    t2 = target.copy()
    t2[:, :3] = (target[:, :3].astype(np.float64) + shift).astype(F32)
    pd = pose.copy()
    pd[:3, 3] += shift
    pd = pd.reshape(1, 16)
    out.append(("far_and_outside-d", _case(t2, scan, np.array([0, len(scan)], dtype=np.uint64), pd, _inv(pd), 2, 0.01)))
    return out


def _sites_target(rng, n_sites, per_site, spread=30.0):
    sites = rng.uniform(0, spread, (n_sites, 3))
    t = np.repeat(sites, per_site, axis=0) + rng.normal(0, 0.01, (n_sites * per_site, 3))
    return sites, t.astype(F32)


def _queries_near(rng, sites, n):
    d = rng.normal(size=(n, 3))
    d *= rng.choice([0.0, 0.03, 0.07, 0.12, 0.2, 0.5], (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    g = np.empty((n, 4))
    g[:, :3] = sites[rng.integers(0, len(sites), n)] + d
    g[:, 3] = rng.uniform(0, 255, n)
    return g


def ragged_ranges(b2l=I4):
    """seven keyframes of RAGGED_SIZES points, to be run on every range of RAGGED_RANGES: every kernel indexes with gi - first_pt"""
    rng = np.random.default_rng(601)
    sites, t = _sites_target(rng, 1000, 3)
    poses = [_pose(rng, 10.0) for _ in RAGGED_SIZES]
    scans, off = _to_local(_queries_near(rng, sites, sum(RAGGED_SIZES)), RAGGED_SIZES, poses, b2l)
    poses = np.array(poses).reshape(-1, 16)
    return [("ragged_ranges", _case(_p4(t, 13), scans, off, poses, _inv(poses), 2, 0.01))]


def many_keyframes():
    """65537 + 300 keyframes of 0, 1 or 2 points, identity rotation, a translation of their own each: more than the 65535 a launch's grid takes
    in y.  k = 2 (two-phase) and k = 6 (the generic exact kernel)"""
    rng = np.random.default_rng(701)
    n_kf = 65537 + 300
    sizes = rng.integers(0, 3, n_kf)
    sites, t = _sites_target(rng, 500, 6)
    g = _queries_near(rng, sites, int(sizes.sum()))
    tr = np.round(rng.uniform(-20, 20, (n_kf, 3)), 3)
    poses = np.tile(np.eye(4).reshape(1, 16), (n_kf, 1))
    poses[:, [3, 7, 11]] = tr
    inv = poses.copy()
    inv[:, [3, 7, 11]] = -tr
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    scans = np.empty((len(g), 4), F32)
    scans[:, :3] = g[:, :3] - np.repeat(tr, sizes, axis=0)
    scans[:, 3] = g[:, 3]
    return [(f"many_keyframes-k{k}", _case(_p4(t, 14), scans, off, poses, inv, k, 0.01)) for k in (2, 6)]


def nonfinite_queries():
    """a clean keyframe with NaN, +inf, -inf and 3e38 written into single coordinates of seeded rows; a second keyframe left clean.  Once over 40
    target points (brute force), once over the small_pair map (grid, two-phase)"""
    target, scan, pose = small_pair_target()
    rng = np.random.default_rng(801)
    scan = scan[:600].copy()
    rows = rng.permutation(600)[:48]
    vals = [np.nan, np.inf, -np.inf, 3.0e38]
    for j, r in enumerate(rows):
        scan[r, j % 3] = vals[(j // 3) % 4]
    scans = np.concatenate([scan, small_pair_target()[1][:600]])
    off = np.array([0, 600, 1200], dtype=np.uint64)
    poses = np.array([pose, pose]).reshape(2, 16)
    inv = _inv(poses)
    out = [("nonfinite_queries-map", _case(target, scans, off, poses, inv, 2, 0.01))]
    # 40 target points (20 sites of two), the queries scattered around the sites, the same rows spoilt
    sites, t40 = _sites_target(rng, 20, 2, 5.0)
    s40, off40 = _to_local(_queries_near(rng, sites, 1200), [600, 600], [pose, pose])
    spoilt = ~np.isfinite(scan[:, :3]) | (scan[:, :3] == F32(3.0e38))
    s40[:600, :3][spoilt] = scan[:, :3][spoilt]
    out.append(("nonfinite_queries-Mt40", _case(_p4(t40, 15), s40, off40, poses, inv, 2, 0.01)))
    return out


BUILDERS = {"straddle": straddle, "exact_threshold": exact_threshold, "unsorted_queue": unsorted_queue, "clamped_cell": clamped_cell,
            "crowded_and_thin_cells": crowded_and_thin_cells, "bucketless": bucketless, "small_targets": small_targets,
            "far_and_outside": far_and_outside, "ragged_ranges": ragged_ranges, "many_keyframes": many_keyframes, "nonfinite_queries": nonfinite_queries}


@functools.lru_cache(maxsize=None)
def cases(name):
    """the (label, case) list of one builder, built once per process"""
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name, index, kf_begin=0, kf_end=None):
    """(coexist flags, local-frame points) of case `index` of builder `name` under the oracle's brute-force search (identity extrinsic), computed
    once per process.  Entries outside [kf_begin, kf_end) are not filled"""
    target, scans, off, poses, inv, k, thr = cases(name)[index][1]
    return _orc().knn_labels(target, scans, off, poses, inv, I4, k, thr, kf_begin, kf_end, use_kdtree=False)


@functools.lru_cache(maxsize=None)
def expected_split(name, index):
    """near flags of the same queries, flattened to one global-frame cloud, under the oracle's brute-force knn_split; computed once per process"""
    case = cases(name)[index][1]
    return _orc().knn_split(case[0], global_points(case), case[5], case[6], use_kdtree=False)


def with_extrinsic(case, l2b=L2B):
    """the same global-frame queries seen through a LiDAR -> base extrinsic: scan points re-derived so that pose * base2lidar * p (quirk Q7) lands on
    them up to float rounding.  Returns (case, base2lidar); the expected values come from knn_labels(..., base2lidar, ...)"""
    target, scans, off, poses, inv, k, thr = case
    b2l = _orc().inverse4x4(l2b)
    g = global_points(case).astype(np.float64)
    local, off2 = _to_local(g, np.diff(off.astype(np.int64)), poses, b2l)
    assert (off2 == off).all()
    return _case(target, local, off, poses, inv, k, thr), b2l


def global_points(case):
    """the queries of a case in the global frame (identity extrinsic), flattened: the input of ltm_knn_split_cloud"""
    _, scans, off, poses, _, _, _ = case
    return _orc().merge_to_global(scans, off, poses, I4)
