"""Fixtures of the search-index tests (tests/test_search_cases_cpu.py, tests/test_gpu_search_edges.py) and a host model of the index: small clouds at the
seams of ltm_search_walk.h and ltm_k_search.hip -- finite counts on both sides of a leaf (32) and of a power-of-two leaf count, every list form of the kNN
kernels full and part full, every state of the kNN seed, exact ties by index, radii on both sides of a tie and at the ends of the float range, and clouds
whose squared distances underflow, are denormal, overflow, or whose codes collapse.  Every cloud is float32 [n, 4] in a permuted order (the intensity
carries the row's number before the permutation, -1 on a non-finite row).

  SHAPES / TIES / RANGE    name -> Case(target, queries, radii); radii are float32 values, used as they are on both sides
  CASES                    all of them; radius_list(name) adds the radii and max_nn values that depend on the brute force
  brute(name)              the reference: every query's finite targets in (d2, index) order, d2 = ((dx*dx)+dy*dy)+dz*dz in float32, computed once
  tree_model(target, bound)  a plain restatement of frame_of, quant21, the Morton code, the stable order by code, leaves of 32, P, the boxes, seed_leaves
                           and walk, with the lower bound of a box either as it was before the absolute term ("relative") or as it is ("fixed")

The model is the specification of the branches: per query it says which seed clamp was taken, how many leaves the seed covered and how many nodes the
walk refused.  It is slow and obvious on purpose."""
import collections
import functools

import numpy as np

from voxel_cases import morton

F32 = np.float32
LEAF = 32                               # kSearchLeaf
K_ALL = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)
K_FEW = (1, 4, 16, 17, 64)
SHAPE_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 1024, 1025)
INF = float("inf")
DENORM_MIN = 2.0 ** -149                # the smallest float32 above 0
NORMAL_MIN = 2.0 ** -126
ABS_TERM = 2.0 ** -148                  # box_lower_bound's absolute term (ltm_box_bound.h)

Case = collections.namedtuple("Case", "target queries radii")


# ------------------------------------------------------------------------------------------------------------------ clouds
def _xyzi(xyz, seed):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p = np.concatenate([xyz.astype(F32), np.arange(len(xyz), dtype=F32)[:, None]], axis=1)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(len(p))])


def with_non_finite(pts):
    """three rows with one non-finite coordinate each (NaN in x, +inf in y, -inf in z) in front of rows Mf/3, Mf/2 and 2Mf/3: n_target = Mf + 3, and a
    target index is not a sorted position"""
    n = len(pts)
    bad = np.array([[np.nan, 1.0, 2.0, -1.0], [3.0, np.inf, 4.0, -1.0], [5.0, 6.0, -np.inf, -1.0]], F32)
    return np.ascontiguousarray(np.insert(pts, [n // 3, n // 2, (2 * n) // 3], bad, axis=0))


def finite_rows(pts):
    return np.isfinite(pts[:, :3]).all(axis=1)


def queries(target, seed=77):
    """32 finite target points as they are, 32 more moved by N(0, 0.3 m), the two corners of the finite box, one point 50 m beyond each of its six faces
    (codes clamped at 0 and at 2097151 on every axis), two non-finite rows"""
    rng = np.random.default_rng(seed)
    fin = target[finite_rows(target), :3].astype(np.float64)
    lo, hi = fin.min(axis=0), fin.max(axis=0)
    same = fin[rng.integers(0, len(fin), 32)]
    moved = fin[rng.integers(0, len(fin), 32)] + rng.normal(0.0, 0.3, (32, 3))
    beyond = np.tile((lo + hi) / 2.0, (6, 1))
    for a in range(3):
        beyond[2 * a, a] = lo[a] - 50.0
        beyond[2 * a + 1, a] = hi[a] + 50.0
    q = np.concatenate([same, moved, [lo, hi], beyond, [[np.nan, 0.0, 0.0], [0.0, -np.inf, 0.0]]])
    out = np.zeros((len(q), 4), F32)
    with np.errstate(all="ignore"):
        out[:, :3] = q.astype(F32)
    return out


def _cube(n, side, seed, origin=0.0):
    return origin + np.random.default_rng(seed).uniform(0.0, side, (n, 3))


def _shapes():
    c = {}
    for n in SHAPE_SIZES:
        t = with_non_finite(_xyzi(_cube(n, 8.0, 100 + n), n))
        c[f"n{n}"] = Case(t, queries(t), (F32(INF),))
    return c


def _lattice_x3():
    g = np.arange(5, dtype=np.float64)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    h = np.arange(4, dtype=np.float64) + 0.5
    centres = np.stack(np.meshgrid(h, h, h, indexing="ij"), axis=-1).reshape(-1, 3)
    q = np.zeros((len(lat) + len(centres), 4), F32)
    q[:, :3] = np.concatenate([lat, centres])
    radii = (F32(0.0), F32(1.0), np.nextafter(F32(1.0), F32(2.0)), np.sqrt(F32(2.0)), F32(-1.0), F32(INF), F32(1e-30))
    return Case(_xyzi(np.tile(lat, (3, 1)), 21), q, radii)


def _ties():
    c = {"lattice_x3": _lattice_x3()}
    t = _xyzi(np.tile([[1.5, -2.25, 3.0]], (100, 1)), 22)
    c["coincident_100"] = Case(t, queries(t), (F32(0.0), F32(0.3), F32(INF)))
    two = np.empty((140, 3))
    two[0::2] = [1.0, 2.0, 3.0]
    two[1::2] = [-4.0, 0.5, 2.0]
    t = np.concatenate([two.astype(F32), np.arange(140, dtype=F32)[:, None]], axis=1)      # interleaved by index: not permuted
    c["two_values_140"] = Case(t, queries(t), (F32(0.3), F32(5.5), F32(INF)))
    return c


def _tiny_radii():
    """radii whose r2 = (float)((double)r * r) is 2^-149, 8 * 2^-149 and 2^-126"""
    return tuple(F32(np.sqrt(np.float64(v))) for v in (DENORM_MIN, 8.0 * DENORM_MIN, NORMAL_MIN))


def _range():
    c = {}
    for name, side, seed in (("underflow_cube", 1e-23, 31), ("partial_underflow", 2e-22, 32), ("partial_underflow_1e22", 1e-22, 37), ("denormal_results", 1e-20, 33)):
        t = _xyzi(_cube(300, side, seed), seed)
        q = t.copy()
        q[:, 3] = 0.0
        c[name] = Case(t, q, _tiny_radii() + (F32(INF),) if name != "denormal_results" else (F32(2e-21), F32(INF)))
    rng = np.random.default_rng(34)
    xyz = _cube(200, 10.0, 34)
    huge = rng.choice(200, 6, replace=False)
    xyz[huge] = rng.choice([-3e38, 3e38], (6, 3))
    t = _xyzi(xyz, 34)
    hq = t[np.flatnonzero(np.abs(t[:, 0]) > 1e38)[:3]].copy()
    hq[:, 3] = 0.0
    c["overflow"] = Case(t, np.concatenate([queries(t[np.abs(t[:, 0]) < 1e38]), hq]), (F32(2.0), F32(1e19), F32(INF)))
    t = _xyzi(np.concatenate([_cube(300, 10.0, 35), [[1e30, 0.0, 0.0]]]), 35)
    far = np.array([[1e30, 0.0, 0.0, 0.0], [1e30, 5.0, 5.0, 0.0], [5e29, 0.0, 0.0, 0.0]], F32)
    c["collapse"] = Case(t, np.concatenate([queries(t[t[:, 0] < 1e29]), far]), (F32(2.0), F32(INF)))
    t = _xyzi(_cube(300, 6.0, 36, origin=1e7 - 3.0), 36)
    c["offset_1e7"] = Case(t, queries(t), (F32(1.0), F32(2.5), F32(INF)))
    return c


SHAPES = _shapes()
TIES = _ties()
RANGE = _range()
CASES = {**SHAPES, **TIES, **RANGE}


# --------------------------------------------------------------------------------------------------------------- brute force
def d2_matrix(q, t):
    """((dx*dx)+dy*dy)+dz*dz in float32 for every (query, target) pair"""
    q = np.asarray(q, F32)
    t = np.asarray(t, F32)
    with np.errstate(all="ignore"):
        dx = q[:, None, 0] - t[None, :, 0]
        dy = q[:, None, 1] - t[None, :, 1]
        dz = q[:, None, 2] - t[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def brute_force(q, t):
    """per query: the finite targets' indices in (d2, index) order, their d2, and which queries are finite (the others have empty rows)"""
    tf = np.flatnonzero(finite_rows(t))
    d = d2_matrix(q[:, :3], t[tf, :3])
    order = np.argsort(d, axis=1, kind="stable")      # stable on ascending index: ties by the smaller index
    return tf[order].astype(np.int32), np.take_along_axis(d, order, axis=1), finite_rows(q)


@functools.lru_cache(maxsize=None)
def brute(name):
    c = CASES[name]
    bi, bd, fq = brute_force(c.queries, c.target)
    for a in (bi, bd, fq):
        a.setflags(write=False)
    return bi, bd, fq


def r2_of(r):
    """r2 = (float)((double)radius * radius), include/ltm.h"""
    with np.errstate(all="ignore"):
        return F32(np.float64(r) * np.float64(r))


def want_knn(name, k):
    bi, bd, fq = brute(name)
    kk = min(k, bi.shape[1])
    wi = np.full((len(fq), k), -1, np.int32)
    wd = np.full((len(fq), k), np.inf, F32)
    wi[fq, :kk] = bi[fq, :kk]
    wd[fq, :kk] = bd[fq, :kk]
    return wi, wd


def want_radius(name, r, max_nn=0):
    """CSR (offsets uint64, idx int32, d2 float32) of the brute force"""
    bi, bd, fq = brute(name)
    r2 = r2_of(r)
    m = np.where(fq, (bd < r2).sum(axis=1), 0)
    if max_nn:
        m = np.minimum(m, max_nn)
    off = np.concatenate([[0], np.cumsum(m)]).astype(np.uint64)
    keep = np.arange(bi.shape[1])[None, :] < m[:, None]
    return off, bi[keep], bd[keep]


@functools.lru_cache(maxsize=None)
def radius_list(name):
    """every (radius, max_nn) of a case: its radii with max_nn 0, 1 and 5; on the shapes also the float32 square root of the median 5th-neighbour distance,
    there with max_nn around the count c >= 2 of one fixed row (c - 1, c, c + 1); on the lattice nextafter(1, 2) with max_nn = 3, inside the six tied
    neighbours at distance 1"""
    c = CASES[name]
    bi, bd, fq = brute(name)
    out = [(r, m) for r in c.radii for m in (0, 1, 5)]
    if name in SHAPES:
        col = min(4, bd.shape[1] - 1)
        r = np.sqrt(F32(np.median(bd[fq, col])))
        out += [(r, m) for m in (0, 1, 5)]
        counts = np.where(fq, (bd < r2_of(r)).sum(axis=1), 0)
        rows = np.flatnonzero(counts >= 2)
        if len(rows):
            cnt = int(counts[rows[0]])
            out += [(r, m) for m in (cnt - 1, cnt, cnt + 1)]
    if name == "lattice_x3":
        out.append((np.nextafter(F32(1.0), F32(2.0)), 3))
    return tuple((F32(r), int(m)) for r, m in out)


# ---------------------------------------------------------------------------------------------------------------- host model
KnnStat = collections.namedtuple("KnnStat", "clamp seed_a seed_b skipped")      # clamp: "zero" | "end" | "interior"


class TreeModel:
    def __init__(self, target, bound):
        assert bound in ("relative", "fixed")
        self.bound = bound
        t = np.ascontiguousarray(target, F32).reshape(-1, 4)
        fin = np.flatnonzero(finite_rows(t))
        assert len(fin), "the model is of a non-empty index"
        p = t[fin, :3]
        # frame_of: origin = the box's minimum, scale = 2097151 / the largest extent (0 for a box that is a point)
        mn, mx = p.min(axis=0), p.max(axis=0)
        ext = float((mx.astype(np.float64) - mn.astype(np.float64)).max())
        self.origin = mn.astype(np.float64)
        self.scale = 2097151.0 / ext if ext > 0.0 else 0.0
        code = self.codes(p)
        order = np.argsort(code, kind="stable")          # the radix sort keeps ascending index among equal codes (the batched, segmented sort does not)
        self.keys = code[order]
        self.pts = p[order]                              # finite target points in Morton order
        self.idx = fin[order].astype(np.int32)           # their rows in the target as given
        self.Mf = len(fin)
        self.L = (self.Mf + LEAF - 1) // LEAF
        self.P = 1
        while self.P < self.L:
            self.P <<= 1
        # boxes of nodes 1 .. 2P-1: leaf l is node P + l, padding leaves are empty (+inf, -inf), an inner node is the union of its children
        self.lo = np.full((2 * self.P, 3), np.inf, F32)
        self.hi = np.full((2 * self.P, 3), -np.inf, F32)
        for l in range(self.L):
            s = self.pts[l * LEAF:min((l + 1) * LEAF, self.Mf)]
            self.lo[self.P + l], self.hi[self.P + l] = s.min(axis=0), s.max(axis=0)
        for v in range(self.P - 1, 0, -1):
            self.lo[v] = np.minimum(self.lo[2 * v], self.lo[2 * v + 1])
            self.hi[v] = np.maximum(self.hi[2 * v], self.hi[2 * v + 1])

    def codes(self, xyz):
        """search_key: quant21 per axis, floor(((double)v - o) * scale) clamped to [0, 2097151]; a non-finite point gets ~0"""
        xyz = np.asarray(xyz, F32).reshape(-1, 3)
        ok = np.isfinite(xyz).all(axis=1)
        with np.errstate(all="ignore"):
            t = np.floor((np.where(ok[:, None], xyz, 0).astype(np.float64) - self.origin) * self.scale)
        code = morton(np.clip(t, 0.0, 2097151.0).astype(np.int64), 21)
        code[~ok] = np.uint64(0xFFFFFFFFFFFFFFFF)
        return code

    def box_lb(self, q):
        """lower bounds of the squared distance from q to every node's box, in double"""
        q = q.astype(np.float64)
        with np.errstate(all="ignore"):
            g = np.maximum(np.maximum(self.lo.astype(np.float64) - q, q - self.hi.astype(np.float64)), 0.0)
            s = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]) * (1.0 - 1.0e-6)
            if self.bound == "fixed":
                s = np.maximum(s - ABS_TERM, 0.0)
        return s

    def seed_leaves(self, qkey, kk):
        p = int(np.searchsorted(self.keys, qkey, side="left"))      # lower_bound_key
        half = kk // 2
        clamp = "interior"
        if p > half:
            start = p - half
        else:
            start, clamp = 0, "zero"
        if start + kk > self.Mf:
            start, clamp = self.Mf - kk, "end"
        return start // LEAF, (start + kk - 1) // LEAF, clamp

    def walk(self, lb, skip_a, skip_b, skip, visit):
        """the stackless depth-first walk; returns the number of nodes that skip() refused"""
        node, refused = 1, 0
        while True:
            if node < self.P:
                if not skip(lb[node]):
                    node <<= 1
                    continue
                refused += 1
            else:
                l = node - self.P
                if l < self.L and not skip_a <= l <= skip_b:
                    if skip(lb[node]):
                        refused += 1
                    else:
                        visit(l)
            while node & 1:
                node >>= 1
            if node == 0:
                return refused
            node += 1

    def _leaf_pairs(self, drow, l):
        a, b = l * LEAF, min((l + 1) * LEAF, self.Mf)
        return [(float(drow[j]), int(self.idx[j])) for j in range(a, b)]

    def knn(self, q, k):
        """(idx [n, k], d2 [n, k], one KnnStat per query or None for a non-finite query)"""
        q = np.asarray(q, F32).reshape(-1, 4)
        kk = min(k, self.Mf)
        out_i = np.full((len(q), k), -1, np.int32)
        out_d = np.full((len(q), k), np.inf, F32)
        stats = [None] * len(q)
        qkeys = self.codes(q[:, :3])
        d = d2_matrix(q[:, :3], self.pts)
        for i in np.flatnonzero(finite_rows(q)):
            best = []                                        # the kk smallest (d2, index) seen so far, ascending

            def visit(l):
                best.extend(self._leaf_pairs(d[i], l))
                best.sort()                                  # tuples order as pair_less: distance, then index
                del best[kk:]

            def skip(lb):                                    # strictly above the current kk-th distance (+inf while the list is not full)
                return lb > (best[kk - 1][0] if len(best) == kk else INF)

            a, b, clamp = self.seed_leaves(qkeys[i], kk)
            for l in range(a, b + 1):
                visit(l)
            refused = self.walk(self.box_lb(q[i, :3]), a, b, skip, visit)
            out_i[i, :kk] = [j for _, j in best]
            out_d[i, :kk] = [dd for dd, _ in best]
            stats[i] = KnnStat(clamp, a, b, refused)
        return out_i, out_d, stats

    def radius(self, q, r, max_nn=0):
        """CSR (offsets, idx, d2) and the number of refused nodes per query"""
        q = np.asarray(q, F32).reshape(-1, 4)
        r2 = float(r2_of(r))
        d = d2_matrix(q[:, :3], self.pts)
        rows, refused = [], np.zeros(len(q), np.int64)
        for i in range(len(q)):
            hits = []
            if finite_rows(q[i:i + 1])[0]:
                refused[i] = self.walk(self.box_lb(q[i, :3]), 1, 0, lambda lb: lb >= r2, lambda l: hits.extend(p for p in self._leaf_pairs(d[i], l) if p[0] < r2))
            hits.sort()
            rows.append(hits[:max_nn] if max_nn else hits)
        off = np.concatenate([[0], np.cumsum([len(h) for h in rows])]).astype(np.uint64)
        return (off, np.array([j for h in rows for _, j in h], np.int32), np.array([dd for h in rows for dd, _ in h], F32), refused)


def tree_model(target, bound="fixed"):
    return TreeModel(target, bound)
