"""The case matrix of the index walkers other than the kNN and radius kernels (tests/test_walker_cases_cpu.py, tests/test_gpu_walker_edges.py): normals,
statistical and radius outlier removal, clusters, FPFH and ICP over the clouds of tests/search_cases.py -- the tree shapes with 0 / 1 / 3 / 31 padding
leaves, exact ties by index, clouds whose squared distances underflow, are denormal, overflow or whose codes collapse -- with, per consumer, the parameters
at which its own list forms are full and one past, its radii sit on both sides of a tie, and its counts sit on both sides of a threshold.  No second copy
of a cloud: CASES is search_cases.CASES plus two clouds at a tiny cluster tolerance that only the cluster consumer uses.

  CASES                     name -> target float32 [n, 4]
  brute_self(name)          (fin, bi, bd): the finite rows of the target, and per finite row all finite targets in (d2, index) order (original indices) with
                            their float d2 -- the queries of every consumer but ICP are the target's own points.  Computed once, read-only
  normals_ks / sor_mean_ks / ror_list / cluster_tolerances / FPFH_CLOUDS, FPFH_KS / ICP_CLOUDS, ICP_MAX_CORR
  clique_leaves(model, r2, rule)   the clique rule of the cluster kernels restated over the leaf boxes of search_cases.TreeModel, as it was ("old": the
                            relative growth alone) and as it is ("new": with the absolute term of ltm_box_bound.h)
  bfs_components(d2, r2)    connected components of d2 < r2 by a plain breadth-first search over the full matrix"""
import functools

import numpy as np

import search_cases as sc

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)

# ------------------------------------------------------------------------------------------------------------------ clouds
# Two points whose exact squared distance is 7.2 * 2^-149 while the float one is 8 * 2^-149 (the squares 2.6, 2.6 and 2.0 units round to 3 + 3 + 2), at a
# tolerance whose r2 is 8 * 2^-149: not adjacent under float d2 < r2, yet the exact diagonal of their box, grown by a relative 1e-6, is below r2.
TINY_TOLERANCE = F32(np.sqrt(np.float64(8.0 * sc.DENORM_MIN)))
_CORNER = (np.sqrt(np.array([2.6, 2.6, 2.0])) * 2.0 ** -74.5).astype(F32)


def _tiny():
    pair = np.zeros((2, 4), F32)
    pair[1, :3] = _CORNER
    pair[:, 3] = (0.0, 1.0)
    # 20 points at either end of the same diagonal, interleaved by index: the first leaf of 32 holds both ends (its box is the pair's), the second one end
    forty = np.zeros((40, 4), F32)
    forty[1::2, :3] = _CORNER
    forty[:, 3] = np.arange(40)
    return {"tiny_tol_pair": pair, "tiny_tol_40": forty}


TINY = _tiny()
CASES = {**{name: c.target for name, c in sc.CASES.items()}, **TINY}
for _a in TINY.values():
    _a.setflags(write=False)

FULL_K_SHAPES = ("n33", "n97", "n1025")      # the shapes that get every k; the other sizes get a few
MATRIX = list(sc.CASES)                      # every consumer but the cluster one runs over these
TIES_AND_RANGE = list(sc.TIES) + list(sc.RANGE)


def _full(name):
    return name in FULL_K_SHAPES or name in sc.TIES or name in sc.RANGE


@functools.lru_cache(maxsize=None)
def brute_self(name):
    t = CASES[name]
    fin = np.flatnonzero(sc.finite_rows(t))
    bi, bd, _ = sc.brute_force(np.ascontiguousarray(t[fin]), t)
    for a in (fin, bi, bd):
        a.setflags(write=False)
    return fin, bi, bd


# -------------------------------------------------------------------------------------------------------------- parameters
NORMALS_K_ALL = (3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)      # 4 / 8 / 16 register slots full and one on either side, the LDS ends
NORMALS_K_FEW = tuple(k for k in sc.K_FEW if 3 <= k <= 64)
SOR_MEAN_K_ALL = (1, 2, 3, 4, 7, 8, 15, 16, 31, 63)                      # slots = mean_k + 1: 4 / 8 / 16 full, one past, the LDS ends
SOR_MEAN_K_FEW = (3, 15, 16, 63)
SOR_STDDEV_MUL = 1.0


def normals_ks(name):
    return NORMALS_K_ALL if _full(name) else NORMALS_K_FEW


def sor_mean_ks(name):
    return SOR_MEAN_K_ALL if _full(name) else SOR_MEAN_K_FEW


def _valid_radii(name):
    """the radii of search_cases.radius_list a filter or a cluster call accepts (finite, > 0), each once, in the order they come"""
    out = []
    for r, _ in sc.radius_list(name):
        if np.isfinite(r) and r > 0 and not any(r == o for o in out):
            out.append(r)
    return out


LATTICE_NEXT = np.nextafter(F32(1.0), F32(2.0))
# (radius, the next float above it): pairs with d2 == r2 exist at the first, and the very same pairs are inside at the second
RADII_AT_A_TIE = {"lattice_x3": ((F32(1.0), LATTICE_NEXT),)}


def self_counts(name, r):
    """per finite row: how many finite targets, the point itself included, have float d2 < r2"""
    _, _, bd = brute_self(name)
    return (bd < sc.r2_of(r)).sum(axis=1)


@functools.lru_cache(maxsize=None)
def ror_list(name):
    """(radius, min_neighbors): every valid radius with min_neighbors 1, 2, c, c + 1, 33 and Mf + 1 (c: the count of the first row that has one >= 2);
    on the lattice the radii on both sides of the tie at distance 1 with 3 | 4 (the three copies of the point) and 21 | 22 (with its six neighbours)"""
    fin, _, _ = brute_self(name)
    out = []
    for r in _valid_radii(name):
        counts = self_counts(name, r)
        rows = np.flatnonzero(counts >= 2)
        c = int(counts[rows[0]]) if len(rows) else 1
        for m in sorted({1, 2, c, c + 1, 33, len(fin) + 1}):
            out.append((r, m))
    if name == "lattice_x3":
        out += [(r, m) for r in (F32(1.0), LATTICE_NEXT) for m in (3, 4, 21, 22)]
    return tuple(dict.fromkeys((F32(r), int(m)) for r, m in out))


@functools.lru_cache(maxsize=None)
def cluster_tolerances(name):
    """the valid radii whose r2 is above 0 (on the lattice 1, the next float, sqrt 2; on the underflow cubes the tiny radii; ...), min_size 1, no max_size"""
    if name in TINY:
        return (TINY_TOLERANCE,)
    return tuple(r for r in _valid_radii(name) if sc.r2_of(r) > 0)


CLUSTER_CLOUDS = MATRIX + list(TINY)
FPFH_CLOUDS = ("n33", "n65", "n97", "n129", "n1025", "lattice_x3", "two_values_140", "offset_1e7", "collapse")
FPFH_KS = (2, 4, 5, 16, 17, 64)
ICP_CLOUDS = [n for n in MATRIX if n != "overflow"]
ICP_MAX_CORR = (1.0, 150.0)


# ---------------------------------------------------------------------------------------------------------------- restatements
def clique_leaves(model, r2, rule):
    """bool per leaf of a search_cases.TreeModel: every pair of its points counts as adjacent without being tested.  "old": diag^2 (1 + 1e-6) < r2 in
    double; "new" (box_is_clique of ltm_box_bound.h): diag^2 (1 + 1e-6) + 2^-148 < r2 and not beyond the float range"""
    assert rule in ("old", "new")
    lo = model.lo[model.P:model.P + model.L].astype(np.float64)
    hi = model.hi[model.P:model.P + model.L].astype(np.float64)
    e = hi - lo
    ub = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]) * (1.0 + 1.0e-6)
    if rule == "old":
        return ub < float(r2)
    ub = ub + sc.ABS_TERM
    return (ub < float(r2)) & (ub <= FLT_MAX)


def leaf_is_all_adjacent(model, l, r2):
    """the truth a clique flag claims: every pair of the leaf's points has float d2 < r2"""
    s = model.pts[l * sc.LEAF:min((l + 1) * sc.LEAF, model.Mf)]
    return bool((sc.d2_matrix(s, s) < r2).all())


def bfs_components(d2, r2):
    """component number per row of the symmetric matrix d2 under the relation d2 < r2, numbered in the order of their lowest row"""
    n = len(d2)
    adj = d2 < r2
    comp = np.full(n, -1, np.int64)
    nc = 0
    for s in range(n):
        if comp[s] >= 0:
            continue
        comp[s] = nc
        todo = [s]
        while todo:
            i = todo.pop()
            nb = np.flatnonzero(adj[i] & (comp < 0))
            comp[nb] = nc
            todo.extend(nb.tolist())
        nc += 1
    return comp


def self_d2(name):
    """float d2 between the finite rows of the target, in their given order"""
    t = CASES[name]
    f = t[sc.finite_rows(t), :3]
    return sc.d2_matrix(f, f)
