"""Fixtures of the "fpfh matches" and "initial alignment" tests (include/ltm.h).  Matches: 33-float rows made by hand, so that ties are exact and NaN rows
sit where the kernel's tiles meet; match_cases(tile) gives name -> (target rows, source rows, kc) for a kernel that stages `tile` target rows at a time.
Alignment: well_posed(), a scene pair 30 degrees and 3 m apart with the restatement's descriptors, matches and alignment, and sac_cases(block), small pairs
around the vote kernel's block of `block` voting points with random descriptors.  The CPU tests pin the restatement (tools/sac_numpy.py) on them, the GPU
tests compare the device with it.  Everything is seeded; the restatement's results are computed once per process and shared."""
import functools

import numpy as np

import icp_fixtures as fx
from tools import fpfh_numpy as fref
from tools import normals_numpy as nref
from tools import sac_numpy as sref

SIZE = 33
KCS = (1, 4, 5, 8, 9, 16)               # 4 / 8 / 16 register slots full and one past the first two, the limits
SOURCE_ROWS = (1, 255, 256, 257)        # one row, one workgroup less one, exactly one, one more


def histogram_rows(n, seed):
    """rows shaped like FPFH descriptors: three groups of 11 non-negative floats, each group summing to about 100"""
    rng = np.random.default_rng(seed)
    g = rng.gamma(0.6, 1.0, size=(n, 3, 11)) + 1e-3
    return np.ascontiguousarray((100.0 * g / g.sum(axis=2, keepdims=True)).reshape(n, SIZE), dtype=np.float32)


def integer_rows(n, seed, patterns=5):
    """rows drawn from a handful of small-integer patterns: every distance is an exact small integer in float32 and most of them tie"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, size=(patterns, SIZE)).astype(np.float32)
    return np.ascontiguousarray(base[rng.integers(0, patterns, size=n)]), base


# the hand case of the CPU tests: the distances from an all-zero source row are 0, 1, 0, 4, 1
def hand_target():
    t = np.zeros((5, SIZE), np.float32)
    t[1, 0] = 1.0
    t[3, 5] = 2.0
    t[4, 1] = 1.0
    return t


def match_cases(tile):
    cases = {}
    for kc in KCS:
        cases[f"kc{kc}"] = (histogram_rows(tile + 1, 100 + kc), histogram_rows(70, 200 + kc), kc)
    for nt in (0, 1, 4, tile - 1, tile, tile + 1, 2 * tile + 3):      # 4 = kc - 1
        cases[f"nt{nt}"] = (histogram_rows(nt, 300 + nt), histogram_rows(70, 301), 5)
    for ns in SOURCE_ROWS:
        cases[f"ns{ns}"] = (histogram_rows(40, 400), histogram_rows(ns, 401 + ns), 4)
    cases["ns0"] = (histogram_rows(40, 400), np.zeros((0, SIZE), np.float32), 4)
    # exact ties across the tile boundaries: every target row is one of five patterns, pattern 0 exactly at the eight rows around each of the first two
    # tile boundaries, and the sources are the patterns themselves and a few neighbours: lists of 16 are runs of equal distances ordered by row alone
    t, base = integer_rows(2 * tile + 5, 500)
    zero = (t == base[0]).all(axis=1)
    t[zero] = base[1]
    t[tile - 6:tile + 2] = base[0]
    t[2 * tile - 4:2 * tile + 4] = base[0]
    s = np.concatenate([base, base + np.float32(1.0), integer_rows(20, 501)[0]])
    cases["ties"] = (t, s, 16)
    cases["ties_kc5"] = (t, s, 5)
    # NaN rows on both sides: at the first row, either side of a tile boundary and the last row of the target; a source NaN in its first and last bin
    t = histogram_rows(tile + 9, 600)
    t[[0, tile - 1, tile, tile + 8], [3, 0, 32, 17]] = np.nan
    s = histogram_rows(66, 601)
    s[5, 0] = np.nan
    s[64, 32] = np.nan
    cases["nan"] = (t, s, 8)
    cases["nan_all_targets"] = (np.full((7, SIZE), np.nan, np.float32), histogram_rows(3, 602), 4)
    few = histogram_rows(6, 603)
    few[[1, 4], [2, 2]] = np.nan
    cases["nan_leaves_fewer_than_kc"] = (few, histogram_rows(9, 604), 8)      # four eligible rows for eight slots
    # infinite components: +inf distances are listed after every finite one by row, inf - inf is NaN and is not listed
    t = histogram_rows(12, 700)
    t[3, 4] = np.inf
    t[7, 4] = np.inf
    s = histogram_rows(5, 701)
    s[2, 4] = np.inf
    cases["inf"] = (t, s, 16)
    return cases


# ------------------------------------------------------------------------------------------------------------------ initial alignment
NORMALS_K = 10
# The well-posed pair: icp_fixtures.scene, the source 1000 of the target's own 3000 points with the fixture's 1 cm of noise, moved by the inverse of 30 degrees
# of yaw and 3 m (mostly upwards, so that both clouds stay inside icp_fixtures.EXTENT).  Sources sampled apart from the target were tried first: ICP then has
# several fixed points a few centimetres apart and the start decides among them; with partners in the target the fixed point is one.
WELL_POSED = dict(seed=21, n_target=3000, n_source=1000, yaw_deg=30.0, t=(1.0, -1.0, 2.65), noise=0.01, fpfh_k=24, kc=4,
                  sac=dict(inlier_distance=0.3, max_iterations=1000, seed=0, similarity_threshold=0.9, inlier_fraction=0.2, eval_stride=1),
                  icp=dict(max_corr_dist=1.0))
WELL_POSED_CONSENSUS = 218      # what the restatement reaches (of 1000 voting points), recorded here: tests/test_sac_cases_cpu.py holds it to this


@functools.lru_cache(maxsize=None)
def well_posed():
    """dict: target, source (n, 3) float32, GT (4, 4), the restatement's descriptors, match lists and alignment"""
    w = WELL_POSED
    rng = np.random.default_rng(w["seed"])
    target = fx.scene(rng, w["n_target"])
    src = target[rng.permutation(w["n_target"])[:w["n_source"]]].astype(np.float64) + rng.normal(0.0, w["noise"], (w["n_source"], 3))
    GT = fx.rigid(w["yaw_deg"], w["t"])
    source = fx.apply(np.linalg.inv(GT), src)
    assert np.abs(target).max() < fx.EXTENT and np.abs(source).max() < fx.EXTENT

    def descriptors(p):
        return fref.fpfh(p, nref.estimate(p, NORMALS_K)["normals"][:, :3], w["fpfh_k"])["descriptors"]

    dt, ds = descriptors(target), descriptors(source)
    idx, dist = sref.match(dt, ds, w["kc"])
    return dict(target=target, source=source, GT=GT, target_rows=dt, source_rows=ds, match_idx=idx, match_dist=dist,
                align=sref.align(target, source, idx, **w["sac"]))


def displacement(A, B, pts):
    """the largest distance between the images of `pts` under the transforms A and B"""
    p = pts.astype(np.float64)
    return float(np.linalg.norm(p @ (A[:3, :3] - B[:3, :3]).T + (A[:3, 3] - B[:3, 3]), axis=1).max())


def _scene_pair(seed, n_target, n_source, nan_rows=True):
    rng = np.random.default_rng(seed)
    target = fx.scene(rng, n_target)
    source = fx.apply(np.linalg.inv(fx.rigid(8.0, (0.5, -0.4, 0.1))), fx.scene(rng, n_source))
    if nan_rows and n_target > 8 and n_source > 8:      # a non-finite point on either side, so that draws meet one
        target[5, 1] = np.nan
        source[2, 0] = np.inf
    return target, source


def sac_cases(block):
    """name -> dict(target, source (n, 3) float32, target_rows, source_rows (n, 33), kc, params) for a vote kernel that gives a workgroup `block` voting
    points.  The descriptors are random histograms: the matches mean nothing, which the equality with the restatement does not need; the similarity
    threshold is low so that hypotheses survive, the inlier distance large so that they collect votes."""
    cases = {}

    def add(name, target, source, kc=3, rows=None, **params):
        p = dict(inlier_distance=1.0, max_iterations=40, seed=3, similarity_threshold=0.3, inlier_fraction=0.25, eval_stride=1)
        p.update(params)
        tr, sr = rows if rows is not None else (histogram_rows(len(target), 900 + len(cases)), histogram_rows(len(source), 950 + len(cases)))
        cases[name] = dict(target=np.ascontiguousarray(target, np.float32), source=np.ascontiguousarray(source, np.float32), target_rows=tr, source_rows=sr, kc=kc, params=p)

    t, s = _scene_pair(31, 300, 3, nan_rows=False)
    add("source_of_3", t, s, max_iterations=64, similarity_threshold=0.0)
    for n in (block - 1, block, block + 1):
        t, s = _scene_pair(32 + n, 300, n)
        add(f"source_{n}", t, s)      # one finite point less than n: the inf row
    t, s = _scene_pair(40, 300, block + 2)
    add("source_block_plus_1_finite", t, s, max_iterations=16)      # block + 1 voting points
    t, s = _scene_pair(41, 200, 90)
    add("stride_larger_than_source", t, s, eval_stride=1000)
    add("stride_4", t, s, eval_stride=4, max_iterations=100)
    for h in (1, 255, 256, 257):      # the hypothesis kernel takes 256 per workgroup
        add(f"iterations_{h}", t, s, max_iterations=h, similarity_threshold=0.5)
    t4, s4 = _scene_pair(42, 4, 60, nan_rows=False)
    add("target_of_4", t4, s4, max_iterations=128, similarity_threshold=0.0, inlier_distance=3.0)
    # every hypothesis invalid: all rows of the source are one repeated row and point
    one = np.tile(np.float32([1.0, 2.0, 0.5]), (50, 1))
    add("all_invalid", t, one, rows=(histogram_rows(len(t), 990), np.tile(histogram_rows(1, 991), (50, 1))), similarity_threshold=0.0)
    add("empty_source", t, np.zeros((0, 3), np.float32))
    add("empty_target", np.zeros((0, 3), np.float32), s)
    far = np.float32(fx.FAR)
    add("far", t + far, s + far, max_iterations=100)
    add("kc16", t, s, kc=16, max_iterations=100)
    add("strict", t, s, similarity_threshold=0.9, max_iterations=300)
    return cases


BATCH = ("source_of_3", "empty_source", "stride_4", "target_of_4", "all_invalid", "far")      # one call over all of them where their parameters agree


@functools.lru_cache(maxsize=None)
def restated(name, block):
    """the restatement's matches and alignment of a case, once per process"""
    c = sac_cases(block)[name]
    idx, dist = sref.match(c["target_rows"], c["source_rows"], c["kc"])
    return idx, dist, sref.align(c["target"], c["source"], idx, **c["params"])
