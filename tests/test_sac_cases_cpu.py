"""The "fpfh matches" and "initial alignment" semantics of include/ltm.h shown on the restatement alone (tools/sac_numpy.py, no device).  Matches: against
a brute force written another way, on hand cases with exact ties, NaN rows on either side and fewer eligible rows than kc, and that the fixtures of
tests/sac_cases.py sit on their seams.  Alignment: known values of the hash and the draws, the transform of a hypothesis, the well-posed pair through
tools/icp_numpy.py, the kinds of invalid hypothesis on the fixtures, and the source order."""
import numpy as np
import pytest

import icp_fixtures as fx
import sac_cases as sc
from tools import icp_numpy as iref
from tools import sac_numpy as sref

TILE = 128      # LTM_MATCH_TILE_ROWS; tests/test_sac_api_cpu.py holds the library to it
EPS32 = float(np.finfo(np.float32).eps)
# A float32 sum of 33 non-negative terms e * e, e a rounded difference: each term is within 3 roundings of its exact value and every partial sum adds one,
# so the sum is within (3 + 33) eps of the float64 value, relatively; 40 eps with room for the float64 side
ROUNDING = 40.0 * EPS32

CASES = sc.match_cases(TILE)


def _brute_force(target, source):
    """float64, another formula: |s|^2 is not used (it cancels badly); the differences are taken in float64 and squared, summed by numpy's pairwise sum"""
    s, t = source.astype(np.float64), target.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((s[:, None, :] - t[None, :, :]) ** 2).sum(axis=2)


@pytest.mark.parametrize("name", list(CASES))
def test_the_restatement_agrees_with_a_float64_brute_force(name):
    """wherever two float64 distances differ by more than the float32 rounding of either, the restatement orders them as float64 does: every listed row is
    no farther than the next listed one and than every eligible row left out, and the listed distances are the float64 ones to rounding"""
    target, source, kc = CASES[name]
    idx, dist = sref.match(target, source, kc)
    assert idx.shape == (len(source), kc) and idx.dtype == np.int32 and dist.shape == (len(source), kc) and dist.dtype == np.float32
    d64 = _brute_force(target, source)
    eligible = ~np.isnan(target).any(axis=1)
    for r in range(len(source)):
        filled = idx[r] >= 0
        n = int(filled.sum())
        assert filled[:n].all(), "filled slots come first"
        assert (np.isposinf(dist[r, n:])).all() and (idx[r, n:] == -1).all()
        if np.isnan(source[r]).any():
            assert n == 0
            continue
        row = d64[r]
        listable = eligible & ~np.isnan(row)
        assert n == min(kc, int(listable.sum()))
        got = idx[r, :n]
        assert len(set(got.tolist())) == n and listable[got].all()
        finite = np.isfinite(row[got])
        assert np.allclose(dist[r, :n][finite], row[got][finite], rtol=ROUNDING, atol=0.0)
        assert (np.isposinf(dist[r, :n][~finite])).all()
        with np.errstate(invalid="ignore"):
            for j in range(n - 1):
                a, b = got[j], got[j + 1]
                assert row[a] <= row[b] + ROUNDING * (row[a] + row[b]) or (np.isinf(row[a]) and np.isinf(row[b]))
                assert dist[r, j] < dist[r, j + 1] or (dist[r, j] == dist[r, j + 1] and a < b), "ascending by (distance, row)"
            if n:
                rest = np.flatnonzero(listable)
                rest = rest[~np.isin(rest, got)]
                last = row[got[-1]]
                ok = (row[rest] >= last - ROUNDING * (row[rest] + last)) | (np.isinf(last) & np.isinf(row[rest]))
                assert ok.all()


def test_hand_case_with_exact_ties():
    """from an all-zero source row the five target rows lie at 0, 1, 0, 4, 1: rows 0 and 2 tie, and so do 1 and 4"""
    t = sc.hand_target()
    s = np.zeros((1, sc.SIZE), np.float32)
    assert sref.distances(s, t).tolist() == [[0.0, 1.0, 0.0, 4.0, 1.0]]
    idx, dist = sref.match(t, s, 4)
    assert idx.tolist() == [[0, 2, 1, 4]] and dist.tolist() == [[0.0, 0.0, 1.0, 1.0]]
    idx, dist = sref.match(t, s, 1)
    assert idx.tolist() == [[0]] and dist.tolist() == [[0.0]]


def test_hand_case_with_nan_rows_on_either_side():
    t = sc.hand_target()
    t[2, 32] = np.nan
    s = np.zeros((2, sc.SIZE), np.float32)
    s[1, 0] = np.nan
    idx, dist = sref.match(t, s, 4)
    assert idx.tolist() == [[0, 1, 4, 3], [-1, -1, -1, -1]]
    assert dist[0].tolist() == [0.0, 1.0, 1.0, 4.0] and np.isposinf(dist[1]).all()


def test_hand_case_with_fewer_eligible_rows_than_kc():
    t = sc.hand_target()
    s = np.zeros((1, sc.SIZE), np.float32)
    idx, dist = sref.match(t, s, 8)
    assert idx.tolist() == [[0, 2, 1, 4, 3, -1, -1, -1]]
    assert dist[0, :5].tolist() == [0.0, 0.0, 1.0, 1.0, 4.0] and np.isposinf(dist[0, 5:]).all()
    idx, dist = sref.match(np.zeros((0, sc.SIZE), np.float32), s, 3)
    assert idx.tolist() == [[-1, -1, -1]] and np.isposinf(dist).all()


def test_the_distance_is_the_stated_float32_sum_in_bin_order():
    """a row where the order of the additions shows: 2^24 first and then thirty-two ones is 2^24 in float32, the ones first would give 2^24 + 32"""
    s = np.zeros((1, sc.SIZE), np.float32)
    t = np.ones((2, sc.SIZE), np.float32)
    t[0, 0] = 4096.0
    t[1, 32] = 4096.0
    d = sref.distances(s, t)
    assert d.dtype == np.float32 and d.tolist() == [[16777216.0, 16777248.0]]


def test_the_fixtures_sit_on_their_seams():
    t, s, kc = CASES["ties"]
    assert len(t) > 2 * TILE and (t[TILE - 1] == t[TILE]).all() and (t[TILE] == t[TILE + 1]).all() and (t[TILE] == t[2 * TILE]).all()
    idx, dist = sref.match(t, s, kc)
    # the first source row IS that pattern: its list is sixteen zeros in row order and crosses the first tile boundary
    assert (dist[0] == 0.0).all() and (np.diff(idx[0]) > 0).all() and idx[0].min() < TILE <= idx[0].max()
    t, s, kc = CASES["nan"]
    assert np.isnan(t[[0, TILE - 1, TILE, len(t) - 1]]).any(axis=1).all() and np.isnan(s).any(axis=1).sum() == 2
    assert sorted(len(CASES[f"ns{n}"][1]) for n in sc.SOURCE_ROWS) == [1, 255, 256, 257]
    assert sorted(len(CASES[n][0]) for n in CASES if n.startswith("nt")) == [0, 1, 4, TILE - 1, TILE, TILE + 1, 2 * TILE + 3]
    assert CASES["nt4"][2] == 5


# ------------------------------------------------------------------------------------------------------------------ initial alignment


def test_known_values_of_the_hash_and_the_draws():
    """seed, h, j -> the printed words and positions: x = seed + 0x9E3779B9 (6 h + j + 1) through murmur3's finaliser"""
    assert [sref.mix(0, 0, j) for j in range(6)] == [0x92CA2F0E, 0x3CD6E3F3, 0x1B147DCC, 0x4C081DBF, 0x487981AB, 0xDB408C9D]
    assert sref.mix(0, 1, 0) == sref.mix(0x9E3779B9 * 6 & 0xFFFFFFFF, 0, 0), "h enters only through 6 h + j + 1"
    assert sref.draws(7, 3, 1000) == [725, 372, 286]
    rows, slots = sref.draws(7, 3, 1000, [4, 1, 3])
    assert rows == [725, 372, 286] and slots[1] == 0 and all(0 <= m < k for m, k in zip(slots, [4, 1, 3]))
    assert sref.draws(5, 0, 1) == [0, 0, 0] and sref.draws(5, 0, 0) == [0, 0, 0]


def test_the_transform_of_a_hypothesis_maps_the_triangle_onto_its_partner():
    """three source points and their images under a rigid motion as the only rows: every valid hypothesis IS that motion (to rounding), its first edge and
    the triangle's plane exactly, and R is orthonormal"""
    G = fx.rigid(40.0, (1.0, 2.0, -0.5), pitch_deg=10.0)
    src = np.float32([[0.0, 0.0, 0.0], [2.0, 0.5, 0.0], [0.5, 3.0, 1.0]])
    tgt = fx.apply(G, src)
    idx = np.int32([[0], [1], [2]])
    seen = 0
    for h in range(40):
        state, T = sref.hypothesis(1, h, src, tgt, idx, 0.9)
        assert state in (sref.VALID, sref.COINCIDENT)
        if state == sref.VALID:
            seen += 1
            assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-14 and np.abs(T - G).max() < 1e-5
    assert seen >= 3


def test_the_well_posed_alignment_leads_icp_where_the_ground_truth_leads_it():
    """30 degrees of yaw and 3 m: ICP (max_corr_dist 1 m) started from the restatement's T ends where it ends from the ground truth -- the largest
    displacement over the source points is below the fixture's noise of 0.01 m, both runs stopping at steps of 1e-6 -- and started from identity it does
    not (a displacement above inlier_distance).  Measured: 1.7e-8 m and 7.9 m."""
    w = sc.well_posed()
    a = w["align"]
    assert a["found"] == 1 and a["consensus"] == sc.WELL_POSED_CONSENSUS and a["n_eval"] == len(w["source"])
    assert a["n_prerejected"] > 0 and (a["states"] == sref.COINCIDENT).sum() > 0, "hypotheses are prerejected and invalid by coincidence on this fixture"
    icp = sc.WELL_POSED["icp"]
    from_T, from_gt, from_identity = (iref.align(w["target"], w["source"], init=i, **icp) for i in (a["T"], w["GT"], None))
    print("displacements:", sc.displacement(from_T["T"], from_gt["T"], w["source"]), sc.displacement(from_identity["T"], from_gt["T"], w["source"]))
    assert sc.displacement(from_T["T"], from_gt["T"], w["source"]) < sc.WELL_POSED["noise"]
    assert sc.displacement(from_identity["T"], from_gt["T"], w["source"]) > sc.WELL_POSED["sac"]["inlier_distance"]
    assert sc.displacement(a["T"], from_gt["T"], w["source"]) > 10.0 * sc.WELL_POSED["noise"], "T itself is coarse: the fit is ICP's"


def test_invalid_hypotheses_of_every_kind_occur_on_the_fixtures():
    block = 1024
    far, strict, none = (sc.restated(n, block)[2] for n in ("far", "strict", "all_invalid"))
    assert (sc.restated("empty_target", block)[2]["states"] == sref.NO_MATCH).any(), "rows without a match"
    assert sc.restated("source_block_plus_1_finite", block)[2]["n_eval"] == block + 1 and sc.restated("stride_larger_than_source", block)[2]["n_eval"] == 1
    assert far["n_valid"] > 0 and far["consensus"] >= 3
    assert far["n_prerejected"] > 0 and strict["n_prerejected"] > 0
    assert (far["states"] == sref.COINCIDENT).sum() > 0 and (far["states"] == sref.NO_POINT).sum() > 0
    assert none["n_valid"] == 0 and none["best"] == -1 and none["found"] == 0 and np.isnan(none["T"]).all()
    assert far["n_valid"] + (far["states"] != sref.VALID).sum() == len(far["states"])
    best = far["best"]
    assert far["hyp_counts"][best] == far["hyp_counts"][far["hyp_valid"] == 1].max() == far["consensus"]
    assert not (far["hyp_counts"][:best][far["hyp_valid"][:best] == 1] == far["consensus"]).any(), "ties go to the smaller h"


def test_the_source_order_is_a_stable_order_by_code():
    pts = np.float32([[1.0, 1.0, 1.0], [np.nan, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    assert sref.source_order(pts).tolist() == [2, 4, 5, 0, 3]      # z is the least significant axis; the equal points keep their order; the NaN row is out
    assert sref.source_order(np.zeros((0, 3), np.float32)).tolist() == []
