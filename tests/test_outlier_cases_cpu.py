"""The fixtures of tests/outlier_cases.py are well-posed, shown on the restatement alone (tools/outlier_numpy.py, no device): the clamp fixture needs the
clamp, the scenes are scenes (the filter removes something and keeps most: a condition on the inputs, not on the device), the fixed-shape sums are sums, the
boundary fixtures sit on their boundaries, and the documented defaults hold."""
import math

import numpy as np
import pytest

import outlier_cases as oc
from tools import outlier_numpy as oref


def test_the_clamp_fixture_has_a_negative_unclamped_variance():
    pts, mean_k, mul = oc.SOR["clamp"]
    want = oc.reference("sor", "clamp")
    d = want["distances"]
    assert mean_k == 1 and len(pts) == 100 and (d == d[0]).all() and d[0] == np.float32(math.sqrt(float(np.float32(0.7) * np.float32(0.7))))
    assert want["variance_unclamped"] < 0.0, want["variance_unclamped"]
    print(f"unclamped variance {want['variance_unclamped']:.3e}")
    # without the clamp the threshold is NaN and nothing passes <=; with it stddev is 0, the threshold is the common distance and everything is kept
    _, sd, thr, _ = oref.sor_statistics(d, 100, mul, clamp=False)
    assert math.isnan(sd) and math.isnan(thr) and not (d.astype(np.float64) <= thr).any()
    assert want["stddev"] == 0.0 and want["threshold"] == want["mean"] and want["n_kept"] == 100 and want["labels"].all()


@pytest.mark.parametrize("kind,name", oc.SCENES)
def test_a_scene_loses_something_and_keeps_most(kind, name):
    want = oc.reference(kind, name)
    removed = want["n_target"] - want["n_kept"]
    print(f"{kind} {name}: {removed} of {want['n_target']} removed")
    assert 1 <= removed <= want["n_target"] // 2


def test_fixed_shape_sums_equal_fsum():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 255, 256, 257, 1000, 16383, 16384, 16385, 40000):
        v = rng.uniform(0.0, 3.0, n).astype(np.float32).astype(np.float64)
        for w in (v, v * v):
            exact = math.fsum(w.tolist())
            got = oref.fixed_sum(w)
            assert abs(got - exact) <= 1e-12 * abs(exact), (n, got, exact)
    assert oref.fixed_sum([]) == 0.0
    # the shape itself: a chain loses every 2^-53 to the 1 in front, the tree adds the odd positions to each other before they meet position 0
    v = np.zeros(256)
    v[0], v[1::2] = 1.0, 2.0 ** -53
    assert oref.fixed_sum(v) == 1.0 + 2.0 ** -46 and float(np.add.accumulate(v)[-1]) == 1.0


def test_degenerate_and_boundary_fixtures_are_what_their_names_say():
    for kind, name in (("sor", "empty"), ("ror", "empty")):
        want = oc.reference(kind, name)
        assert (want["n_target"], want["n_finite"], want["n_kept"]) == (0, 0, 0)
    want = oc.reference("sor", "empty")
    assert (want["mean"], want["stddev"], want["threshold"]) == (0.0, 0.0, 0.0)
    want = oc.reference("sor", "one_point")
    assert (want["n_finite"], want["mean"], want["stddev"], want["n_kept"]) == (1, 0.0, 0.0, 1) and want["distances"][0] == 0.0
    want = oc.reference("sor", "two_points")      # mean_k 8 stays the divisor: 0.5 / 8
    assert (want["distances"] == np.float32(0.0625)).all() and want["n_kept"] == 2
    for kind in ("sor", "ror"):
        want = oc.reference(kind, "all_non_finite")
        assert want["n_finite"] == 0 and want["n_kept"] == 0 and not want["labels"].any()
        want = oc.reference(kind, "non_finite_mixed")
        fin = oref.finite_mask(oc.case(kind, "non_finite_mixed")[0])
        assert 0 < want["n_finite"] == fin.sum() < want["n_target"] and not want["labels"][~fin].any()
    assert (oc.reference("sor", "non_finite_mixed")["distances"][~oref.finite_mask(oc.SOR["non_finite_mixed"][0])] == 0.0).all()
    for mk in (8, 20):
        for extra in (0, 1, 2):
            assert oc.reference("sor", f"k{mk}_n{mk + extra}")["n_finite"] == mk + extra
    want = oc.reference("sor", "coincident_500")
    assert not want["distances"].any() and want["n_kept"] == 500 and want["threshold"] == 0.0
    want = oc.reference("ror", "coincident_500")
    assert (want["counts"] == 500).all() and want["n_kept"] == 500
    assert sorted(oc.SOR[f"blob_k{mk}"][1] for mk in oc.MEAN_KS) == [1, 3, 4, 7, 8, 15, 16, 50, 63]
    for n in (255, 256, 257, 16383, 16384, 16385):
        assert oref.finite_mask(oc.SOR[f"n{n}"][0]).sum() == n
    # the lattice: at radius 1 only the point itself is strictly inside, at the next float the six axis neighbours are too
    a, b = oc.reference("ror", "lattice_r1"), oc.reference("ror", "lattice_r1_next")
    assert (a["counts"] == 1).all() and a["n_kept"] == 0
    assert b["n_kept"] == 4 ** 3 and sorted(set(b["counts"].tolist())) == [4, 5, 6, 7]
    assert oref.r2_of(1.0) == np.float32(1.0) < oref.r2_of(oc.ROR["lattice_r1_next"][1])
    want = oc.reference("ror", "plane_min1")
    assert want["n_kept"] == want["n_finite"] == want["n_target"]
    want = oc.reference("ror", "plane_min33")
    assert (want["counts"] == 33).any() and (want["counts"] < 33).any()
    want = oc.reference("ror", "plane_min_over_n")
    assert want["n_kept"] == 0 and oc.ROR["plane_min_over_n"][2] > want["n_target"] and (want["counts"] < 631).all()
    assert oc.reference("sor", "plane_negative_mul")["n_kept"] < oc.reference("sor", "plane")["n_kept"]


def test_documented_defaults():
    assert oref.SOR_DEFAULTS == dict(mean_k=1, stddev_mul=0.0) and oref.ROR_DEFAULTS == dict(radius=0.0, min_neighbors=1)
    assert oref.MAX_MEAN_K == 63 and (oref.CHUNK, oref.GROUP) == (256, 64)


def test_large_input_forms_agree_with_brute_force():
    pts, mean_k, mul = oc.SOR["plane"]
    a, b = oc.reference("sor", "plane"), oref.statistical_large(pts, mean_k, mul)
    assert a["distances"].tobytes() == b["distances"].tobytes() and a["labels"].tobytes() == b["labels"].tobytes() and a["threshold"] == b["threshold"]
    pts, r, m = oc.ROR["plane_min33"]
    a, b = oc.reference("ror", "plane_min33"), oref.radius_large(pts, r, m)
    assert a["counts"].tobytes() == b["counts"].tobytes() and a["labels"].tobytes() == b["labels"].tobytes()
