"""The plane restatement (tools/plane_numpy.py) pinned without a device: against an independent brute force written here from include/ltm.h, "planes" -- plain
Python loops over hypotheses and points in float64, no numpy broadcasting -- on every fixture of tests/plane_cases.py of at most 2000 points (hypotheses, valid
bytes, counts, best, labels); and the fixtures are what they claim.  Also measured here: how far the order of the moment sums moves the coefficients, the
figure behind the tolerance of tests/test_gpu_plane.py."""
import math

import numpy as np
import pytest

import plane_cases as pc
from tools import plane_numpy as pref


def _mix(seed, h, j):
    x = (seed + 0x9E3779B9 * (3 * h + j + 1)) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xffffffff
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xffffffff
    x ^= x >> 16
    return x


def brute_force(pts, p):
    """hypotheses, valid bytes, counts and the best hypothesis, one point at a time"""
    q = [(float(r[0]), float(r[1]), float(r[2])) for r in np.asarray(pts, np.float32)]
    fin = [all(math.isfinite(v) for v in r) for r in q]
    live = [r for r, f in zip(q, fin) if f]
    n, H, thr, ax = len(q), p["max_iterations"], p["distance_threshold"], p["axis"]
    constrained = any(v != 0.0 for v in ax) and p["eps_angle"] < 1.5707963267948966
    c2 = math.cos(p["eps_angle"]) ** 2 if constrained else 0.0
    idx, valid, counts, hyp = [], [], [], []
    for h in range(H):
        s = [(_mix(p["seed"], h, j) * n) >> 32 for j in range(3)]
        idx.append(s)
        ok = len(set(s)) == 3 and all(fin[k] for k in s)
        N = p0 = T = None
        if ok:
            p0, p1, p2 = q[s[0]], q[s[1]], q[s[2]]
            u = [p1[k] - p0[k] for k in range(3)]
            v = [p2[k] - p0[k] for k in range(3)]
            N = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
            n2 = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]
            ok = n2 > 0.0 and math.isfinite(n2)
            if ok and constrained:
                dot = (N[0] * ax[0] + N[1] * ax[1]) + N[2] * ax[2]
                ok = dot * dot >= (c2 * n2) * ((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2])
            T = (thr * thr) * n2
        valid.append(1 if ok else 0)
        hyp.append((N, p0, T) if ok else None)
        c = 0
        if ok:
            Nx, Ny, Nz = N
            ox, oy, oz = p0
            for x, y, z in live:
                s_ = (Nx * (x - ox) + Ny * (y - oy)) + Nz * (z - oz)
                if s_ * s_ < T:
                    c += 1
        counts.append(c)
    best = -1
    for h in range(H):
        if valid[h] and (best < 0 or counts[h] > counts[best]):
            best = h
    return idx, valid, counts, hyp, best, fin


def brute_labels(pts, fin, coeff, point, thr):
    out = []
    for r, f in zip(np.asarray(pts, np.float32), fin):
        e = [float(r[k]) - float(point[k]) for k in range(3)]
        out.append(1 if f and abs((float(coeff[0]) * e[0] + float(coeff[1]) * e[1]) + float(coeff[2]) * e[2]) < thr else 0)
    return out


@pytest.mark.parametrize("name", pc.SMALL)
def test_restatement_equals_brute_force(name):
    pts, p = pc.CASES[name]
    got = pc.reference(name)
    idx, valid, counts, hyp, best, fin = brute_force(pts, p)
    assert got["hyps"]["idx"].tolist() == idx
    assert got["valid"].tolist() == valid
    assert got["counts"].dtype == np.uint32 and got["counts"].tolist() == counts
    for h, t in enumerate(hyp):
        if t is not None:
            assert got["hyps"]["N"][h].tolist() == list(t[0]) and got["hyps"]["p0"][h].tolist() == list(t[1]) and got["hyps"]["T"][h] == t[2]
    assert got["best"] == best and got["found"] == (1 if best >= 0 else 0)
    assert got["n_valid"] == sum(valid) and got["consensus"] == (counts[best] if best >= 0 else 0)
    if best < 0:
        assert np.isnan(got["coeff"]).all() and np.isnan(got["point"]).all() and not got["labels"].any()
    else:
        assert got["labels"].tolist() == brute_labels(pts, fin, got["coeff"], got["point"], p["distance_threshold"])
        assert abs(float(np.dot(got["coeff"][:3], got["coeff"][:3])) - 1.0) < 1e-14
        assert abs(float(np.dot(got["coeff"][:3], got["point"])) + got["coeff"][3]) <= 1e-12 * max(1.0, float(np.abs(got["point"]).max()))
    assert got["n_inliers"] == int(got["labels"].sum())


def test_fixtures_are_what_they_claim():
    for name in ("empty", "one_point", "two_points", "all_nonfinite", "coincident", "collinear"):
        r = pc.reference(name)
        assert r["found"] == 0 and r["n_valid"] == 0 and not r["counts"].any(), name
    assert pc.reference("three_points")["consensus"] == 3
    # collinear: every draw of three distinct points gives N = 0 exactly, not merely small
    pts, p = pc.CASES["collinear"]
    idx = pc.reference("collinear")["hyps"]["idx"]
    distinct = [s for s in idx.tolist() if len(set(s)) == 3]
    assert len(distinct) > 100
    for s in distinct:
        a, b, c = (pts[k, :3].astype(np.float64) for k in s)
        assert not np.cross(b - a, c - a).any()
    mixed = pc.CASES["nonfinite_mixed"][0]
    bad = ~np.isfinite(mixed[:, :3]).all(axis=1)
    r = pc.reference("nonfinite_mixed")
    assert bad.sum() > 50 and not r["labels"][bad].any() and 0 < r["n_valid"] < 128      # some hypotheses drew a non-finite point
    for name, (pts, _) in pc.CASES.items():      # permuted: the position is not the generation order
        if len(pts) > 3:
            assert (np.diff(pts[:, 3]) != 1).any(), name


def test_the_boundary_pair_sits_on_and_one_step_below_T():
    pts, p = pc.CASES["lattice_boundary"]
    r = pc.reference("lattice_boundary")
    on = int(np.flatnonzero(pts[:, 2] == np.float32(0.5))[0])
    below = int(np.flatnonzero((pts[:, 2] != 0) & (pts[:, 2] != np.float32(0.5)))[0])
    assert pts[below, 2] == np.nextafter(np.float32(0.5), np.float32(0))
    v = np.flatnonzero(r["valid"])
    assert len(v) >= 32
    ks = set()
    for h in v:
        N, p0, T = r["hyps"]["N"][h], r["hyps"]["p0"][h], r["hyps"]["T"][h]
        assert N[0] == 0.0 and N[1] == 0.0 and N[2] == round(N[2]) and N[2] != 0.0      # N = (0, 0, +-k)
        ks.add(abs(int(N[2])))
        s_on = N[2] * (float(pts[on, 2]) - p0[2])
        s_below = N[2] * (float(pts[below, 2]) - p0[2])
        assert s_on * s_on == T and s_below * s_below < T      # exactly on T (out, strict <) and below it (in)
        assert r["counts"][h] == 401
    assert len(ks) > 3
    assert r["labels"][on] == 0 and r["labels"][below] == 1 and r["n_inliers"] == 401 and r["refined"] == 0


def test_wall_and_ground_needs_the_axis():
    free, axis = pc.reference("wall_and_ground"), pc.reference("wall_and_ground_axis")
    assert free["found"] and abs(free["coeff"][0]) > 0.99 and abs(free["coeff"][3] + 8.0) < 0.05 and free["consensus"] > 1900      # the wall x = 8
    assert axis["found"] and axis["coeff"][2] > 0.99 and abs(axis["coeff"][3] - 1.9) < 0.05 and 1500 < axis["consensus"] < 1900    # the ground z = -1.9
    assert free["n_valid"] == 128 and 0 < axis["n_valid"] < 64
    assert (axis["valid"] <= free["valid"]).all()
    assert (axis["counts"][axis["valid"] == 1] == free["counts"][axis["valid"] == 1]).all()


def test_equal_support_ties_and_the_smaller_h_wins():
    pts, p = pc.CASES["equal_support"]
    r = pc.reference("equal_support")
    top = np.flatnonzero((r["counts"] == r["counts"].max()) & (r["valid"] == 1))
    assert r["counts"].max() == 225 and len(top) >= 2
    planes = {float(r["hyps"]["p0"][h][2]) for h in top}
    assert planes == {0.0, 10.0}                      # hypotheses on both planes reach the same count
    assert r["best"] == int(top[0]) and r["consensus"] == 225
    first_other = next(int(h) for h in top if r["hyps"]["p0"][h][2] != r["hyps"]["p0"][top[0]][2])
    assert first_other > r["best"]
    assert abs(r["coeff"][2]) == 1.0 and -r["coeff"][3] == r["hyps"]["p0"][r["best"]][2]
    assert r["labels"].sum() == 225


def coefficient_spread():
    """the largest difference of a coefficient or plane-point component, over the fixtures, between the moment sums in the fixed shape and in three random
    orders; and the same for the unrefined coefficients against numpy's own normalisation"""
    worst_refined = worst_unrefined = 0.0
    for name, (pts, p) in pc.CASES.items():
        r = pc.reference(name)
        if not r["found"]:
            continue
        scale = max(1.0, float(np.abs(r["point"]).max()))
        c0, q0, ref0 = pref.refine(pts, r["hyps"], r["best"], r["consensus"], p)
        for k in range(3):
            perm = np.random.default_rng(1000 + k).permutation(len(pts))
            c1, q1, ref1 = pref.refine(pts, r["hyps"], r["best"], r["consensus"], p, perm=perm)
            assert ref1 == ref0, name
            worst_refined = max(worst_refined, float(np.abs(c1[:3] - c0[:3]).max()), float(np.abs(c1[3] - c0[3])) / scale,
                                float(np.abs(q1 - q0).max()) / scale)
        cu, qu = pref.unrefined(r["hyps"], r["best"], p)
        N = r["hyps"]["N"][r["best"]]
        nn = N / np.linalg.norm(N)
        nn = nn * np.sign(np.dot(nn, cu[:3]))
        worst_unrefined = max(worst_unrefined, float(np.abs(nn - cu[:3]).max()), abs(float(-np.dot(nn, qu)) - cu[3]) / scale)
    return worst_refined, worst_unrefined


def test_the_tolerance_of_the_device_test_is_the_measured_one():
    from test_gpu_plane import COEFF_TOL_REFINED, COEFF_TOL_UNREFINED, MEASURED_REFINED, MEASURED_UNREFINED
    refined, unref = coefficient_spread()
    print(f"coefficient spread over the order of the moment sums: refined {refined:.3e}, unrefined {unref:.3e}")
    assert refined <= MEASURED_REFINED and unref <= MEASURED_UNREFINED      # what DESIGN.md 4.10 records still holds
    assert COEFF_TOL_REFINED == 100.0 * MEASURED_REFINED and COEFF_TOL_UNREFINED == 100.0 * MEASURED_UNREFINED
