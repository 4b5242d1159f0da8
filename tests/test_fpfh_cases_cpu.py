"""The FPFH semantics of include/ltm.h ("fpfh") shown on the restatement alone (tools/fpfh_numpy.py, no device): the theta bin rule against atan2, the bin
header against its numpy copy, a known answer, descriptors that tell an edge from a plane, the normalisation, and that the fixtures of tests/fpfh_cases.py
sit on their seams."""
import os
import subprocess

import numpy as np
import pytest

import fpfh_cases as fc
from conftest import ROOT
from tools import fpfh_numpy as fref
from tools import normals_numpy as nref

THETA_EPS = 1e-15      # rad; measured: the largest distance from a boundary at which the two rules differed was 4.45e-16 (see the test below)


def _normals(case):
    pts = case["points"]
    if case["normal"] is not None:
        return np.tile(np.float32(case["normal"]), (len(pts), 1))
    if len(pts) == 0:
        return np.zeros((0, 3), np.float32)
    return nref.estimate(pts[:, :3], fc.NORMALS_K)["normals"][:, :3]


def _boundary_distance(y, x):
    t = np.arctan2(y, x)
    boundaries = -np.pi + 2.0 * np.pi * np.arange(1, 11) / 11.0
    return np.abs(t[:, None] - boundaries[None, :]).min(axis=1)


def test_theta_rule_equals_atan2_except_at_the_boundaries():
    """On 10^6 random (x, y) the sign-test rule gives floor(11 (atan2(y, x) + pi) / (2 pi)) clamped, everywhere.  On 7 x 10^6 directions placed within
    1e-17 .. 1e-9 rad of a boundary, at radii e^-20 .. e^20, the two differ by at most one bin and only within THETA_EPS = 1e-15 rad of a boundary, the
    distance measured from numpy's arctan2 itself: the largest such distance measured was 4.45e-16 rad (2 ulp of the angle near pi; x86-64, numpy's
    arctan2), which is the rounding of cos / sin / arctan2 in making and reading the samples, not a bias of the rule.  The signed zeros follow
    atan2 (theta = +pi -> bin 10, -pi -> bin 0, +-0 -> bin 5); x == y == 0 is bin 5 by definition."""
    rng = np.random.default_rng(123)
    xy = rng.normal(size=(1_000_000, 2))
    assert (fref.bin_theta(xy[:, 1], xy[:, 0]) == fref.bin_theta_atan2(xy[:, 1], xy[:, 0])).all()
    worst = 0.0
    for scale in (1e-17, 1e-16, 3e-16, 1e-15, 1e-14, 1e-12, 1e-9):
        n = 1_000_000
        theta = -np.pi + 2.0 * np.pi * rng.integers(1, 11, n) / 11.0 + rng.uniform(-scale, scale, n)
        r = np.exp(rng.uniform(-20.0, 20.0, n))
        x, y = r * np.cos(theta), r * np.sin(theta)
        rule, ref = fref.bin_theta(y, x), fref.bin_theta_atan2(y, x)
        differ = rule != ref
        assert np.abs(rule - ref).max() <= 1
        if differ.any():
            worst = max(worst, float(_boundary_distance(y[differ], x[differ]).max()))
    print(f"largest distance from a boundary at which the rules differ: {worst:.3e} rad")
    assert worst <= THETA_EPS
    for y, x, want in ((0.0, -1.0, 10), (-0.0, -1.0, 0), (0.0, 1.0, 5), (-0.0, 1.0, 5), (0.0, 0.0, 5), (-0.0, -0.0, 5), (-0.0, 0.0, 5), (0.0, -0.0, 5),
                       (1.0, 0.0, 8), (-1.0, 0.0, 2)):
        assert int(fref.bin_theta(np.float64(y), np.float64(x))) == want, (y, x)
        if (x, y) != (0.0, 0.0):
            assert int(fref.bin_theta_atan2(np.float64(y), np.float64(x))) == want, (y, x)


BINS_PROGRAM = r"""
#include "ltm_fpfh_bins.h"
#include <cstdio>
#include <vector>
int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    double v[2];
    while (std::fread(v, sizeof(double), 2, in) == 2) {
        const unsigned char b[2] = {(unsigned char)ltm::fpfh_bin_theta(v[0], v[1]), (unsigned char)ltm::fpfh_bin_unit(v[0])};
        std::fwrite(b, 1, 2, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
"""


def test_the_bin_header_equals_its_numpy_copy(tmp_path):
    """lt-mapper_amd/csrc/ltm_fpfh_bins.h, the header the kernel includes, compiled alone for the host under the address and undefined-behaviour sanitizers: on
    random values, values at the bin edges and signed zeros it gives the bins of tools/fpfh_numpy.py"""
    src = tmp_path / "bins.cpp"
    src.write_text(BINS_PROGRAM)
    exe = tmp_path / "bins"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "lt-mapper_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rng = np.random.default_rng(7)
    edges = (2.0 * np.arange(0, 12) / 11.0 - 1.0)
    special = np.array([[0.0, -1.0], [-0.0, -1.0], [0.0, 1.0], [-0.0, 1.0], [0.0, 0.0], [-0.0, -0.0], [-0.0, 0.0], [0.0, -0.0], [1.0, 0.0], [-1.0, 0.0],
                        [-1.5, 2.0], [1.5, -2.0], [np.inf, 1.0], [-np.inf, 1.0]])
    near = np.concatenate([np.nextafter(edges, -2.0), edges, np.nextafter(edges, 2.0)])
    theta = -np.pi + 2.0 * np.pi * rng.integers(1, 11, 20000) / 11.0 + rng.uniform(-1e-15, 1e-15, 20000)
    v = np.concatenate([rng.uniform(-1.2, 1.2, (50000, 2)), special, np.column_stack([near, rng.uniform(-1.0, 1.0, len(near))]),
                        np.column_stack([np.sin(theta), np.cos(theta)])]).astype(np.float64)
    (tmp_path / "in.bin").write_bytes(np.ascontiguousarray(v).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8).reshape(-1, 2)
    assert len(got) == len(v)
    assert (got[:, 0] == fref.bin_theta(v[:, 0], v[:, 1])).all()
    assert (got[:, 1] == fref.bin_unit(v[:, 0])).all()
    table = open(os.path.join(ROOT, "lt-mapper_amd", "csrc", "ltm_fpfh_bins.h")).read()
    header = open(os.path.join(ROOT, "include", "ltm.h")).read()
    for c, s in fref.THETA_TABLE:      # the table as printed in both headers
        for value in (c, s):
            assert repr(abs(value)) in table and repr(abs(value)) in header, value
    want = [(np.cos(-np.pi + 2.0 * np.pi * j / 11.0), np.sin(-np.pi + 2.0 * np.pi * j / 11.0)) for j in range(1, 11)]
    assert np.abs(np.array(fref.THETA_TABLE) - np.array(want)).max() <= 2.3e-16      # the nearest doubles, give or take the rounding of this line's cos / sin


def test_known_answer_on_the_lattice_plane():
    """Points of the plane z = 0 with normals (0, 0, 1).  For a pair (p, q): d = q - p lies in the plane, so a1 = n.d / |d| = 0 and a2 = 0; no swap, u = n,
    phi = a1 = 0 -> floor(11 * 0.5) = bin 5 of phi (entry 16).  v = d x u = (d.y, -d.x, 0) / |d| is in the plane, so alpha = v.n = 0 -> bin 5 of alpha (entry
    5).  w = u x v is in the plane too, so y = w.n = 0 and x = u.n = 1: theta = 0 -> floor(11 * pi / (2 pi)) = bin 5 of theta (entry 27).  Every SPFH thus has
    all its pairs in those three bins, every weighted sum too, and each group scales to exactly 100.0 there and 0 elsewhere -- for every point, the border
    included, since no step looked at where the neighbours lie in the plane."""
    xyz = fc.lattice_plane()
    normals = np.tile(np.float32([0.0, 0.0, 1.0]), (len(xyz), 1))
    for k in (5, 9, 17):
        r = fref.fpfh(xyz.astype(np.float32), normals, k)
        want = np.zeros(33, np.float32)
        want[[5, 16, 27]] = 100.0
        interior = fc.lattice_interior(xyz, 2)
        assert interior.sum() == 64
        assert (r["descriptors"][interior] == want[None, :]).all()
        assert (r["descriptors"] == want[None, :]).all()
        assert (r["spfh_counts"][:, [5, 16, 27]] == k - 1).all() and r["spfh_counts"].sum() == 3 * (k - 1) * len(xyz) and r["pairs_skipped"] == 0


def test_descriptors_tell_the_edge_from_the_plane():
    """Two planes meeting at a right angle, hand normals, k = 12.  The 42 points next to the edge against the 462 points at least 1.0 (ten steps) from it, whose
    neighbours' neighbourhoods are all in one plane: the smallest L2 distance between a descriptor of the first group and one of the second, measured with the
    restatement, is 98.79; asserted: half of it.  The interior descriptors are all the planar known answer."""
    xyz, normals, dist = fc.edge_scene()
    r = fref.fpfh(xyz.astype(np.float32), normals.astype(np.float32), 12)
    d = r["descriptors"].astype(np.float64)
    edge, interior = d[dist <= 1e-9], d[dist >= 1.0 - 1e-9]
    assert (len(edge), len(interior)) == (42, 462)
    gap = np.sqrt(((edge[:, None, :] - interior[None, :, :]) ** 2).sum(axis=2)).min()
    print(f"smallest edge-to-interior descriptor distance: {gap:.4f}")
    assert gap >= 98.79 / 2
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    assert (interior == want[None, :]).all()


@pytest.mark.parametrize("name", fc.ALL)
def test_groups_sum_to_100_or_are_zero(name):
    """every group of every finite row: 11 floats, each within half an ulp of a value <= 100 (2^-24 * 100 relative to the group's scale), around a double sum
    that is 100 to 1e-13: |sum - 100| <= 11 * 100 * 2^-24 = 6.6e-5; or all zero.  NaN rows are whole rows, where the point or its normal is not finite"""
    case = fc.CASES[name]
    pts, normals = case["points"], _normals(case)
    r = fref.fpfh(pts, normals, case["k"])
    d = r["descriptors"]
    assert d.shape == (len(pts), 33) and r["spfh_counts"].shape == (len(pts), 33) and r["spfh_counts"].max(initial=0) <= 63
    nan_row = np.isnan(d).any(axis=1)
    assert (np.isnan(d).all(axis=1) == nan_row).all()
    degenerate = ~(np.isfinite(pts[:, :3]).all(axis=1) & np.isfinite(normals).all(axis=1))
    assert (nan_row == degenerate).all() and not r["spfh_counts"][nan_row].any()
    groups = d[~nan_row].astype(np.float64).reshape(-1, 3, 11)
    sums = groups.sum(axis=2)
    zero = (groups == 0.0).all(axis=2)
    assert (zero | (np.abs(sums - 100.0) <= 11 * 100.0 * 2.0 ** -24)).all()
    assert (groups >= 0.0).all()
    counts = r["spfh_counts"].reshape(-1, 3, 11).sum(axis=2)
    assert (counts[:, 0] == counts[:, 1]).all() and (counts[:, 0] == counts[:, 2]).all()      # one increment per feature per pair


def test_the_fixtures_sit_on_their_seams():
    c = fc.CASES["coincident_500"]
    r = fref.fpfh(c["points"], _normals(c), c["k"])
    assert r["pairs_skipped"] == c["k"] * 499 and not r["spfh_counts"].any() and (r["descriptors"] == 0.0).all()      # every pair skipped, all-zero groups
    c = fc.CASES["line_normals_along"]
    r = fref.fpfh(c["points"], _normals(c), c["k"])
    assert r["pairs_skipped"] == 40 * (c["k"] - 1) and (r["descriptors"] == 0.0).all()      # d is along u in every pair: |v| == 0
    c = fc.CASES["duplicates"]
    r = fref.fpfh(c["points"], _normals(c), c["k"])
    assert r["pairs_skipped"] == 80 and np.isfinite(r["descriptors"]).all() and (r["descriptors"].sum(axis=1) > 299.0).all()      # d2 == 0 with another index
    for name in ("one_point", "two_points", "all_non_finite"):      # fewer than 3 finite points: NaN normals, NaN rows
        c = fc.CASES[name]
        r = fref.fpfh(c["points"], _normals(c), c["k"])
        assert np.isnan(r["descriptors"]).all() and not r["spfh_counts"].any()
    c = fc.CASES["two_finite_among_non_finite"]
    r = fref.fpfh(c["points"], _normals(c), c["k"])
    assert r["n_finite"] == 2 and np.isfinite(r["descriptors"]).all(axis=1).sum() == 2 and r["spfh_counts"].sum() == 6
    assert len(fc.CASES["non_finite_mixed"]["points"]) == 300 and [len(fc.CASES[f"n{n}"]["points"]) for n in (255, 256, 257)] == [255, 256, 257]
    assert set(fc.BATCH) <= set(fc.ALL) and len(fc.CASES["empty"]["points"]) == 0
    with pytest.raises(ValueError):
        fref.fpfh(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), 1)
    with pytest.raises(ValueError):
        fref.fpfh(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), 65)


@pytest.mark.parametrize("name", ("blob_k8", "plane_k32", "non_finite_mixed", "sphere_shell"))
def test_a_permuted_input_gives_permuted_rows(name):
    """no distance ties in these scenes, so the neighbourhoods do not depend on the rows' order and every value follows its point, bit for bit"""
    case = fc.CASES[name]
    pts, normals = case["points"], _normals(case)
    r = fref.fpfh(pts, normals, case["k"])
    q = np.random.default_rng(5).permutation(len(pts))
    r2 = fref.fpfh(pts[q], normals[q], case["k"])
    assert r2["descriptors"].tobytes() == r["descriptors"][q].tobytes()
    assert (r2["spfh_counts"] == r["spfh_counts"][q]).all()


@pytest.mark.parametrize("name", ("blob_k17", "plane", "duplicates", "coincident_500", "lattice_plane"))
def test_neighbourhoods_agree_with_the_normals_restatement(name):
    case = fc.CASES[name]
    xyz = np.ascontiguousarray(case["points"][:, :3])
    kk = min(case["k"], len(xyz))
    nb, d2 = fref.neighbours(xyz, kk)
    assert (nb == nref.neighbours(xyz, kk)).all()
    assert (np.diff(d2, axis=1) >= 0.0).all()
    assert (fref.fpfh(xyz, _normals(case), case["k"])["neighbours"] == nb).all()
