"""CPU checks of the cluster interface (no device needed): the entry points of include/ltm.h "clusters" are declared, exported and bound and refuse bad
arguments before a device could be touched; the restatement (tools/cluster_numpy.py) is pinned independently of the kernels against an O(n^2) brute force
with a sequential union-find written here, on every fixture of tests/cluster_cases.py of at most 2000 points; the boundary fixture really sits on
d2 == r2 in float32; and the host header compiles under -Wall -Wextra -Werror, links and runs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
from conftest import ROOT
from tools import cluster_numpy as cref

ENTRY_POINTS = ("ltm_cluster_default_params", "ltm_search_cluster", "ltm_clusters_info", "ltm_clusters_device", "ltm_clusters_download", "ltm_clusters_extract",
                "ltm_clusters_free", "ltm_debug_cluster_stats")


def test_header_declares_and_library_exports_the_entry_points(ltm):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltm.h")).read(), flags=re.S)
    lib = ltm.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} not declared in include/ltm.h"
        assert hasattr(lib, name), f"{name} not exported by libltm_hip.so"
        assert name in ltm.SIGNATURES
    assert lib.ltm_abi_version() == 1
    assert C.sizeof(ltm.ClusterParams) == 16
    p = ltm.ClusterParams(9.0, 9, 9)
    lib.ltm_cluster_default_params(C.byref(p))
    assert (p.tolerance, p.min_size, p.max_size) == (0.0, 1, 0)      # PCL: tolerance must be set, 1, no limit
    for name in ("info", "labels", "indices", "extract", "close", "sizes", "first_index", "boxes", "centroids"):
        assert hasattr(ltm.Clusters, name)
    assert hasattr(ltm.SearchIndex, "cluster") and hasattr(ltm.Context, "cluster")


def test_argument_errors_need_no_device(ltm):
    lib = ltm.load_library()
    p = ltm.ClusterParams(0.5, 1, 0)
    ih = (C.c_void_p * 1)(0x1000)
    out = (C.c_void_p * 1)()
    sz, vp, u = C.c_size_t(), C.c_void_p(), (C.c_uint64 * 6)()
    bogus = C.c_void_p(0x1000)
    assert lib.ltm_search_cluster(None, 1, ih, C.byref(p), out) == -1
    assert lib.ltm_search_cluster(None, 1, None, None, None) == -1
    assert lib.ltm_clusters_info(None, bogus, C.byref(sz), C.byref(sz), C.byref(sz)) == -1
    assert lib.ltm_clusters_device(None, bogus, C.byref(vp), C.byref(vp), C.byref(vp)) == -1
    assert lib.ltm_clusters_download(None, bogus, None, None, None, None, None) == -1
    assert lib.ltm_clusters_extract(None, bogus, 1, C.byref(C.c_uint64())) == -1
    assert lib.ltm_clusters_free(None, bogus) == -1
    assert lib.ltm_clusters_free(None, None) == -1
    assert lib.ltm_debug_cluster_stats(None, u, 0) == -1
    assert out[0] is None
    # the Python surface checks its arguments before it calls the library
    ctx = object.__new__(ltm.Context)
    idx = ltm.SearchIndex(ctx, None)
    for tol in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ltm.Context.cluster(ctx, [idx], tol)
        with pytest.raises(ValueError):
            ltm.SearchIndex.cluster(idx, tol)
    for lo, hi in ((0, None), (5, 4), (-1, None), (1, -2)):
        with pytest.raises(ValueError):
            ltm.Context.cluster(ctx, [idx], 0.5, min_size=lo, max_size=hi)
    for bad in (np.zeros((4, 3), np.float32), None, object()):
        with pytest.raises(TypeError):
            ltm.Context.cluster(ctx, [idx, bad], 0.5)
    idx.h = None      # nothing to free


def brute_force(pts, tol, lo, hi):
    """the section "clusters" of include/ltm.h restated without scipy: all pairs in float32, a sequential union-find, the filter and the canonical order"""
    xyz = np.asarray(pts, np.float32)[:, :3]
    n = len(xyz)
    r2 = np.float32(np.float64(tol) * np.float64(tol))
    fin = np.isfinite(xyz).all(axis=1)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in range(n):
        if not fin[i] or i == 0:
            continue
        d = xyz[i] - xyz[:i]
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ri = find(i)
        for j in np.flatnonzero((d2 < r2) & fin[:i]):
            rj = find(int(j))
            if rj != ri:
                parent[max(ri, rj)] = min(ri, rj)
                ri = min(ri, rj)
    comps = {}
    for i in range(n):
        if fin[i]:
            comps.setdefault(find(i), []).append(i)
    kept = [m for m in comps.values() if len(m) >= lo and (hi is None or len(m) <= hi)]
    kept.sort(key=lambda m: (-len(m), m[0]))
    labels = np.full(n, -1, np.int32)
    for c, m in enumerate(kept):
        labels[m] = c
    return labels, kept


@pytest.mark.parametrize("name", cc.SMALL)
def test_restatement_equals_brute_force(name):
    pts, tol, lo, hi = cc.CASES[name]
    got = cc.reference(name)
    labels, kept = brute_force(pts, tol, lo, hi)
    assert (got["labels"] == labels).all()
    assert got["sizes"].tolist() == [len(m) for m in kept]
    assert got["first"].tolist() == [m[0] for m in kept]
    assert got["offsets"].tolist() == np.cumsum([0] + [len(m) for m in kept]).tolist()
    assert got["idx"].tolist() == [i for m in kept for i in m]
    xyz = np.asarray(pts, np.float32)[:, :3]
    for c, m in enumerate(kept):
        assert (got["boxes"][c, :3] == xyz[m].min(axis=0)).all() and (got["boxes"][c, 3:] == xyz[m].max(axis=0)).all()
        mean = np.array([sum(float(v) for v in xyz[m, d]) / len(m) for d in range(3)])      # plain left-to-right double sum
        bound = len(m) * 2.0 ** -52 * max(float(np.abs(xyz[m]).max()), 1e-300)
        assert np.abs(got["centroids"][c] - mean).max() <= bound


def test_fixtures_are_what_they_claim():
    a, b = cc.CASES["boundary_equal"][0], cc.CASES["boundary_below"][0]
    r2 = cref.r2_of(0.5)
    assert r2 == np.float32(0.25)
    assert cref.d2_float32(a[:1, :3], a[1:, :3])[0] == r2                        # exactly on the boundary: strict <, not adjacent
    assert cref.d2_float32(b[:1, :3], b[1:, :3])[0] < r2
    assert len(cc.reference("boundary_equal")["sizes"]) == 2 and cc.reference("boundary_below")["sizes"].tolist() == [2]
    assert cc.reference("chain_5000")["sizes"].tolist() == [5000]
    assert cc.reference("two_chains")["sizes"].tolist() == [5000, 5000]
    assert cc.reference("duplicates")["sizes"].tolist() == [1000, 1000]
    assert cc.reference("tolerance_above_cloud")["sizes"].tolist() == [1500]
    assert (cc.reference("tolerance_below_pairs")["sizes"] == 1).all() and len(cc.reference("tolerance_below_pairs")["sizes"]) == 1728
    assert sorted(cc.reference("filter_seams")["sizes"].tolist()) == [5, 7, 9]
    eq = cc.reference("equal_sizes")
    assert eq["sizes"].tolist() == [12, 8, 8, 8, 8, 8, 8, 3] and (np.diff(eq["first"][1:7]) > 0).all()      # the tie rule decides among the six
    for name in ("empty", "all_nonfinite"):
        assert len(cc.reference(name)["sizes"]) == 0 and (cc.reference(name)["labels"] == -1).all()
    mixed = cc.CASES["nonfinite_mixed"][0]
    bad = ~np.isfinite(mixed[:, :3]).all(axis=1)
    assert bad.sum() > 50 and (cc.reference("nonfinite_mixed")["labels"][bad] == -1).all()
    assert len(cc.reference("blobs")["sizes"]) >= 15 and (cc.reference("blobs")["labels"] == -1).sum() > 100
    for name, (pts, _, _, _) in cc.CASES.items():      # permuted: original index is not the generation order
        if len(pts) > 2:
            assert (np.diff(pts[:, 3]) != 1).any(), name


PROGRAM = r"""
#include "removert/DeviceEuclideanClusterExtraction.h"
#include <cstdio>

int main()
{
    ltm_cluster_params p;
    ltm_cluster_default_params(&p);
    std::printf("defaults %.1f %u %u\n", p.tolerance, p.min_size, p.max_size);
    ltm_config cfg{};
    cfg.vfov = 50.0f; cfg.hfov = 360.0f;
    for (int i = 0; i < 16; ++i) cfg.lidar2base[i] = (i % 5 == 0) ? 1.0 : 0.0;
    ltm_ctx* ctx = nullptr;
    const int rc = ltm_create(&cfg, &ctx);
    if (rc != LTM_OK) { std::printf("no device: %d\n", rc); return 0; }
    {
        // 5 points 0.25 apart, a gap, 3 points 0.25 apart, a gap, one point alone
        ltremovert::Cloud cloud;
        for (int i = 0; i < 3; ++i) cloud.push_back(ltremovert::PointType{10.0f + 0.25f * (float)i, 0.0f, 0.0f, 0.0f});
        cloud.push_back(ltremovert::PointType{20.0f, 0.0f, 0.0f, 0.0f});
        for (int i = 0; i < 5; ++i) cloud.push_back(ltremovert::PointType{0.25f * (float)i, 0.0f, 0.0f, 0.0f});
        ltremovert::DeviceEuclideanClusterExtraction ec(ctx);
        ec.setClusterTolerance(0.5);
        ec.setMinClusterSize(2);
        ec.setInputCloud(cloud);
        std::vector<ltremovert::PointIndices> clusters;
        ec.extract(clusters);
        std::printf("clusters %zu sizes %zu %zu first %d %d labels %d %d %d\n", clusters.size(), clusters[0].indices.size(), clusters[1].indices.size(),
                    clusters[0].indices[0], clusters[1].indices[0], ec.labels()[0], ec.labels()[3], ec.labels()[8]);
        std::vector<std::vector<ltremovert::PointIndices>> many;
        ltremovert::Cloud none;
        ec.extract({&cloud, &none, &cloud}, many);
        std::printf("batch %zu: %zu %zu %zu tolerance %.2f min %d\n", many.size(), many[0].size(), many[1].size(), many[2].size(), ec.getClusterTolerance(),
                    ec.getMinClusterSize());
    }
    ltm_destroy(ctx);
    return 0;
}
"""


def test_device_cluster_header_compiles_and_links(tmp_path, ltm):
    ltm.load_library()
    src = tmp_path / "cluster_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "cluster_user"
    pkg = os.path.join(ROOT, "lt-mapper_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", pkg, "-lltm_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "defaults 0.0 1 0" in r.stdout, r.stdout
    import torch
    if torch.cuda.is_available():
        assert "clusters 2 sizes 5 3 first 4 0 labels 1 -1 0" in r.stdout, r.stdout
        assert "batch 3: 2 0 2 tolerance 0.50 min 2" in r.stdout, r.stdout
    else:
        assert "no device" in r.stdout, r.stdout
