"""CPU checks of the outlier-filter interface (no device needed): the entry points of include/ltm.h "outlier filters" are declared, exported and bound; the
parameter structs and their defaults are as stated; bad arguments are refused before a device could be touched, by the library and by the Python surface; and
the host header DeviceOutlierRemoval.h compiles under -Wall -Wextra -Werror, links and runs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tools import outlier_numpy as oref

ENTRY_POINTS = ("ltm_sor_default_params", "ltm_ror_default_params", "ltm_search_filter_statistical", "ltm_search_filter_radius", "ltm_outliers_info",
                "ltm_outliers_device", "ltm_outliers_download", "ltm_outliers_split_scanset", "ltm_outliers_split_cloud", "ltm_outliers_free",
                "ltm_debug_outlier_stats")


def test_header_declares_and_library_exports_the_entry_points(ltm):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltm.h")).read(), flags=re.S)
    lib = ltm.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} not declared in include/ltm.h"
        assert hasattr(lib, name), f"{name} not exported by libltm_hip.so"
        assert name in ltm.SIGNATURES
    assert lib.ltm_abi_version() == 1
    assert re.search(r"#define\s+LTM_OUTLIERS_STATISTICAL\s+0\b", src) and re.search(r"#define\s+LTM_OUTLIERS_RADIUS\s+1\b", src)
    assert (ltm.OUTLIERS_STATISTICAL, ltm.OUTLIERS_RADIUS) == (0, 1)
    assert C.sizeof(ltm.SorParams) == 16 and C.sizeof(ltm.RorParams) == 16
    assert (ltm.SorParams.mean_k.offset, ltm.SorParams.stddev_mul.offset, ltm.RorParams.radius.offset, ltm.RorParams.min_neighbors.offset) == (0, 8, 0, 8)
    s = ltm.SorParams(9, 9.0)
    lib.ltm_sor_default_params(C.byref(s))
    assert dict(mean_k=s.mean_k, stddev_mul=s.stddev_mul) == oref.SOR_DEFAULTS
    r = ltm.RorParams(9.0, 9)
    lib.ltm_ror_default_params(C.byref(r))
    assert dict(radius=r.radius, min_neighbors=r.min_neighbors) == oref.ROR_DEFAULTS
    lib.ltm_sor_default_params(None)
    lib.ltm_ror_default_params(None)
    assert ltm.SOR_MAX_MEAN_K == oref.MAX_MEAN_K
    for name in ("info", "kind", "n_target", "n_finite", "n_kept", "mean", "stddev", "threshold", "offsets", "labels", "distances", "counts", "split", "close",
                 "__enter__", "__exit__"):
        assert hasattr(ltm.Outliers, name)
    for name in ("statistical_outliers", "radius_outliers", "outlier_stats"):
        assert hasattr(ltm.Context, name)
    for name in ("statistical_outliers", "radius_outliers"):
        assert hasattr(ltm.SearchIndex, name)
    q = ltm.sor_params(50, -1.5)
    assert (q.mean_k, q.stddev_mul) == (50, -1.5)
    q = ltm.ror_params(0.25)
    assert (q.radius, q.min_neighbors) == (0.25, 1)


def test_argument_errors_need_no_device(ltm):
    lib = ltm.load_library()
    s, r = ltm.sor_params(8, 1.0), ltm.ror_params(0.5, 2)
    idx = (C.c_void_p * 1)(0x1000)
    sz, kind, vp, u = C.c_size_t(), C.c_int(), C.c_void_p(), (C.c_uint64 * 4)()
    a, b = C.c_uint64(7), C.c_uint64(7)
    bogus = C.c_void_p(0x1000)
    out = C.c_void_p(0x1234)
    assert lib.ltm_search_filter_statistical(None, 1, idx, C.byref(s), C.byref(out)) == -1 and out.value is None      # no handle is returned
    out = C.c_void_p(0x1234)
    assert lib.ltm_search_filter_radius(None, 1, idx, C.byref(r), C.byref(out)) == -1 and out.value is None
    assert lib.ltm_search_filter_statistical(None, 0, None, None, None) == -1
    assert lib.ltm_search_filter_radius(None, 0, None, None, None) == -1
    assert lib.ltm_outliers_info(None, bogus, C.byref(kind), C.byref(sz), C.byref(sz)) == -1
    assert lib.ltm_outliers_device(None, bogus, C.byref(vp), C.byref(vp), C.byref(vp), C.byref(vp)) == -1
    assert lib.ltm_outliers_download(None, bogus, *([None] * 9)) == -1
    assert lib.ltm_outliers_split_scanset(None, bogus, 1, C.byref(a), C.byref(b)) == -1
    assert lib.ltm_outliers_split_cloud(None, bogus, 1, C.byref(a), C.byref(b)) == -1
    assert lib.ltm_outliers_free(None, bogus) == -1
    assert lib.ltm_outliers_free(None, None) == -1
    assert lib.ltm_debug_outlier_stats(None, u, 0) == -1
    assert (a.value, b.value) == (7, 7)


def test_python_surface_raises_before_it_calls_the_library(ltm):
    ctx = object.__new__(ltm.Context)      # no library handle: any call into it would fail with AttributeError, not ValueError
    index = ltm.SearchIndex(ctx, 0)
    nan, inf = float("nan"), float("inf")
    for mean_k in (0, -1, 64, 1.5, 2 ** 32):
        with pytest.raises(ValueError):
            ltm.Context.statistical_outliers(ctx, [index], mean_k, 1.0)
        with pytest.raises(ValueError):
            index.statistical_outliers(mean_k, 1.0)
    for mul in (nan, inf, -inf):
        with pytest.raises(ValueError):
            ltm.Context.statistical_outliers(ctx, [index], 8, mul)
    for radius in (0.0, -1.0, nan, inf):
        with pytest.raises(ValueError):
            ltm.Context.radius_outliers(ctx, [index], radius, 2)
        with pytest.raises(ValueError):
            index.radius_outliers(radius)
    for m in (0, -3, 2.5, 2 ** 32):
        with pytest.raises(ValueError):
            ltm.Context.radius_outliers(ctx, [index], 0.5, m)
    for bad in ([np.zeros((4, 4), np.float32)], [None], [ltm.Cloud(ctx, 0)], [index, object()]):
        with pytest.raises(TypeError):
            ltm.Context.statistical_outliers(ctx, bad, 8, 1.0)
        with pytest.raises(TypeError):
            ltm.Context.radius_outliers(ctx, bad, 0.5)


PROGRAM = r"""
#include "removert/DeviceOutlierRemoval.h"
#include <cstdio>

int main()
{
    ltm_sor_params s;
    ltm_ror_params r;
    ltm_sor_default_params(&s);
    ltm_ror_default_params(&r);
    std::printf("defaults %u %.1f %.1f %u\n", s.mean_k, s.stddev_mul, r.radius, r.min_neighbors);
    {
        ltremovert::DeviceStatisticalOutlierRemoval sor(nullptr);
        ltremovert::DeviceRadiusOutlierRemoval ror(nullptr);
        sor.setMeanK(50);
        sor.setStddevMulThresh(1.5);
        ror.setRadiusSearch(0.8);
        ror.setMinNeighborsInRadius(2);
        int refused = 0;
        ltremovert::Cloud none;
        try { sor.filter(none); } catch (const std::logic_error&) { ++refused; }
        try { ror.filter(none); } catch (const std::logic_error&) { ++refused; }
        std::printf("refused %d mean_k %d mul %.1f radius %.1f min %d\n", refused, sor.getMeanK(), sor.getStddevMulThresh(), ror.getRadiusSearch(),
                    ror.getMinNeighborsInRadius());
    }
    ltm_config cfg{};
    cfg.vfov = 50.0f; cfg.hfov = 360.0f;
    for (int i = 0; i < 16; ++i) cfg.lidar2base[i] = (i % 5 == 0) ? 1.0 : 0.0;
    ltm_ctx* ctx = nullptr;
    const int rc = ltm_create(&cfg, &ctx);
    if (rc != LTM_OK) { std::printf("no device: %d\n", rc); return 0; }
    {
        // a 10 x 10 lattice of z = 0 with spacing 1, and two strays far above it at positions 3 and 57
        ltremovert::Cloud cloud, none;
        for (int i = 0; i < 10; ++i) for (int j = 0; j < 10; ++j) cloud.push_back(ltremovert::PointType{(float)i, (float)j, 0.0f, 0.0f});
        cloud.insert(cloud.begin() + 3, ltremovert::PointType{4.0f, 4.0f, 30.0f, 0.0f});
        cloud.insert(cloud.begin() + 57, ltremovert::PointType{5.0f, 5.0f, -40.0f, 0.0f});
        ltremovert::DeviceStatisticalOutlierRemoval sor(ctx);
        sor.setMeanK(4);
        sor.setStddevMulThresh(1.0);
        sor.setInputCloud(cloud);
        ltremovert::Cloud kept;
        sor.filter(kept);
        std::printf("sor kept %zu removed %zu: %d %d\n", kept.size(), sor.getRemovedIndices().size(), sor.getRemovedIndices()[0], sor.getRemovedIndices()[1]);
        ltremovert::DeviceRadiusOutlierRemoval ror(ctx);
        ror.setRadiusSearch(1.5);
        ror.setMinNeighborsInRadius(3);
        std::vector<ltremovert::Cloud> outs;
        std::vector<std::vector<int>> removed;
        ror.filter({&cloud, &none, &cloud}, outs, &removed);
        std::printf("ror batch %zu: %zu %zu %zu removed %zu %zu %zu first %d %d\n", outs.size(), outs[0].size(), outs[1].size(), outs[2].size(), removed[0].size(),
                    removed[1].size(), removed[2].size(), removed[0][0], removed[2][1]);
    }
    ltm_destroy(ctx);
    return 0;
}
"""


def test_device_outlier_header_compiles_and_links(tmp_path, ltm):
    ltm.load_library()
    src = tmp_path / "outlier_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "outlier_user"
    pkg = os.path.join(ROOT, "lt-mapper_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", pkg, "-lltm_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "defaults 1 0.0 0.0 1" in r.stdout, r.stdout
    assert "refused 2 mean_k 50 mul 1.5 radius 0.8 min 2" in r.stdout, r.stdout
    import torch
    if torch.cuda.is_available():
        # the strays have a mean neighbour distance of ~30 and ~40 against ~1 on the lattice; within 1.5 of a lattice point there are at least 4 points
        assert "sor kept 100 removed 2: 3 57" in r.stdout, r.stdout
        assert "ror batch 3: 100 0 100 removed 2 0 2 first 3 57" in r.stdout, r.stdout
    else:
        assert "no device" in r.stdout, r.stdout
