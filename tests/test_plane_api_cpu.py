"""CPU checks of the plane interface (no device needed): the entry points of include/ltm.h "planes" are declared, exported and bound; the parameter struct
and its defaults are as stated; bad arguments are refused before a device could be touched, by the library and by the Python surface; and the host header
DeviceSACSegmentation.h compiles under -Wall -Wextra -Werror, links and runs."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import plane_cases as pc
from conftest import ROOT

ENTRY_POINTS = ("ltm_plane_default_params", "ltm_plane_block_points", "ltm_scanset_segment_planes", "ltm_cloud_segment_plane", "ltm_planes_info",
                "ltm_planes_device", "ltm_planes_download", "ltm_planes_split_scanset", "ltm_planes_split_cloud", "ltm_planes_free", "ltm_debug_plane_stats")


def test_header_declares_and_library_exports_the_entry_points(ltm):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltm.h")).read(), flags=re.S)
    lib = ltm.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} not declared in include/ltm.h"
        assert hasattr(lib, name), f"{name} not exported by libltm_hip.so"
        assert name in ltm.SIGNATURES
    assert lib.ltm_abi_version() == 1
    assert C.sizeof(ltm.PlaneParams) == 56
    p = ltm.PlaneParams(9.0, 9, 9, (C.c_double * 3)(9.0, 9.0, 9.0), 9.0, 9)
    lib.ltm_plane_default_params(C.byref(p))
    assert (p.distance_threshold, p.max_iterations, p.seed, list(p.axis), p.eps_angle, p.refine) == (0.0, 128, 0, [0.0, 0.0, 0.0], 0.0, 1)
    lib.ltm_plane_default_params(None)
    assert ltm.plane_block_points() == pc.BLOCK_POINTS
    assert re.search(r"#define\s+LTM_PLANE_BLOCK_POINTS\s+%d\b" % pc.BLOCK_POINTS, src)
    for name in ("info", "found", "best", "consensus", "n_valid", "n_inliers", "refined", "coefficients", "points", "labels", "hypothesis_counts",
                 "hypothesis_valid", "split", "close", "__enter__", "__exit__"):
        assert hasattr(ltm.Planes, name)
    for name in ("segment_planes", "segment_plane", "plane_stats"):
        assert hasattr(ltm.Context, name)
    q = ltm.plane_params(0.1, axis=(0, 0, 1), eps_angle=math.radians(10.0), seed=5, refine=False)
    assert (q.distance_threshold, q.max_iterations, q.seed, list(q.axis), q.eps_angle, q.refine) == (0.1, 128, 5, [0.0, 0.0, 1.0], math.radians(10.0), 0)


def test_argument_errors_need_no_device(ltm):
    lib = ltm.load_library()
    p = ltm.plane_params(0.1)
    out = C.c_void_p(0x1234)
    sz, m, vp, u = C.c_size_t(), C.c_uint32(), C.c_void_p(), (C.c_uint64 * 4)()
    a, b = C.c_uint64(7), C.c_uint64(7)
    bogus = C.c_void_p(0x1000)
    assert lib.ltm_scanset_segment_planes(None, 1, 0, 1, C.byref(p), C.byref(out)) == -1 and out.value is None      # no handle is returned
    out = C.c_void_p(0x1234)
    assert lib.ltm_cloud_segment_plane(None, 1, C.byref(p), C.byref(out)) == -1 and out.value is None
    assert lib.ltm_scanset_segment_planes(None, 1, 0, 1, None, None) == -1
    assert lib.ltm_cloud_segment_plane(None, 1, None, None) == -1
    assert lib.ltm_planes_info(None, bogus, C.byref(sz), C.byref(sz), C.byref(m)) == -1
    assert lib.ltm_planes_device(None, bogus, C.byref(vp), C.byref(vp), C.byref(vp)) == -1
    assert lib.ltm_planes_download(None, bogus, *([None] * 11)) == -1
    assert lib.ltm_planes_split_scanset(None, bogus, 1, C.byref(a), C.byref(b)) == -1
    assert lib.ltm_planes_split_cloud(None, bogus, 1, C.byref(a), C.byref(b)) == -1
    assert lib.ltm_planes_free(None, bogus) == -1
    assert lib.ltm_planes_free(None, None) == -1
    assert lib.ltm_debug_plane_stats(None, u, 0) == -1
    assert (a.value, b.value) == (7, 7)


def test_python_surface_raises_before_it_calls_the_library(ltm):
    ctx = object.__new__(ltm.Context)      # no library handle: any call into it would fail with AttributeError, not ValueError
    scans = ltm.ScanSet(ctx, 0)
    cloud = ltm.Cloud(ctx, 0)
    nan, inf = float("nan"), float("inf")
    for thr in (0.0, -1.0, nan, inf):
        with pytest.raises(ValueError):
            ltm.Context.segment_planes(ctx, scans, thr)
        with pytest.raises(ValueError):
            ltm.Context.segment_plane(ctx, cloud, thr)
    for it in (0, -1, 4097, 1.5):
        with pytest.raises(ValueError):
            ltm.Context.segment_planes(ctx, scans, 0.1, max_iterations=it)
    for axis in ((0.0, 1.0), (nan, 0.0, 1.0), (0.0, inf, 0.0), (1.0, 2.0, 3.0, 4.0)):
        with pytest.raises(ValueError):
            ltm.Context.segment_planes(ctx, scans, 0.1, axis=axis)
    for eps in (-0.1, nan, inf):
        with pytest.raises(ValueError):
            ltm.Context.segment_planes(ctx, scans, 0.1, axis=(0.0, 0.0, 1.0), eps_angle=eps)
    for seed in (-1, 2 ** 32, 0.5):
        with pytest.raises(ValueError):
            ltm.Context.segment_plane(ctx, cloud, 0.1, seed=seed)
    for bad in (np.zeros((4, 4), np.float32), None, cloud, object()):
        with pytest.raises(TypeError):
            ltm.Context.segment_planes(ctx, bad, 0.1)
    for bad in (scans, None):
        with pytest.raises(TypeError):
            ltm.Context.segment_plane(ctx, bad, 0.1)
    for kb, ke in ((-1, 2), (3, 2)):
        with pytest.raises(ValueError):
            ltm.Context.segment_planes(ctx, scans, 0.1, kf_begin=kb, kf_end=ke)


PROGRAM = r"""
#include "removert/DeviceSACSegmentation.h"
#include <cstdio>

int main()
{
    ltm_plane_params p;
    ltm_plane_default_params(&p);
    std::printf("defaults %.1f %u %u %.1f %.1f %.1f %.1f %d block %u\n", p.distance_threshold, p.max_iterations, p.seed, p.axis[0], p.axis[1], p.axis[2], p.eps_angle,
                p.refine, ltm_plane_block_points());
    {
        ltremovert::DeviceSACSegmentation probe(nullptr);
        int refused = 0;
        try { probe.setModelType(5); } catch (const std::invalid_argument&) { ++refused; }       // SACMODEL_CYLINDER
        try { probe.setMethodType(1); } catch (const std::invalid_argument&) { ++refused; }      // SAC_LMEDS
        probe.setModelType(ltremovert::SACMODEL_PERPENDICULAR_PLANE);
        probe.setMethodType(ltremovert::SAC_RANSAC);
        std::printf("refused %d model %d method %d optimize %d iterations %d\n", refused, probe.getModelType(), probe.getMethodType(),
                    (int)probe.getOptimizeCoefficients(), probe.getMaxIterations());
    }
    ltm_config cfg{};
    cfg.vfov = 50.0f; cfg.hfov = 360.0f;
    for (int i = 0; i < 16; ++i) cfg.lidar2base[i] = (i % 5 == 0) ? 1.0 : 0.0;
    ltm_ctx* ctx = nullptr;
    const int rc = ltm_create(&cfg, &ctx);
    if (rc != LTM_OK) { std::printf("no device: %d\n", rc); return 0; }
    {
        // a 10 x 10 lattice of z = 2 and a 9 x 9 wall x = 20: exact planes
        ltremovert::Cloud ground, wall, both, none;
        for (int i = 0; i < 10; ++i) for (int j = 0; j < 10; ++j) ground.push_back(ltremovert::PointType{(float)i, (float)j, 2.0f, 0.0f});
        for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) wall.push_back(ltremovert::PointType{20.0f, (float)i, 3.0f + (float)j, 0.0f});
        both = wall;
        both.insert(both.end(), ground.begin(), ground.end());
        ltremovert::DeviceSACSegmentation seg(ctx);
        seg.setModelType(ltremovert::SACMODEL_PLANE);
        seg.setMethodType(ltremovert::SAC_RANSAC);
        seg.setDistanceThreshold(0.25);
        seg.setMaxIterations(64);
        seg.setInputCloud(both);
        ltremovert::PointIndices inliers;
        ltremovert::ModelCoefficients coeff;
        seg.segment(inliers, coeff);
        std::printf("plane %zu first %d c %.2f d %.2f\n", inliers.indices.size(), inliers.indices[0], coeff.values[2], coeff.values[3]);
        seg.setModelType(ltremovert::SACMODEL_PERPENDICULAR_PLANE);
        seg.setAxis(1.0, 0.0, 0.0);
        seg.setEpsAngle(0.2);
        seg.setMaxIterations(512);
        std::vector<ltremovert::PointIndices> many;
        std::vector<ltremovert::ModelCoefficients> coeffs;
        seg.segment({&both, &none, &ground}, many, coeffs);
        std::printf("batch %zu: %zu %zu %zu coeff %zu %zu %zu first %d x %.2f d %.2f\n", many.size(), many[0].indices.size(), many[1].indices.size(),
                    many[2].indices.size(), coeffs[0].values.size(), coeffs[1].values.size(), coeffs[2].values.size(), many[0].indices[0], coeffs[0].values[0],
                    coeffs[0].values[3]);
    }
    ltm_destroy(ctx);
    return 0;
}
"""


def test_device_sac_header_compiles_and_links(tmp_path, ltm):
    ltm.load_library()
    src = tmp_path / "sac_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "sac_user"
    pkg = os.path.join(ROOT, "lt-mapper_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", pkg, "-lltm_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "defaults 0.0 128 0 0.0 0.0 0.0 0.0 1 block %d" % pc.BLOCK_POINTS in r.stdout, r.stdout
    assert "refused 2 model 11 method 0 optimize 1 iterations 128" in r.stdout, r.stdout
    import torch
    if torch.cuda.is_available():
        # without an axis the larger plane wins: the ground, points 81 .. 180 of the cloud, z = 2; with the axis x the wall; the ground alone has no plane near x
        assert "plane 100 first 81 c 1.00 d -2.00" in r.stdout, r.stdout
        assert "batch 3: 81 0 0 coeff 4 0 0 first 0 x 1.00 d -20.00" in r.stdout, r.stdout
    else:
        assert "no device" in r.stdout, r.stdout
