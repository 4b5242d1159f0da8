"""CPU checks of the FPFH interface (no device needed): the entry points of include/ltm.h "fpfh" are declared, exported and bound; bad arguments are refused
before a device could be touched; the Python surface carries its names; and the host header DeviceFPFHEstimation.h compiles under -Wall -Wextra -Werror,
links and runs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tools import fpfh_numpy as fref

ENTRY_POINTS = ("ltm_search_fpfh", "ltm_fpfh_info", "ltm_fpfh_device", "ltm_fpfh_download", "ltm_fpfh_free", "ltm_debug_fpfh_stats")


def test_header_declares_and_library_exports_the_entry_points(ltm):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltm.h")).read(), flags=re.S)
    lib = ltm.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} not declared in include/ltm.h"
        assert hasattr(lib, name), f"{name} not exported by libltm_hip.so"
        assert name in ltm.SIGNATURES
    assert re.search(r"typedef\s+struct\s+ltm_fpfh\s+ltm_fpfh\s*;", src)
    assert lib.ltm_abi_version() == 1
    assert (ltm.FPFH_SIZE, ltm.FPFH_MIN_K, ltm.FPFH_MAX_K) == (fref.SIZE, fref.MIN_K, fref.MAX_K) == (33, 2, 64)
    assert ltm.FPFH_STATS == ("finite_points", "distance_evaluations", "pairs_skipped", "lds_points")
    for name in ("info", "k", "n_target", "n_finite", "offsets", "descriptors", "device_view", "spfh_counts", "close", "__enter__", "__exit__"):
        assert hasattr(ltm.Fpfh, name)
    for name in ("fpfh", "fpfh_stats"):
        assert hasattr(ltm.Context, name)
    assert hasattr(ltm.SearchIndex, "fpfh")


def test_argument_errors_need_no_device(ltm):
    lib = ltm.load_library()
    idx = (C.c_void_p * 1)(0x1000)
    sz, k, vp, u = C.c_size_t(7), C.c_int(7), C.c_void_p(0x77), (C.c_uint64 * 4)(7, 7, 7, 7)
    bogus = C.c_void_p(0x1000)
    for kk in (10, 1, 65):
        out = C.c_void_p(0x1234)
        assert lib.ltm_search_fpfh(None, 1, idx, kk, C.byref(out)) == -1 and out.value is None      # no handle is returned
    assert lib.ltm_search_fpfh(None, 0, None, 10, None) == -1
    assert lib.ltm_fpfh_info(None, bogus, C.byref(sz), C.byref(sz), C.byref(k)) == -1
    assert lib.ltm_fpfh_device(None, bogus, C.byref(vp), C.byref(vp), C.byref(vp)) == -1
    assert lib.ltm_fpfh_download(None, bogus, None, None, None, None) == -1
    assert lib.ltm_fpfh_free(None, bogus) == -1
    assert lib.ltm_fpfh_free(None, None) == -1
    assert lib.ltm_debug_fpfh_stats(None, u, 0) == -1
    assert (sz.value, k.value, vp.value, list(u)) == (7, 7, 0x77, [7, 7, 7, 7])      # nothing was written


def test_python_surface_refuses_what_is_no_index(ltm):
    ctx = object.__new__(ltm.Context)      # no library handle: any call into it would fail with AttributeError, not TypeError
    index = ltm.SearchIndex(ctx, 0)
    for bad in ([np.zeros((4, 4), np.float32)], [None], [ltm.Cloud(ctx, 0)], [index, object()]):
        with pytest.raises(TypeError):
            ltm.Context.fpfh(ctx, bad, 10)


PROGRAM = r"""
#include "removert/DeviceFPFHEstimation.h"
#include <cmath>
#include <cstdio>

int main()
{
    {
        ltremovert::DeviceFPFHEstimation fpfh(nullptr);
        std::vector<float> out;
        ltremovert::Cloud cloud;
        int refused = 0;
        try { fpfh.compute(out); } catch (const std::logic_error&) { ++refused; }      // no input
        fpfh.setInputCloud(cloud);
        try { fpfh.compute(out); } catch (const std::logic_error&) { ++refused; }      // no k
        fpfh.setKSearch(12);
        try { fpfh.compute(out); } catch (const std::logic_error&) { ++refused; }      // a cloud needs setInputNormals
        fpfh.setInputNormals(10);
        std::printf("refused %d k %d normals %d size %d\n", refused, fpfh.getKSearch(), fpfh.getNormalsK(), ltremovert::DeviceFPFHEstimation::kDescriptorSize);
    }
    ltm_config cfg{};
    cfg.vfov = 50.0f; cfg.hfov = 360.0f;
    for (int i = 0; i < 16; ++i) cfg.lidar2base[i] = (i % 5 == 0) ? 1.0 : 0.0;
    ltm_ctx* ctx = nullptr;
    const int rc = ltm_create(&cfg, &ctx);
    if (rc != LTM_OK) { std::printf("no device: %d\n", rc); return 0; }
    {
        // a 10 x 10 lattice of z = 1: every descriptor is the planar known answer; one point without finite coordinates at position 7
        ltremovert::Cloud cloud;
        for (int i = 0; i < 10; ++i) for (int j = 0; j < 10; ++j) cloud.push_back(ltremovert::PointType{(float)i, (float)j, 1.0f, 0.0f});
        cloud.insert(cloud.begin() + 7, ltremovert::PointType{NAN, 0.0f, 0.0f, 0.0f});
        ltremovert::DeviceFPFHEstimation fpfh(ctx);
        fpfh.setInputCloud(cloud);
        fpfh.setInputNormals(9, 4.5f, 4.5f, 10.0f);
        fpfh.setKSearch(9);
        std::vector<float> out;
        fpfh.compute(out);
        size_t planar = 0, nan_rows = 0;
        for (size_t i = 0; i < cloud.size(); ++i) {
            const float* row = out.data() + 33 * i;
            if (std::isnan(row[0])) { ++nan_rows; continue; }
            bool ok = true;
            for (int b = 0; b < 33; ++b) ok = ok && row[b] == ((b == 5 || b == 16 || b == 27) ? 100.0f : 0.0f);
            planar += ok ? 1 : 0;
        }
        std::printf("rows %zu planar %zu nan %zu nan_at_7 %d\n", out.size() / 33, planar, nan_rows, (int)std::isnan(out[33 * 7]));
        int refused = 0;
        fpfh.setKSearch(65);
        try { fpfh.compute(out); } catch (const std::runtime_error&) { ++refused; }
        std::printf("k65 refused %d\n", refused);
    }
    ltm_destroy(ctx);
    return 0;
}
"""


def test_device_fpfh_header_compiles_and_links(tmp_path, ltm):
    ltm.load_library()
    src = tmp_path / "fpfh_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "fpfh_user"
    pkg = os.path.join(ROOT, "lt-mapper_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", pkg, "-lltm_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refused 3 k 12 normals 10 size 33" in r.stdout, r.stdout
    import torch
    if torch.cuda.is_available():
        assert "rows 101 planar 100 nan 1 nan_at_7 1" in r.stdout, r.stdout
        assert "k65 refused 1" in r.stdout, r.stdout
    else:
        assert "no device" in r.stdout, r.stdout
