"""CPU checks of the search index's interface (no device needed): include/ltm.h declares it, libltm_hip.so exports it, capi binds it, the C++
host mirror DeviceKdTree.h compiles and links against the library, and every entry point refuses a null context or handle before it could
touch a device."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

ENTRY_POINTS = ("ltm_search_build", "ltm_search_free", "ltm_search_info", "ltm_knn_search", "ltm_radius_search", "ltm_search_result_info",
                "ltm_search_result_free", "ltm_debug_pool_live")


def test_header_declares_and_library_exports_the_search_entry_points(ltm):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltm.h")).read(), flags=re.S)
    lib = ltm.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/ltm.h"
        assert hasattr(lib, name), f"{name} not exported by libltm_hip.so"
        assert name in ltm.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
    assert "typedef struct ltm_search ltm_search;" in src and "typedef struct ltm_search_result ltm_search_result;" in src
    assert hasattr(ltm, "SearchIndex") and hasattr(ltm.Context, "search_index")


def test_null_context_and_null_handles_are_refused(ltm):
    lib = ltm.load_library()
    out = C.c_void_p()
    sz = C.c_size_t()
    p = C.c_void_p()
    u = C.c_uint64()
    for ctx in (None,):
        assert lib.ltm_search_build(ctx, 1, C.byref(out)) == -1
        assert lib.ltm_search_free(ctx, None) == -1
        assert lib.ltm_search_info(ctx, None, C.byref(sz), C.byref(sz)) == -1
        assert lib.ltm_knn_search(ctx, None, 1, 4, None, None) == -1
        assert lib.ltm_radius_search(ctx, None, 1, 1.0, 0, C.byref(out)) == -1
        assert lib.ltm_search_result_info(ctx, None, C.byref(sz), C.byref(sz), C.byref(p), C.byref(p), C.byref(p)) == -1
        assert lib.ltm_search_result_free(ctx, None) == -1
        assert lib.ltm_debug_pool_live(ctx, C.byref(u), C.byref(u)) == -1
    # a handle that was never issued, with a null context: refused the same way, nothing dereferenced
    bogus = C.c_void_p(0x1000)
    assert lib.ltm_search_free(None, bogus) == -1
    assert lib.ltm_knn_search(None, bogus, 1, 1, None, None) == -1
    assert lib.ltm_search_result_free(None, bogus) == -1


PROGRAM = r"""
#include "removert/DeviceKdTree.h"
#include <cstdio>

int main()
{
    ltm_config cfg{};
    cfg.vfov = 50.0f; cfg.hfov = 360.0f;
    for (int i = 0; i < 16; ++i) cfg.lidar2base[i] = (i % 5 == 0) ? 1.0 : 0.0;
    ltm_ctx* ctx = nullptr;
    const int rc = ltm_create(&cfg, &ctx);
    if (rc != LTM_OK) { std::printf("no device: %d\n", rc); return 0; }
    {
        ltremovert::DeviceKdTree tree(ctx);
        ltremovert::Cloud target;
        for (int i = 0; i < 100; ++i) target.push_back(ltremovert::PointType{(float)i, 0.0f, 0.0f, 0.0f});
        tree.setInputCloud(target);
        std::vector<int> idx;
        std::vector<float> d2;
        const int found = tree.nearestKSearch(ltremovert::PointType{10.2f, 0.0f, 0.0f, 0.0f}, 3, idx, d2);
        const int in_r = tree.radiusSearch(ltremovert::PointType{10.2f, 0.0f, 0.0f, 0.0f}, 1.5, idx, d2);
        std::printf("knn %d first %d radius %d\n", found, found ? idx[0] : -1, in_r);
    }
    ltm_destroy(ctx);
    return 0;
}
"""


def test_device_kdtree_header_compiles_and_links(tmp_path, ltm):
    ltm.load_library()
    src = tmp_path / "kdtree_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "kdtree_user"
    pkg = os.path.join(ROOT, "lt-mapper_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", pkg, "-lltm_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    import torch
    if torch.cuda.is_available():
        assert "knn 3 first 10 radius 3" in r.stdout, r.stdout
    else:
        assert "no device" in r.stdout, r.stdout
