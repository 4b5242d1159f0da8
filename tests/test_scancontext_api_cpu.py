"""CPU checks of the scan-context interface (no device needed): include/ltm.h declares it, libltm_hip.so exports it, capi binds it, the defaults are
the reference's, every entry point refuses a null context or handle before it could touch a device, and the C++ host mirror DeviceSCManager.h
compiles without warnings, links against the library and runs."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

ENTRY_POINTS = ("ltm_sc_default_params", "ltm_sc_from_scanset", "ltm_sc_from_descriptors", "ltm_sc_info", "ltm_sc_download", "ltm_sc_distance",
                "ltm_sc_detect", "ltm_sc_free")


def test_header_declares_and_library_exports_the_scan_context_entry_points(ltm):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltm.h")).read(), flags=re.S)
    lib = ltm.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/ltm.h"
        assert hasattr(lib, name), f"{name} not exported by libltm_hip.so"
        assert name in ltm.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
    assert sorted(n for n in ltm.SIGNATURES if n.startswith("ltm_sc_")) == sorted(ENTRY_POINTS)
    assert "typedef struct ltm_sc ltm_sc;" in src and "ltm_sc_params;" in src
    assert "#define LTM_ABI_VERSION 1" in src
    assert hasattr(ltm, "ScanContexts") and hasattr(ltm.Context, "scan_contexts") and hasattr(ltm.Context, "scan_contexts_from")
    for method in ("download", "distance", "detect", "close"):
        assert hasattr(ltm.ScanContexts, method)


def test_default_params_are_the_reference_values(ltm):
    p = ltm.ScParams()
    ltm.load_library().ltm_sc_default_params(C.byref(p))
    got = (p.lidar_height, p.num_ring, p.num_sector, p.max_radius, p.num_candidates, p.search_ratio, p.dist_thres)
    assert got == (2.0, 20, 60, 80.0, 3, 0.1, 0.3)
    ltm.load_library().ltm_sc_default_params(None)      # a null pointer is ignored
    q = ltm.sc_params(num_candidates=0, search_ratio=1.0)
    assert (q.num_candidates, q.search_ratio, q.num_ring) == (0, 1.0, 20)


def test_null_context_and_null_handles_are_refused(ltm):
    lib = ltm.load_library()
    out = C.c_void_p()
    n = C.c_size_t()
    r = C.c_int()
    p = ltm.sc_params()
    pairs = (C.c_int32 * 2)(0, 0)
    d = C.c_double()
    s = C.c_int32()
    f = C.c_float()
    desc = (C.c_double * 1200)()
    for handle in (None, C.c_void_p(0x1000)):       # a handle that was never issued, with a null context: nothing is dereferenced
        assert lib.ltm_sc_from_scanset(None, 1, 0, 1, C.byref(p), C.byref(out)) == -1
        assert lib.ltm_sc_from_descriptors(None, desc, 1, C.byref(p), C.byref(out)) == -1
        assert lib.ltm_sc_info(None, handle, C.byref(n), C.byref(r), C.byref(r)) == -1
        assert lib.ltm_sc_download(None, handle, desc, None, None) == -1
        assert lib.ltm_sc_distance(None, handle, handle, pairs, 1, C.byref(p), C.byref(d), C.byref(s)) == -1
        assert lib.ltm_sc_detect(None, handle, handle, C.byref(p), C.byref(s), C.byref(s), C.byref(d), C.byref(s), C.byref(f)) == -1
        assert lib.ltm_sc_free(None, handle) == -1
    assert out.value is None


PROGRAM = r"""
#include "removert/DeviceSCManager.h"
#include <cmath>
#include <cstdio>

int main()
{
    ltm_config cfg{};
    cfg.vfov = 50.0f; cfg.hfov = 360.0f;
    for (int i = 0; i < 16; ++i) cfg.lidar2base[i] = (i % 5 == 0) ? 1.0 : 0.0;
    ltm_sc_params prm;
    ltm_sc_default_params(&prm);
    std::printf("defaults %d x %d, %d candidates\n", prm.num_ring, prm.num_sector, prm.num_candidates);
    ltm_ctx* ctx = nullptr;
    const int rc = ltm_create(&cfg, &ctx);
    if (rc != LTM_OK) { std::printf("no device: %d\n", rc); return 0; }
    {
        ltremovert::DeviceSCManager central(ctx), query(ctx);
        // three places: a wall of height 1 + k at 10 m (ring 3) that covers sectors [10 k, 10 k + 20)
        for (int k = 0; k < 3; ++k) {
            ltremovert::Cloud scan;
            for (int s = 10 * k; s < 10 * k + 20; ++s)
                for (int j = 0; j < 4; ++j) {
                    const double th = (s + 0.3 + 0.1 * j) * 6.0 * 3.14159265358979323846 / 180.0;
                    scan.push_back(ltremovert::PointType{(float)(10.0 * std::cos(th)), (float)(10.0 * std::sin(th)), (float)(1.0 + k + 0.2 * j * (s % 3)), 0.0f});
                }
            central.makeAndSaveScancontextAndKeys(scan);
        }
        // the second place again, turned by 7 sectors
        ltremovert::DeviceSCManager::Descriptor turned(1200, 0.0);
        const ltremovert::DeviceSCManager::Descriptor& second = central.polarcontexts()[1];
        for (int r = 0; r < 20; ++r)
            for (int c = 0; c < 60; ++c) turned[r * 60 + (c + 7) % 60] = second[r * 60 + c];
        query.saveScancontextAndKeys(turned);
        const std::pair<int, float> loop = central.detectLoopClosureIDBetweenSession(query.getConstRefRecentSCD());
        const std::pair<double, int> d = central.distanceBtnScanContext(turned, second);
        const std::vector<ltremovert::DeviceSCManager::Loop> all = central.detectAll(query.polarcontexts());
        std::printf("loop %d yaw %.4f shift %d dist %s all %d\n", loop.first, loop.second, d.second, std::fabs(d.first) < 1e-9 ? "zero" : "large", all[0].nn_align);
    }
    ltm_destroy(ctx);
    return 0;
}
"""


def test_device_sc_manager_header_compiles_and_links(tmp_path, ltm):
    ltm.load_library()
    src = tmp_path / "sc_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "sc_user"
    pkg = os.path.join(ROOT, "lt-mapper_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", pkg, "-lltm_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "defaults 20 x 60, 3 candidates" in r.stdout, r.stdout
    import torch
    if torch.cuda.is_available():
        assert "loop 1 yaw 0.7330 shift 7 dist zero all 7" in r.stdout, r.stdout
    else:
        assert "no device" in r.stdout, r.stdout
