"""CPU checks of the loop-submap interface (no device needed): the header declares every new entry point, the library exports it and capi binds it, null
arguments are refused before a device could be touched, ltm_pose6d_to_affine3f is the stated float formula bit for bit, and the C++ host mirror
DeviceLoopSubmaps.h compiles without warnings, links against the library and runs its no-device paths."""
import ctypes as C
import ctypes.util
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from tools import submap_numpy as ref

NEW = ("ltm_pose6d_to_affine3f", "ltm_submaps_assemble", "ltm_search_build_scanset", "ltm_icp_align_scanset")


def test_header_declares_and_library_exports_the_entry_points(ltm):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltm.h")).read(), flags=re.S)
    lib = ltm.load_library()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/ltm.h"
        assert hasattr(lib, name), f"{name} not exported by libltm_hip.so"
        assert name in ltm.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
    for name in ("loop_submaps", "search_index_batch", "verify_loops"):
        assert hasattr(ltm.Context, name)
    assert callable(ltm.pose6d_to_affine3f)


def test_null_context_and_null_arguments_are_refused(ltm):
    lib = ltm.load_library()
    out = C.c_uint64()
    keys = np.zeros(1, np.int32)
    assert lib.ltm_submaps_assemble(None, 1, None, keys.ctypes.data, 1, 0, 0.3, 1, C.byref(out)) == -1
    hs = (C.c_void_p * 1)()
    assert lib.ltm_search_build_scanset(None, 1, 0, 1, hs) == -1
    res = np.zeros(1, ltm.ICP_RESULT)
    th = (C.c_void_p * 1)(0x1000)
    kf = np.zeros(1, np.uint32)
    assert lib.ltm_icp_align_scanset(None, 1, th, 1, kf.ctypes.data, None, None, res.ctypes.data, None) == -1
    pose = np.zeros(6, np.float32)
    aff = np.zeros(12, np.float32)
    assert lib.ltm_pose6d_to_affine3f(None, 1, aff.ctypes.data) == -1
    assert lib.ltm_pose6d_to_affine3f(pose.ctypes.data, 1, None) == -1
    assert lib.ltm_pose6d_to_affine3f(pose.ctypes.data, 1, aff.ctypes.data) == 0


def _libm():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for f in (libm.cosf, libm.sinf):
        f.restype, f.argtypes = C.c_float, [C.c_float]
    cosf = np.vectorize(lambda v: libm.cosf(float(v)), otypes=[np.float32])
    sinf = np.vectorize(lambda v: libm.sinf(float(v)), otypes=[np.float32])
    return cosf, sinf


def test_pose6d_to_affine3f_is_the_stated_formula_bit_for_bit(ltm):
    """1000 seeded poses (translations up to 2 km, every angle in [-pi, pi]); cos / sin come from the same libm on both sides, so only the stated products
    and sums -- each rounded to float32 on its own -- are under test"""
    rng = np.random.default_rng(20)
    poses = np.concatenate([rng.uniform(-2000.0, 2000.0, (1000, 3)), rng.uniform(-np.pi, np.pi, (1000, 3))], axis=1).astype(np.float32)
    got = ltm.pose6d_to_affine3f(poses)
    want = ref.pose6d_to_affine3f(poses, *_libm())
    assert got.shape == (1000, 3, 4) and got.dtype == np.float32
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_pose6d_to_affine3f_known_answers(ltm):
    eye = np.eye(4, dtype=np.float32)[:3]
    assert (ltm.pose6d_to_affine3f(np.zeros(6)) == eye).all()      # (-0.0 == 0.0: row 2 starts with -sinf(0))
    got = ltm.pose6d_to_affine3f([1.0, 2.0, 3.0, 0.0, 0.0, np.pi / 2.0])[0]
    # yaw = pi/2 swaps the axes: x -> y, y -> -x; cosf((float)(pi/2)) is not zero but about -4.4e-8, and every entry is within one ulp of it of the ideal
    c = abs(float(_libm()[0](np.float32(np.pi / 2.0))))
    assert 0.0 < c < 1e-7
    ulp = float(np.spacing(np.float32(c)))
    want = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]])
    assert np.abs(got.astype(np.float64) - want).max() <= c + ulp
    assert (got[:, 3] == np.float32([1.0, 2.0, 3.0])).all() and got[1, 0] == 1.0 and got[0, 1] == -1.0 and got[2, 2] == 1.0


def test_restatement_windows_and_identity():
    """the restatement itself: windows clip to the set, out-of-range keys give empty windows, the identity maps -0.0 to +0.0"""
    scans = np.arange(40, dtype=np.float32).reshape(10, 4)
    scans[0, 0] = -0.0
    off = np.array([0, 0, 3, 4, 10], np.uint64)
    pts, o = ref.assemble(scans, off, [-3, 0, 3, 100], 1)
    assert o.tolist() == [0, 0, 3, 10, 10]      # keyframe sizes 0, 3, 1, 6: key 0 -> keyframes 0, 1; key 3 -> keyframes 2, 3
    assert (pts[:, 3] == scans[:, 3]).all()
    assert not np.signbit(pts[0, 0])
    pts, o = ref.assemble(scans, off, [2], 25)
    assert o.tolist() == [0, 10]


PROGRAM = r"""
#include "removert/DeviceLoopSubmaps.h"
#include <cstdio>

int main()
{
    using namespace ltremovert;
    const Affine3f I = getTransformation(Pose6D{0, 0, 0, 0, 0, 0});
    std::printf("identity %g %g %g %g\n", I[0], I[5], I[10], I[3]);
    const Cloud moved = transformPointCloud(Cloud{PointType{1.0f, 2.0f, 3.0f, 7.0f}}, Pose6D{10.0f, 20.0f, 30.0f, 0, 0, 0});
    std::printf("moved %g %g %g %g\n", moved[0].x, moved[0].y, moved[0].z, moved[0].intensity);
    ltm_config cfg{};
    cfg.vfov = 50.0f; cfg.hfov = 360.0f;
    for (int i = 0; i < 16; ++i) cfg.lidar2base[i] = (i % 5 == 0) ? 1.0 : 0.0;
    ltm_ctx* ctx = nullptr;
    const int rc = ltm_create(&cfg, &ctx);
    if (rc != LTM_OK) { std::printf("no device: %d\n", rc); return 0; }
    {
        // three keyframes of a 4 x 4 lattice with 0.25 m pitch, 1 m apart along x; poses move them onto each other
        Cloud all;
        std::vector<uint64_t> off{0};
        std::vector<Pose6D> poses;
        for (int k = 0; k < 3; ++k) {
            for (int x = 0; x < 4; ++x)
                for (int y = 0; y < 4; ++y) all.push_back(PointType{0.25f * x + 1.0f * k, 0.25f * y, 0.0f, (float)k});
            off.push_back(all.size());
            poses.push_back(Pose6D{-1.0f * k, 0, 0, 0, 0, 0});
        }
        ltm_scanset scans = 0;
        if (ltm_scanset_upload(ctx, all.data(), sizeof(PointType), off.data(), 3, &scans) != LTM_OK) return 1;
        DeviceLoopSubmaps sub(ctx, scans, poses, 0.5f);
        const ltm_scanset local = sub.loopFindNearKeyframesLocalCoord({1, 7}, 1);
        const ltm_scanset central = sub.loopFindNearKeyframesCentralCoord({1}, 1);
        std::printf("local %zu %zu central %zu\n", sub.download(local, 0).size(), sub.download(local, 1).size(), sub.download(central, 0).size());
        std::vector<ltm_search*> idx = sub.buildTargets(local);
        size_t nt = 0, nf = 0;
        ltm_search_info(ctx, idx[0], &nt, &nf);
        std::printf("indices %zu target %zu finite %zu\n", idx.size(), nt, nf);
        for (ltm_search* s : idx) ltm_search_free(ctx, s);
        ltm_scanset_free(ctx, local);
        ltm_scanset_free(ctx, central);
        ltm_scanset_free(ctx, scans);
    }
    ltm_destroy(ctx);
    return 0;
}
"""


def test_device_loop_submaps_header_compiles_and_links(tmp_path, ltm):
    ltm.load_library()
    src = tmp_path / "submap_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "submap_user"
    pkg = os.path.join(ROOT, "lt-mapper_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", pkg, "-lltm_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "identity 1 1 1 0" in r.stdout and "moved 11 22 33 7" in r.stdout, r.stdout
    import torch
    if torch.cuda.is_available():
        # leaf 0.5 m (every quantity exact in float): a lattice covers 2 x 2 cells, the three lattices side by side 12; moved onto each other by their
        # poses they fall into the 4 cells of one lattice; key 7 +- 1 is outside the set: an empty submap
        assert "local 12 0 central 4" in r.stdout, r.stdout
        assert "indices 2 target 12 finite 12" in r.stdout, r.stdout
    else:
        assert "no device" in r.stdout, r.stdout
