"""CPU checks of the normals and point-to-plane ICP interface (no device needed): the new entry points are declared, exported and bound and the
structs are what they were, method="point" stays the default, argument errors are raised before a device could be touched, every ICP fixture of the GPU
tests (tests/normals_cases.py) is one on which the order of the sums decides nothing discrete, the plane restatement (tools/icp_plane_numpy.py) is closer
to the truth in fewer iterations than the point-to-point one, and the C++ host mirrors compile without warnings, link and run."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import icp_fixtures as fx
import normals_cases as nc
from conftest import ROOT
from tools import icp_plane_numpy as plane_ref

NEW = ("ltm_search_estimate_normals", "ltm_search_normals_info", "ltm_search_normals_download", "ltm_icp_align_plane", "ltm_icp_align_plane_scanset")


def test_header_declares_and_library_exports_the_new_entry_points(ltm):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltm.h")).read(), flags=re.S)
    lib = ltm.load_library()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/ltm.h"
        assert hasattr(lib, name), f"{name} not exported by libltm_hip.so"
        assert name in ltm.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
    # the plane entry points take what the point-to-point ones take
    assert ltm.SIGNATURES["ltm_icp_align_plane"] == ltm.SIGNATURES["ltm_icp_align"]
    assert ltm.SIGNATURES["ltm_icp_align_plane_scanset"] == ltm.SIGNATURES["ltm_icp_align_scanset"]
    # the structs are unchanged
    assert ltm.ICP_RESULT.itemsize == 160 and ltm.ICP_RESULT.fields["fitness"][1] == 128 and ltm.ICP_RESULT.fields["n_corr"][1] == 156
    assert [f for f, _ in ltm.IcpParams._fields_] == ["max_corr_dist", "max_iterations", "transformation_epsilon", "euclidean_fitness_epsilon"]
    assert C.sizeof(ltm.IcpParams) == 32
    assert ltm.ICP_STATES[:5] == ("too few correspondences", "iterations", "transform", "absolute mse", "relative mse") and len(ltm.ICP_STATES) == 6
    for cls, names in ((ltm.Context, ("estimate_normals", "icp_align", "verify_loops")), (ltm.SearchIndex, ("estimate_normals", "normals"))):
        for n in names:
            assert hasattr(cls, n), (cls, n)


def test_the_defaults_keep_the_point_to_point_method(ltm):
    assert inspect.signature(ltm.Context.icp_align).parameters["method"].default == "point"
    vl = inspect.signature(ltm.Context.verify_loops).parameters
    assert vl["method"].default == "point" and vl["normal_k"].default == 10
    assert inspect.signature(ltm.Context.estimate_normals).parameters["k"].default == 10
    assert inspect.signature(ltm.SearchIndex.estimate_normals).parameters["k"].default == 10


def test_argument_errors_need_no_device(ltm):
    lib = ltm.load_library()
    p = ltm.icp_params()
    res = np.zeros(1, ltm.ICP_RESULT)
    th = (C.c_void_p * 1)(0x1000)
    sh = (C.c_uint64 * 1)(1)
    kf = np.zeros(1, np.uint32)
    assert lib.ltm_icp_align_plane(None, 1, th, sh, None, C.byref(p), res.ctypes.data, None) == -1
    assert lib.ltm_icp_align_plane_scanset(None, 1, th, 1, kf.ctypes.data, None, C.byref(p), res.ctypes.data, None) == -1
    assert lib.ltm_search_estimate_normals(None, 1, th, 10, None) == -1
    assert lib.ltm_search_normals_info(None, th[0], None, None) == -1
    assert lib.ltm_search_normals_download(None, th[0], None) == -1
    # the Python surface checks its arguments before it calls the library: no context is needed to get these
    ctx = object.__new__(ltm.Context)
    with pytest.raises(ValueError):
        ltm.Context.icp_align(ctx, [], method="gicp")
    with pytest.raises(ValueError):
        ltm.Context.estimate_normals(ctx, [], k=2)
    with pytest.raises(ValueError):
        ltm.Context.estimate_normals(ctx, [], k=65)
    with pytest.raises(TypeError):
        ltm.Context.estimate_normals(ctx, [np.zeros((4, 3))], k=10)
    idx = ltm.SearchIndex(ctx, None)
    with pytest.raises(ValueError):
        ltm.Context.estimate_normals(ctx, [idx, idx])
    with pytest.raises(ValueError):
        ltm.Context.estimate_normals(ctx, [idx], viewpoints=np.zeros((2, 3)))


def _fixture_condition(kind, key=None, max_corr_dist=150.0):
    """the discrete part of the result is the same whichever order the sums run in, and the transforms stay within the bound the GPU tests use"""
    t, s, nrm, base = nc.plane_fixture(kind, key, max_corr_dist)
    n = int(np.isfinite(s[:, :3]).all(axis=1).sum())
    worst = 0.0
    for order in (np.arange(n)[::-1], np.random.default_rng(n).permutation(n)):
        r = plane_ref.align(t, nrm, s, order=order, max_corr_dist=max_corr_dist)
        assert (r["iterations"], r["state"], r["converged"]) == (base["iterations"], base["state"], base["converged"])
        assert np.array_equal(r["trace"][:, 0], base["trace"][:, 0], equal_nan=True)
        worst = max(worst, np.abs(r["T"] - base["T"]).max())
    assert worst <= fx.tol_T(n) * (nc.FAR_SCALE if kind == "far" else 1.0), (worst, fx.tol_T(n))
    return base


def test_fixture_condition_scenes_and_the_truth():
    """point-to-plane ends closer to the ground truth than point-to-point, in fewer iterations, on every scene pair"""
    for name in fx.SCENES:
        plane = _fixture_condition("scene", name)
        point = fx.scene_fixture(name)[2]
        truth = fx.rigid(fx.SCENES[name][3], fx.SCENES[name][4])
        e_plane, e_point = np.abs(plane["T"] - truth).max(), np.abs(point["T"] - truth).max()
        print(f"{name}: plane {plane['iterations']} iterations, error {e_plane:.2e}; point {point['iterations']} iterations, error {e_point:.2e}")
        assert plane["converged"] == 1 and plane["state"] == 2 and point["state"] == 2
        assert e_plane <= e_point and plane["iterations"] < point["iterations"]


def test_fixture_condition_far_from_the_origin():
    """the same scene 2 km from the origin: it converges to the near fixture's transform conjugated by the offset (in more iterations: the step's
    translation, which the transform test looks at, includes the rotation's lever arm of 2 km)"""
    far = _fixture_condition("far", nc.FAR_SCENE)
    near = nc.plane_fixture("scene", nc.FAR_SCENE)[3]
    assert (far["state"], far["converged"], far["n_corr"]) == (near["state"], near["converged"], near["n_corr"]) and far["iterations"] >= near["iterations"]
    shift = np.eye(4)
    shift[:3, 3] = fx.FAR
    assert np.abs(far["T"] - shift @ near["T"] @ np.linalg.inv(shift)).max() < 1e-2


def test_fixture_condition_outliers():
    near = _fixture_condition("outlier", None, 1.0)
    far = _fixture_condition("outlier", None, 150.0)
    assert (near["trace"][:near["iterations"], 0] == 600).all() and (far["trace"][:far["iterations"], 0] == 640).all()
    assert np.abs(near["T"] - far["T"]).max() > 0.1, "with the outliers kept the alignment ends elsewhere"


def test_fixture_condition_edges():
    assert len(fx.edge_pairs()) == nc.N_EDGE
    states = [_fixture_condition("edge", k)["state"] for k in range(nc.N_EDGE)]
    assert states[0] == 5, "three correspondences cannot determine six unknowns"
    assert all(s == 2 for s in states[1:]), states


def test_restatement_edge_cases():
    t, s = fx.lattice_pair()
    nrm = nc.target_normals("lattice")
    e = np.zeros((0, 3), np.float32)
    for r in (plane_ref.align(e, e, s), plane_ref.align(t, nrm, e), plane_ref.align(t, nrm, s, max_iterations=0)):
        assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 0) and r["fitness"] == plane_ref.DBL_MAX and (r["T"] == np.eye(4)).all()
    # a single exact plane: three unknowns are not determined, whatever the start
    pt, ps = nc.plane_z0()
    pn = nc.nref.estimate(pt, 10)["normals"]
    assert (pn == np.float32((0, 0, 1, 0))).all()
    init = fx.rigid(2.0, (0.1, 0.0, 0.0))
    r = plane_ref.align(pt, pn, ps, init=init)
    assert (r["iterations"], r["converged"], r["state"]) == (0, 0, 5) and r["n_corr"] == len(ps) and (r["T"] == init).all()
    # a correspondence whose normal is not finite is dropped; fewer than three left: state 0
    few = nrm.copy()
    few[2:] = np.nan
    r = plane_ref.align(t, few, t[:10].copy())
    assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 2)
    # the lattice's known answer is point-to-plane's as well (normals along the axes): the shift of 0.25 in x
    r = nc.plane_fixture("lattice")[3]
    assert r["converged"] == 1 and abs(r["T"][0, 3] - 0.25) < 1e-9 and np.abs(r["T"][:3, :3] - np.eye(3)).max() < 1e-9


PROGRAM = r"""
#include "removert/DeviceICP.h"
#include "removert/DeviceNormalEstimation.h"
#include <cmath>
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
        // a floor and two walls, 21 x 21 points each, and every fourth point of them moved by (-0.05, 0.02, 0.03)
        ltremovert::Cloud target, source;
        int n = 0;
        for (int face = 0; face < 3; ++face)
            for (int a = 0; a <= 20; ++a)
                for (int b = 0; b <= 20; ++b, ++n) {
                    const float u = 0.5f * a, v = 0.5f * b;
                    const ltremovert::PointType p = face == 0 ? ltremovert::PointType{u, v, 0.0f, 0.0f}
                                                   : face == 1 ? ltremovert::PointType{u, 0.0f, v, 0.0f} : ltremovert::PointType{0.0f, u, v, 0.0f};
                    target.push_back(p);
                    if (n % 4 == 0) source.push_back(ltremovert::PointType{p.x - 0.05f, p.y + 0.02f, p.z + 0.03f, 0.0f});
                }
        ltremovert::DeviceNormalEstimation ne(ctx);
        ne.setInputCloud(target);
        ne.setKSearch(8);
        ne.setViewPoint(5.0f, 5.0f, 5.0f);
        ltremovert::NormalCloud normals;
        ne.compute(normals);
        const ltremovert::Normal& f = normals[21 * 10 + 10];      // the middle of the floor
        std::printf("normals %zu floor %.1f %.1f %.1f curvature %.1f\n", normals.size(), f.normal_x, f.normal_y, f.normal_z, f.curvature);
        ltremovert::DeviceICP icp(ctx);
        icp.setMethod(ltremovert::DeviceICP::PointToPlane);
        icp.setKSearch(8);
        icp.setViewPoint(5.0f, 5.0f, 5.0f);
        icp.setInputSource(source);
        icp.setInputTarget(target);
        ltremovert::Cloud aligned;
        icp.align(aligned);
        const ltremovert::Matrix4d T = icp.getFinalTransformation();
        const double err = std::fabs(T[3] - 0.05) + std::fabs(T[7] + 0.02) + std::fabs(T[11] + 0.03);
        std::printf("plane converged %d t %s iterations %s\n", (int)icp.hasConverged(), err < 1e-6 ? "exact" : "off", icp.result().iterations <= 4 ? "few" : "many");
    }
    ltm_destroy(ctx);
    return 0;
}
"""


def test_host_headers_compile_and_link(tmp_path, ltm):
    ltm.load_library()
    src = tmp_path / "plane_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "plane_user"
    pkg = os.path.join(ROOT, "lt-mapper_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", pkg, "-lltm_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    import torch
    if torch.cuda.is_available():
        assert "normals 1323 floor 0.0 0.0 1.0 curvature 0.0" in r.stdout, r.stdout
        assert "plane converged 1 t exact iterations few" in r.stdout, r.stdout
    else:
        assert "no device" in r.stdout, r.stdout
