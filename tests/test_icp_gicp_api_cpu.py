"""CPU checks of the generalized-ICP interface (no device needed): ltm_icp_align_gicp is declared, exported and bound and refuses bad arguments before a
device could be touched; the restatement (tools/icp_gicp_numpy.py) is pinned independently of the kernel -- its normal equations against finite
differences of the cost, its weight matrix against np.linalg.inv of GICP's two regularised covariances built from np.linalg.eigh --; a known answer;
the restatement against the ground truth beside point-to-point and point-to-plane; and the conditions every fixture of tests/gicp_cases.py must meet for
the GPU tests (tests/test_gpu_icp_gicp.py) to be able to ask for equal discrete fields."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import gicp_cases as gc
import icp_fixtures as fx
import normals_cases as nc
from conftest import ROOT
from tools import icp_gicp_numpy as gicp_ref
from tools import icp_numpy as point_ref
from tools import icp_plane_numpy as plane_ref
from tools import normals_numpy as nref


def test_header_declares_and_library_exports_the_entry_point(ltm):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltm.h")).read(), flags=re.S)
    lib = ltm.load_library()
    assert re.search(r"\bltm_icp_align_gicp\s*\(", src), "ltm_icp_align_gicp not declared in include/ltm.h"
    assert hasattr(lib, "ltm_icp_align_gicp"), "ltm_icp_align_gicp not exported by libltm_hip.so"
    assert "ltm_icp_align_gicp" in ltm.SIGNATURES
    assert lib.ltm_abi_version() == 1
    assert "gicp" in ltm.ICP_METHODS and ltm.ICP_METHODS[:2] == ("point", "plane")
    assert inspect.signature(ltm.Context.icp_align).parameters["gicp_epsilon"].default == 1e-3
    assert inspect.signature(ltm.Context.icp_align).parameters["method"].default == "point"
    # verify_loops' normals: PCL's k_correspondences_ = 20 for this method when the caller gives none, 10 for point-to-plane as before, the caller's otherwise
    given_none = inspect.signature(ltm.Context.verify_loops).parameters["normal_k"].default
    assert (ltm.normals_k_of("gicp", given_none), ltm.normals_k_of("plane", given_none)) == (20, 10) and given_none == 10
    assert (ltm.normals_k_of("gicp", 10), ltm.normals_k_of("gicp", 20), ltm.normals_k_of("plane", 20)) == (10, 20, 20)
    # the structs are unchanged
    assert ltm.ICP_RESULT.itemsize == 160 and C.sizeof(ltm.IcpParams) == 32


def test_argument_errors_need_no_device(ltm):
    lib = ltm.load_library()
    p = ltm.icp_params()
    res = np.zeros(1, ltm.ICP_RESULT)
    th = (C.c_void_p * 1)(0x1000)
    sh = (C.c_void_p * 1)(0x2000)
    none = (C.c_void_p * 1)(None)
    assert lib.ltm_icp_align_gicp(None, 1, th, sh, None, C.byref(p), 1e-3, res.ctypes.data, None) == -1
    for eps in (0.0, -1.0, 1.5, float("nan")):
        assert lib.ltm_icp_align_gicp(None, 1, th, sh, None, C.byref(p), eps, res.ctypes.data, None) == -1
    assert lib.ltm_icp_align_gicp(None, 1, none, sh, None, C.byref(p), 1e-3, res.ctypes.data, None) == -1
    assert lib.ltm_icp_align_gicp(None, 1, th, none, None, C.byref(p), 1e-3, res.ctypes.data, None) == -1
    assert lib.ltm_icp_align_gicp(None, 1, None, None, None, None, 1e-3, None, None) == -1
    # the Python surface checks its arguments before it calls the library
    ctx = object.__new__(ltm.Context)
    idx = ltm.SearchIndex(ctx, None)
    for eps in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ltm.Context.icp_align(ctx, [(idx, idx)], method="gicp", gicp_epsilon=eps)
    for source in (np.zeros((4, 3), np.float32), (object(), 0), None):
        with pytest.raises(TypeError):
            ltm.Context.icp_align(ctx, [(idx, source)], method="gicp")
    with pytest.raises(TypeError):
        ltm.Context.icp_align(ctx, [(np.zeros((4, 3)), idx)], method="gicp")
    with pytest.raises(ValueError):
        ltm.Context.verify_loops(ctx, None, None, [], method="gicp", normal_k=2)


def test_normal_equations_are_the_cost_s_gradient_and_hessian():
    """for fixed M's, sum A^T M d = -1/2 the gradient of sum (d - A x)^T M (d - A x) at x = 0 and sum A^T M A = 1/2 its Hessian, by central differences
    (step 1e-4 in double; the cost is quadratic in x, so the differences are exact to rounding)"""
    rng = np.random.default_rng(5)
    n = 40
    p, q = rng.uniform(-5.0, 5.0, (n, 3)), rng.uniform(-5.0, 5.0, (n, 3))
    unit = lambda v: v / np.linalg.norm(v, axis=1)[:, None]      # noqa: E731
    M = gicp_ref.weights(unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3))), 1e-3)
    H, g = gicp_ref.normal_equations(p, q, M)
    assert np.allclose(H, H.T, rtol=0, atol=1e-9 * np.abs(H).max())

    def cost(x):
        r = (q - p) - (np.cross(x[:3], p) + x[3:])      # A x = omega x p + t'
        return float(np.einsum("ni,nij,nj->", r, M, r))

    h = 1e-4
    e = np.eye(6) * h
    grad = np.array([(cost(e[i]) - cost(-e[i])) / (2 * h) for i in range(6)])
    hess = np.array([[(cost(e[i] + e[j]) - cost(e[i] - e[j]) - cost(-e[i] + e[j]) + cost(-e[i] - e[j])) / (4 * h * h) for j in range(6)] for i in range(6)])
    dg = np.abs(g + 0.5 * grad).max() / np.abs(g).max()
    dH = np.abs(H - 0.5 * hess).max() / np.abs(H).max()
    print(f"right side against -1/2 gradient: {dg:.2e}, matrix against 1/2 Hessian: {dH:.2e} (bound 1e-6)")
    assert dg <= 1e-6 and dH <= 1e-6


def test_the_weight_is_the_inverse_of_gicp_s_two_covariances():
    """M of the restatement (from the two normals alone) equals inv(C_B + R C_A R^T) with C = V diag(epsilon, 1, 1) V^T from np.linalg.eigh of the
    neighbourhood covariance, on every well-posed point of one scene: the normals form IS GICP's regularised covariance"""
    name = "scene_3000_700"
    cloud = fx.scene_pair(*fx.SCENES[name])[0]
    r = nc.normals_fixture(name + "_k20")[3]
    ok = np.flatnonzero(nc.well_posed(r))
    assert len(ok) > 0.9 * len(cloud)
    p = cloud.astype(np.float64)
    nb = r["neighbours"]
    kk = nb.shape[1]
    d = p[nb[ok]] - p[ok][:, None, :]
    mean = d.sum(axis=1) / kk
    cov = np.einsum("nki,nkj->nij", d, d) / kk - mean[:, :, None] * mean[:, None, :]
    _, V = np.linalg.eigh(cov)
    eps = gc.GICP_EPSILON
    Creg = np.einsum("nij,j,nkj->nik", V, np.array([eps, 1.0, 1.0]), V)
    R = fx.rigid(5.0, (0, 0, 0), pitch_deg=3.0)[:3, :3]
    CB, CA = Creg, np.roll(Creg, 1, axis=0)      # the point itself as the target point, its predecessor as the source point
    want = np.linalg.inv(CB + R @ CA @ R.T)
    n64 = r["normals64"][ok, :3]
    got = gicp_ref.weights(n64, np.roll(n64, 1, axis=0) @ R.T, eps)
    rel = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
    print(f"{len(ok)} well-posed points: largest relative difference {rel.max():.2e} (bound 1e-9)")
    assert rel.max() <= 1e-9


def test_known_answer_an_exact_subset_moved():
    """a source that is an exact subset of a scene target, moved by 2 degrees and 0.1 m: the truth to 1e-5 on every entry of T (the float rounding of
    the moved source at 16 m is 1.9e-6)"""
    target = fx.scene_pair(*fx.SCENES["scene_3000_700"])[0]
    truth = fx.rigid(2.0, (0.06, -0.06, 0.05))
    source = fx.apply(np.linalg.inv(truth), target[::4])
    tn = nref.estimate(target, nc.ICP_NORMAL_K)["normals"]
    sn = nref.estimate(source, nc.ICP_NORMAL_K)["normals"]
    r = gicp_ref.align(target, tn, source, sn)
    err = np.abs(r["T"] - truth).max()
    print(f"exact subset: {r['iterations']} iterations, state {r['state']}, error {err:.2e} (bound 1e-5)")
    assert r["converged"] == 1 and r["n_corr"] == len(source)
    assert err <= 1e-5


def _others(name):
    """the point and plane restatements' results on a scene pair"""
    if name in fx.SCENES:
        return fx.scene_fixture(name)[2], nc.plane_fixture("scene", name)[3]
    t, s, tn, _, _ = gc.gicp_fixture("scene", name)
    return point_ref.align(t, s), plane_ref.align(t, tn, s)


def test_against_the_ground_truth_beside_the_other_methods():
    for name in gc.SCENES:
        t, s, _, _, r = gc.gicp_fixture("scene", name)
        point, plane = _others(name)
        truth = gc.scene_truth(name)
        e = [np.abs(x["T"] - truth).max() for x in (point, plane, r)]
        print(f"{name}: largest entry of T - truth, iterations: point {e[0]:.2e} {point['iterations']}, plane {e[1]:.2e} {plane['iterations']}, "
              f"gicp {e[2]:.2e} {r['iterations']}")
        assert r["converged"] == 1, name
        if len(s) >= 700:
            assert e[2] < e[0], (name, e)


def _condition(kind, key=None, max_corr_dist=150.0, scale=1.0):
    """every normal that enters a correspondence is well-posed (or NaN); the discrete part of the result is the same whichever order the sums run in and
    with every normal component moved by one float ulp; the transforms stay within a tenth of the bound the GPU tests use"""
    t, s, tn, sn, base = gc.gicp_fixture(kind, key, max_corr_dist)
    et, es = gc.estimates(kind, key)
    ft, fs = np.flatnonzero(np.isfinite(t).all(axis=1)), np.flatnonzero(np.isfinite(s[:, :3]).all(axis=1))
    used_t, used_s = set(), set()

    def note(at, idx):
        used_s.update(fs[at].tolist())
        used_t.update(ft[idx].tolist())

    again = gicp_ref.align(t, tn, s, sn, max_corr_dist=max_corr_dist, on_iteration=note)
    assert np.array_equal(again["T"], base["T"])
    for what, est, used in (("target", et, used_t), ("source", es, used_s)):
        gap = est["gap"][sorted(used)]
        bad = ~(np.isnan(gap) | (gap >= nc.WELL_POSED_GAP))
        assert not bad.any(), (kind, key, what, int(bad.sum()), float(gap[bad].min()))
    n = gc.finite_count(s)
    runs = {"reversed": dict(order=np.arange(n)[::-1]), "permuted": dict(order=np.random.default_rng(n).permutation(n)), "normals one ulp off": {}}
    worst = {}
    for what, kw in runs.items():
        a, b = (tn, sn) if kw else (gc.ulp_moved(tn, 2 * n + 1), gc.ulp_moved(sn, 2 * n + 2))
        r = gicp_ref.align(t, a, s, b, max_corr_dist=max_corr_dist, **kw)
        assert (r["iterations"], r["state"], r["converged"]) == (base["iterations"], base["state"], base["converged"]), (kind, key, what)
        assert np.array_equal(r["trace"][:, 0], base["trace"][:, 0], equal_nan=True), (kind, key, what)
        worst[what] = np.abs(r["T"] - base["T"]).max()
    bound = gc.tol_T(n, scale) / 10.0
    print(f"{kind} {key} {max_corr_dist}: iterations {base['iterations']} state {base['state']} n_corr {base['n_corr']}; T moves by "
          + ", ".join(f"{w:.2e} ({k})" for k, w in worst.items()) + f"; bound {bound:.2e} = {gc.T_FACTOR:g} tol_T / 10 (tol_T / 10 = {fx.tol_T(n) * scale / 10:.2e})")
    assert max(worst.values()) < bound, (kind, key, worst, bound)
    return base


def test_fixture_condition_scenes():
    for name in gc.SCENES:
        r = _condition("scene", name)
        assert r["converged"] == 1 and r["state"] == 2


def test_fixture_condition_outliers():
    near = _condition("outlier", None, 1.0)
    far = _condition("outlier", None, 150.0)
    assert (near["trace"][:near["iterations"], 0] == 600).all() and (far["trace"][:far["iterations"], 0] == 640).all()


def test_fixture_condition_edges():
    sizes = [(len(gc.clouds("edge", k)[0]), gc.finite_count(gc.clouds("edge", k)[1])) for k in range(gc.N_EDGE)]
    assert sizes == [(4, 3), (31, 63), (32, 64), (33, 65), (1025, 255), (1025, 256), (1025, 257), (33, 257)]
    assert len(gc.clouds("edge", gc.NAN_EDGE)[1]) == 262
    for k in range(gc.N_EDGE):
        r = _condition("edge", k)
        assert r["converged"] == 1, k      # three correspondences are enough here: M is positive definite


def test_fixture_condition_far_from_the_origin():
    far = _condition("far", gc.FAR_SCENE, scale=gc.FAR_SCALE)
    near = gc.gicp_fixture("scene", gc.FAR_SCENE)[4]
    assert (far["state"], far["converged"], far["n_corr"]) == (near["state"], near["converged"], near["n_corr"])
    shift = np.eye(4)
    shift[:3, 3] = fx.FAR
    assert np.abs(far["T"] - shift @ near["T"] @ np.linalg.inv(shift)).max() < 1e-2


def test_restatement_edge_cases():
    t, s = fx.lattice_pair()
    tn = nref.estimate(t, nc.ICP_NORMAL_K)["normals"]
    sn = nref.estimate(s, nc.ICP_NORMAL_K)["normals"]
    e = np.zeros((0, 3), np.float32)
    for r in (gicp_ref.align(e, e, s, sn), gicp_ref.align(t, tn, e, e), gicp_ref.align(t, tn, s, sn, max_iterations=0)):
        assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 0) and r["fitness"] == gicp_ref.DBL_MAX and (r["T"] == np.eye(4)).all()
    # a correspondence without both normals is dropped; fewer than three left: state 0
    few = tn.copy()
    few[2:] = np.nan
    r = gicp_ref.align(t, few, t[:10].copy(), tn[:10])
    assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 2)
    r = gicp_ref.align(t, tn, t[:10].copy(), few[:10])
    assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 2)
    # a single exact plane does not stop the method: epsilon constrains the in-plane unknowns
    pt, ps = nc.plane_z0()
    r = gicp_ref.align(pt, nref.estimate(pt, nc.ICP_NORMAL_K)["normals"], ps, nref.estimate(ps, nc.ICP_NORMAL_K)["normals"], init=fx.rigid(2.0, (0.1, 0.0, 0.0)))
    assert r["state"] != 5 and r["iterations"] >= 1
    # all correspondences on one line, normals across it: the rotation about the line is not determined -> state 5
    line = np.stack([np.linspace(-4.0, 4.0, 50), np.zeros(50), np.zeros(50)], 1).astype(np.float32)
    up = np.tile(np.float32((0.0, 0.0, 1.0)), (50, 1))
    r = gicp_ref.align(line, up, line[::2] + np.float32((0.01, 0.0, 0.0)), up[::2])
    assert (r["state"], r["converged"], r["iterations"]) == (5, 0, 0)


PROGRAM = r"""
#include "removert/DeviceICP.h"
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
        // a floor and two walls, 21 x 21 points each, and every second point of them moved by (-0.05, 0.02, 0.03)
        ltremovert::Cloud target, source;
        int n = 0;
        for (int face = 0; face < 3; ++face)
            for (int a = 0; a <= 20; ++a)
                for (int b = 0; b <= 20; ++b, ++n) {
                    const float u = 0.5f * a, v = 0.5f * b;
                    const ltremovert::PointType p = face == 0 ? ltremovert::PointType{u, v, 0.0f, 0.0f}
                                                   : face == 1 ? ltremovert::PointType{u, 0.0f, v, 0.0f} : ltremovert::PointType{0.0f, u, v, 0.0f};
                    target.push_back(p);
                    if (n % 2 == 0) source.push_back(ltremovert::PointType{p.x - 0.05f, p.y + 0.02f, p.z + 0.03f, 0.0f});
                }
        ltremovert::DeviceICP icp(ctx);
        icp.setMethod(ltremovert::DeviceICP::Generalized);
        icp.setCorrespondenceRandomness(12);
        icp.setRotationEpsilon(2e-3);
        icp.setViewPoint(5.0f, 5.0f, 5.0f);
        icp.setInputSource(source);
        icp.setInputTarget(target);
        ltremovert::Cloud aligned;
        icp.align(aligned);
        const ltremovert::Matrix4d T = icp.getFinalTransformation();
        const double err = std::fabs(T[3] - 0.05) + std::fabs(T[7] + 0.02) + std::fabs(T[11] + 0.03);
        std::printf("gicp converged %d t %s iterations %s k %d\n", (int)icp.hasConverged(), err < 1e-5 ? "exact" : "off", icp.result().iterations <= 6 ? "few" : "many",
                    icp.getCorrespondenceRandomness());
    }
    ltm_destroy(ctx);
    return 0;
}
"""


def test_host_header_compiles_and_links(tmp_path, ltm):
    ltm.load_library()
    src = tmp_path / "gicp_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "gicp_user"
    pkg = os.path.join(ROOT, "lt-mapper_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", pkg, "-lltm_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    import torch
    if torch.cuda.is_available():
        assert "gicp converged 1 t exact iterations few k 12" in r.stdout, r.stdout
    else:
        assert "no device" in r.stdout, r.stdout
