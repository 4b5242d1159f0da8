"""CPU checks of the ICP interface (no device needed): the defaults are the reference's, the numpy restatement (tools/icp_numpy.py) gives the known
answers, every fixture of the GPU tests (tests/icp_fixtures.py) is one on which the order of the sums does not decide anything discrete, null arguments
are refused before a device could be touched, and the C++ host mirror DeviceICP.h compiles without warnings, links against the library and runs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import icp_fixtures as fx
from conftest import ROOT
from tools import icp_numpy as ref


def test_header_declares_and_library_exports_the_icp_entry_points(ltm):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltm.h")).read(), flags=re.S)
    lib = ltm.load_library()
    for name in ("ltm_icp_default_params", "ltm_icp_align"):
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/ltm.h"
        assert hasattr(lib, name), f"{name} not exported by libltm_hip.so"
        assert name in ltm.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
    assert "ltm_icp_params;" in src and "ltm_icp_result;" in src
    assert hasattr(ltm.Context, "icp_align")
    assert ltm.ICP_RESULT.itemsize == 160 and ltm.ICP_RESULT.fields["fitness"][1] == 128 and ltm.ICP_RESULT.fields["n_corr"][1] == 156


def test_default_params_are_the_reference_values(ltm):
    p = ltm.IcpParams()
    ltm.load_library().ltm_icp_default_params(C.byref(p))
    assert (p.max_corr_dist, p.max_iterations, p.transformation_epsilon, p.euclidean_fitness_epsilon) == (150.0, 100, 1e-6, 1e-6)
    ltm.load_library().ltm_icp_default_params(None)      # a null pointer is ignored
    q = ltm.icp_params(max_corr_dist=1.0)
    assert (q.max_corr_dist, q.max_iterations) == (1.0, 100)


def test_null_context_is_refused(ltm):
    lib = ltm.load_library()
    p = ltm.icp_params()
    res = np.zeros(1, ltm.ICP_RESULT)
    th = (C.c_void_p * 1)(0x1000)
    sh = (C.c_uint64 * 1)(1)
    assert lib.ltm_icp_align(None, 1, th, sh, None, C.byref(p), res.ctypes.data, None) == -1


def test_restatement_known_answer():
    """6 x 5 x 4 unit lattice against every third point of it shifted by (-0.25, 0, 0): one step finds the shift, the second sees no motion"""
    t, s = fx.lattice_pair()
    fx.check_known_answer(ref.align(t, s), 1e-12)


def test_restatement_known_answer_far_from_the_origin():
    """the same with both clouds moved by (+1000.125, -2000.5, 0): 1e-9 holds because the moments are taken about the means (two passes)"""
    t, s = fx.lattice_pair(fx.FAR)
    fx.check_known_answer(ref.align(t, s), 1e-9)


def test_restatement_edge_cases():
    t, s = fx.lattice_pair()
    e = np.zeros((0, 3), np.float32)
    for r in (ref.align(e, s), ref.align(t, e), ref.align(t, s, max_iterations=0)):
        assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 0) and r["fitness"] == ref.DBL_MAX and (r["T"] == np.eye(4)).all()
    r = ref.align(t, s + np.float32(100.0), max_corr_dist=1.0)      # every point beyond the limit
    assert (r["iterations"], r["converged"], r["state"], r["n_corr"]) == (0, 0, 0, 0) and 1e3 < r["fitness"] < 1e5 and r["last_mse"] == ref.DBL_MAX
    assert r["trace"][0, 0] == 0 and np.isnan(r["trace"][0, 1])


def _fixture_condition(target, source, base, **kw):
    """the discrete part of the result is the same whichever order the sums run in, and the transforms stay within the bound the GPU tests use"""
    n = int(np.isfinite(source[:, :3]).all(axis=1).sum())
    worst = 0.0
    for order in (np.arange(n)[::-1], np.random.default_rng(n).permutation(n)):
        r = ref.align(target, source, order=order, **kw)
        assert (r["iterations"], r["state"], r["converged"]) == (base["iterations"], base["state"], base["converged"])
        assert (r["trace"][:, 0] == base["trace"][:, 0])[~np.isnan(base["trace"][:, 0])].all() and (np.isnan(r["trace"][:, 0]) == np.isnan(base["trace"][:, 0])).all()
        worst = max(worst, np.abs(r["T"] - base["T"]).max())
    assert worst <= fx.tol_T(n), (worst, fx.tol_T(n))


def test_fixture_condition_scenes():
    for name in fx.SCENES:
        t, s, base = fx.scene_fixture(name)
        assert base["converged"] == 1 and 3 <= base["iterations"] < 100
        _fixture_condition(t, s, base)


def test_fixture_condition_restart():
    """started from its own answer the restatement stops within two iterations on the fixtures the GPU test asks that of"""
    assert len(fx.RESTART_QUIET) >= 2
    for name in fx.SCENES:
        r = fx.restart_fixture(name)
        assert r["converged"] == 1
        if name in fx.RESTART_QUIET:
            assert r["iterations"] <= 2, (name, r["iterations"])


def test_fixture_condition_outliers():
    t, s, near = fx.outlier_fixture(1.0)
    _, _, far = fx.outlier_fixture(150.0)
    it = near["iterations"]
    assert (near["trace"][:it, 0] == 600).all() and (far["trace"][:far["iterations"], 0] == 640).all()
    assert np.abs(near["T"] - far["T"]).max() > 0.1, "with the outliers kept the alignment ends elsewhere"
    _fixture_condition(t, s, near, max_corr_dist=1.0)
    _fixture_condition(t, s, far, max_corr_dist=150.0)


def test_fixture_condition_edges_and_lattices():
    for t, s, base in fx.edge_fixtures():
        assert base["converged"] == 1
        _fixture_condition(t, s, base)
    for off in ((0.0, 0.0, 0.0), fx.FAR):
        t, s = fx.lattice_pair(off)
        _fixture_condition(t, s, ref.align(t, s))


PROGRAM = r"""
#include "removert/DeviceICP.h"
#include <cstdio>

int main()
{
    ltm_config cfg{};
    cfg.vfov = 50.0f; cfg.hfov = 360.0f;
    for (int i = 0; i < 16; ++i) cfg.lidar2base[i] = (i % 5 == 0) ? 1.0 : 0.0;
    ltm_icp_params prm;
    ltm_icp_default_params(&prm);
    std::printf("defaults %.1f %d %.0e %.0e\n", prm.max_corr_dist, prm.max_iterations, prm.transformation_epsilon, prm.euclidean_fitness_epsilon);
    ltm_ctx* ctx = nullptr;
    const int rc = ltm_create(&cfg, &ctx);
    if (rc != LTM_OK) { std::printf("no device: %d\n", rc); return 0; }
    {
        // the 6 x 5 x 4 unit lattice and every third point of it shifted by -0.25 in x
        ltremovert::Cloud target, source;
        int n = 0;
        for (int x = 0; x < 6; ++x)
            for (int y = 0; y < 5; ++y)
                for (int z = 0; z < 4; ++z, ++n) {
                    target.push_back(ltremovert::PointType{(float)x, (float)y, (float)z, 0.0f});
                    if (n % 3 == 0) source.push_back(ltremovert::PointType{(float)x - 0.25f, (float)y, (float)z, 0.0f});
                }
        ltremovert::DeviceICP icp(ctx);
        icp.setMaxCorrespondenceDistance(150);
        icp.setMaximumIterations(100);
        icp.setTransformationEpsilon(1e-6);
        icp.setEuclideanFitnessEpsilon(1e-6);
        icp.setInputSource(source);
        icp.setInputTarget(target);
        ltremovert::Cloud aligned;
        icp.align(aligned);
        const ltremovert::Matrix4d T = icp.getFinalTransformation();
        std::printf("converged %d fitness %s tx %.6f aligned %zu x %.3f\n", (int)icp.hasConverged(), icp.getFitnessScore() < 1e-24 ? "zero" : "large", T[3],
                    aligned.size(), aligned.back().x);
        // the batched form: the same pair twice, against ONE index
        const std::vector<ltm_icp_result> all = icp.alignAll({&source, &source});
        std::printf("batch %zu iterations %d %d state %d\n", all.size(), all[0].iterations, all[1].iterations, all[1].state);
    }
    ltm_destroy(ctx);
    return 0;
}
"""


def test_device_icp_header_compiles_and_links(tmp_path, ltm):
    ltm.load_library()
    src = tmp_path / "icp_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "icp_user"
    pkg = os.path.join(ROOT, "lt-mapper_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", pkg, "-lltm_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "defaults 150.0 100 1e-06 1e-06" in r.stdout, r.stdout
    import torch
    if torch.cuda.is_available():
        assert "converged 1 fitness zero tx 0.250000 aligned 40 x 5.000" in r.stdout, r.stdout
        assert "batch 2 iterations 2 2 state 2" in r.stdout, r.stdout
    else:
        assert "no device" in r.stdout, r.stdout
