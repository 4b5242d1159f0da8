"""The union-find of the cluster kernels on CPU threads (no device needed): lt-mapper_amd/csrc/ltm_unionfind.h compiles for the host, and a stand-alone program
runs the very same find / unite from 8 std::threads over the edge lists of three fixtures (a long chain, blobs in noise, two piles of duplicates) in
shuffled order.  It checks what the flatten pass of ltm_k_cluster.hip relies on -- every root is the smallest position of its component -- and that the
partition is the one a sequential union-find gives.  Plain g++; with LTM_TEST_TSAN=1 in the environment the same program is also built with
-fsanitize=thread (the stand-alone program only) and has to run clean."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
from conftest import ROOT
from tools import cluster_numpy as cref

PROGRAM = r"""
#include "ltm_unionfind.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <thread>
#include <vector>

static uint32_t seq_find(std::vector<uint32_t>& p, uint32_t x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const uint32_t n = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<uint32_t> e;
    uint32_t buf[2];
    while (std::fread(buf, sizeof(uint32_t), 2, f) == 2) { e.push_back(buf[0]); e.push_back(buf[1]); }
    std::fclose(f);
    const size_t m = e.size() / 2;
    // sequential: union by smaller root
    std::vector<uint32_t> sp(n);
    std::iota(sp.begin(), sp.end(), 0u);
    for (size_t k = 0; k < m; ++k) {
        const uint32_t a = seq_find(sp, e[2 * k]), b = seq_find(sp, e[2 * k + 1]);
        if (a != b) sp[std::max(a, b)] = std::min(a, b);
    }
    // 8 threads, the header's own code
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    const int T = 8;
    std::vector<uint32_t> retries(T, 0u);
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            uint32_t r = 0;
            for (size_t k = (size_t)t; k < m; k += T) ltm::uf::unite(parent.data(), e[2 * k], e[2 * k + 1], &r);
            retries[t] = r;
        });
    for (auto& x : th) x.join();
    size_t bad_root = 0, bad_part = 0, comps = 0;
    std::vector<uint32_t> cmin(n, 0xffffffffu);
    for (uint32_t i = 0; i < n; ++i) { const uint32_t s = seq_find(sp, i); cmin[s] = std::min(cmin[s], i); }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r = ltm::uf::find(parent.data(), i), s = seq_find(sp, i);
        if (r != cmin[s]) ++bad_root;              // the root is the component's minimum
        if (ltm::uf::find(parent.data(), s) != r) ++bad_part;      // same partition
        if (r == i) ++comps;
    }
    uint32_t rt = 0;
    for (uint32_t r : retries) rt += r;
    std::printf("n %u edges %zu components %zu bad_root %zu bad_partition %zu retries %u\n", n, m, comps, bad_root, bad_part, rt);
    return bad_root || bad_part ? 1 : 0;
}
"""


def _edges(name):
    pts, tol, _, _ = cc.CASES[name]
    e, _ = cref.edges(pts, tol)
    e = e[np.random.default_rng(3).permutation(len(e))]
    flip = np.random.default_rng(4).random(len(e)) < 0.5
    e[flip] = e[flip][:, ::-1]
    return len(pts), np.ascontiguousarray(e, np.uint32)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("unionfind")
    src = d / "unionfind_user.cpp"
    src.write_text(PROGRAM)
    exes = []
    variants = [("plain", ["-O2"])]
    if os.environ.get("LTM_TEST_TSAN") == "1":
        variants.append(("tsan", ["-O1", "-g", "-fsanitize=thread"]))
    for name, flags in variants:
        exe = d / f"unionfind_{name}"
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *flags, "-I", os.path.join(ROOT, "lt-mapper_amd", "csrc"), str(src),
                            "-o", str(exe)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        exes.append(exe)
    return d, exes


@pytest.mark.parametrize("name", ["chain_5000", "blobs", "duplicates"])
def test_threads_leave_every_root_at_the_component_minimum(programs, name):
    d, exes = programs
    n, e = _edges(name)
    want = len(cref.cluster(cc.CASES[name][0], cc.CASES[name][1])["sizes"])      # min_size 1: every component
    path = d / f"{name}.edges"
    e.tofile(path)
    for exe in exes:
        r = subprocess.run([str(exe), str(n), str(path)], capture_output=True, text=True, timeout=300)
        print(exe.name, r.stdout.strip())
        assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
        assert f"n {n} edges {len(e)} components {want} bad_root 0 bad_partition 0" in r.stdout, r.stdout
