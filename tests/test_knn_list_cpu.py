"""The k-best list of the search index alone (csrc/ltm_knn_list.h, no device and no HIP header): a stand-alone program compiled with g++ without
contraction under the address and undefined-behaviour sanitizers and run as a child process.  The register list at every KT in {1, 2, 4, 8, 16} and every
kk in 0..KT, pushed through the list and through its by-value slots handle.  (The header holds what the kernel on knn_collect uses; the LDS form and the
forms with fewer payload words, which the search, normals and filter kernels write out, are not in it and are covered by the GPU parity tests and
tests/test_gpu_knn_list_consumers.py.)  Candidates: distinct indices, distances drawn from five values (0, a denormal, two equal finite values, +inf), in
sequences of every length from 0 to kk + 3 and in seeded random sequences of 200.  After EVERY push the live slots must be the kk smallest candidates so
far under pair_less, in that order, the words travelling with their distance, and kth() must be +inf until kk candidates have arrived and the kk-th
distance afterwards."""
import os
import subprocess

from conftest import ROOT

PROGRAM = r"""
#include "ltm_knn_list.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64()      // xorshift64*
{
    state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
    return state * 0x2545f4914f6cdd1dull;
}

struct Cand { float d; int i; uint32_t pos; };
static const float kValues[5] = {0.0f, 0x1p-149f, 2.0f, 2.0f, std::numeric_limits<float>::infinity()};
static uint32_t pos_of(int i) { return (uint32_t)i * 7u + 3u; }      // the second word is a function of the index: a word that strays shows

// n candidates with distinct indices in random order
static std::vector<Cand> sequence(int n)
{
    std::vector<int> idx(n);
    for (int a = 0; a < n; ++a) idx[a] = a * 3 + 1;
    for (int a = n - 1; a > 0; --a) std::swap(idx[a], idx[next_u64() % (uint64_t)(a + 1)]);
    std::vector<Cand> c(n);
    for (int a = 0; a < n; ++a) c[a] = Cand{kValues[next_u64() % 5], idx[a], pos_of(idx[a])};
    return c;
}

// what a list of kk slots must hold after the candidates seen[0 .. n)
static std::vector<Cand> expected(std::vector<Cand> seen, int kk)
{
    std::sort(seen.begin(), seen.end(), [](const Cand& a, const Cand& b) { return a.d < b.d || (a.d == b.d && a.i < b.i); });
    if ((int)seen.size() > kk) seen.resize(kk);
    return seen;
}

// the live slots of `list` against `want` (ranks 0 .. in ascending order), and kth()
template <class List>
static void check(const List& list, const std::vector<Cand>& want, int kk, int n_pushed)
{
    std::vector<Cand> got;
    int next_rank = 0;
    list.for_each([&](int r, float d, int i, uint32_t pos) {
        CHECK(r == next_rank);
        ++next_rank;
        got.push_back(Cand{d, i, pos});
    });
    // the list shows its kk slots from the start (+inf, no index)
    CHECK((int)got.size() == kk && got.size() >= want.size());
    for (size_t a = 0; a < got.size(); ++a) {
        if (a >= want.size()) { CHECK(std::isinf(got[a].d) && got[a].d > 0.0f && got[a].i == INT_MAX); continue; }
        CHECK(got[a].d == want[a].d && got[a].i == want[a].i && got[a].pos == want[a].pos && got[a].pos == pos_of(got[a].i));
        if (a > 0) CHECK(got[a - 1].d <= got[a].d);
    }
    if (kk > 0) {
        const float inf = std::numeric_limits<float>::infinity();
        CHECK(list.kth() == (n_pushed < kk ? inf : want[kk - 1].d));
    }
}

static long n_checks = 0;
template <int KT>
static void run_reg()
{
    for (int kk = 0; kk <= KT; ++kk) {
        auto one = [&](const std::vector<Cand>& seq, bool through_slots) {
            ltm::KnnListReg<KT> list;
            list.init(kk);
            check(list, {}, kk, 0);
            std::vector<Cand> seen;
            for (const Cand& c : seq) {
                // both doors: the list's own push and the by-value handle the tree walk uses
                if (through_slots) list.slots().push(c.d, c.i, c.pos); else list.push(c.d, c.i, c.pos);
                seen.push_back(c);
                check(list, expected(seen, kk), kk, (int)seen.size());
                ++n_checks;
            }
        };
        for (int n = 0; n <= kk + 3; ++n)
            for (int rep = 0; rep < 8; ++rep) one(sequence(n), rep & 1);
        for (int rep = 0; rep < 4; ++rep) one(sequence(200), rep & 1);
    }
}

template <bool SMALL>
static int form_of(int slots)
{
    int kt = -1;
    ltm::knn_list_dispatch<SMALL>(slots, [&](auto c) { kt = decltype(c)::value; });
    return kt;
}

int main()
{
    CHECK(ltm::pair_less(1.0f, 5, 2.0f, 0) && !ltm::pair_less(2.0f, 0, 1.0f, 5) && ltm::pair_less(1.0f, 2, 1.0f, 3) && !ltm::pair_less(1.0f, 3, 1.0f, 3));
    CHECK(ltm::pair_less(0.0f, 0, 0x1p-149f, 0) && ltm::pair_less(3e38f, 7, kValues[4], 0) && ltm::pair_less(kValues[4], 1, kValues[4], 2));
    run_reg<1>(); run_reg<2>(); run_reg<4>(); run_reg<8>(); run_reg<16>();
    // the form that holds a number of slots: the smallest register form, the LDS form (0) past 16
    const int small[] = {1, 2, 4, 4, 8, 8, 8, 8, 16, 16, 16, 16, 16, 16, 16, 16, 0};
    for (int s = 1; s <= 17; ++s) { CHECK(form_of<true>(s) == small[s - 1]); CHECK(form_of<false>(s) == (s <= 4 ? 4 : small[s - 1])); }
    CHECK(form_of<true>(64) == 0 && form_of<false>(64) == 0);
    std::printf("%ld states checked\n", n_checks);
    std::printf("knn list ok\n");
    return 0;
}
"""


def test_knn_list_alone_under_host_sanitizers(tmp_path):
    src = tmp_path / "knn_list_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "knn_list_user"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-g", "-O1", "-I", os.path.join(ROOT, "lt-mapper_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "knn list ok" in r.stdout and not r.stderr, r.stdout + r.stderr
