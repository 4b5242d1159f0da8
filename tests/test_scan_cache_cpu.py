"""The scan-image cache alone (csrc/ltm_scan_cache.h, no device and no HIP header): a stand-alone program with a fake pool that hands out malloc'ed blocks and
records every free is compiled with g++ under the address and undefined-behaviour sanitizers and run as a child process.  It checks eviction order, the cap's
boundary, the empty cache, drop by scan set, that every buffer is freed exactly once, a bound image added later, and the staged build the builder in
ltm_api_vote.cpp uses (abandoned: everything back and the cache untouched; handed over: all entries in, with fresh stamps)."""
import os
import subprocess

from conftest import ROOT

PROGRAM = r"""
#include "ltm_scan_cache.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

// hands out malloc'ed blocks; a block freed twice or never handed out ends the program, a block never freed is counted at the end
struct FakePool {
    std::map<void*, int> frees;      // every block ever handed out -> times freed
    size_t n_alloc = 0;
    template <class T> T* alloc(size_t bytes = 16)
    {
        void* p = std::malloc(bytes);
        CHECK(p && !frees.count(p));      // (a block is given back to malloc only at the end, so addresses are unique)
        frees[p] = 0; ++n_alloc;
        return static_cast<T*>(p);
    }
    void free(void* p)
    {
        CHECK(p != nullptr);
        auto it = frees.find(p);
        CHECK(it != frees.end());
        CHECK(it->second == 0);
        it->second = 1;
    }
    size_t n_freed() const { size_t n = 0; for (const auto& kv : frees) n += (size_t)kv.second; return n; }
    ~FakePool() { for (auto& kv : frees) std::free(kv.first); }
};

static FakePool pool;

static ScanImgEntry entry(uint64_t ss, int rows, size_t bytes, bool with_q)
{
    return ScanImgEntry{ss, rows, 8, 0, 4, pool.alloc<uint32_t>(), pool.alloc<uint32_t>(), bytes, 0, with_q ? pool.alloc<float>() : nullptr, with_q ? 0.1f : -1.0f};
}
static bool has(ScanCache& c, uint64_t ss, int rows)      // without touching
{
    for (const ScanImgEntry& e : c.entries) if (e.ss == ss && e.rows == rows) return true;
    return false;
}

int main()
{
    {   // eviction strictly by stamp; a touched entry outlives an untouched older one
        ScanCache c([](void* p) { pool.free(p); });
        c.cap = 400;
        for (int r = 1; r <= 4; ++r) c.insert(entry(7, r, 100, r % 2 == 0));      // stamps 1 .. 4, qbound null for 1 and 3
        CHECK(c.held() == 400 && c.stamp == 4);
        CHECK(c.find(7, 9, 8, 0, 4) == nullptr && c.find(7, 1, 9, 0, 4) == nullptr && c.find(7, 1, 8, 1, 4) == nullptr && c.find(7, 1, 8, 0, 3) == nullptr && c.find(8, 1, 8, 0, 4) == nullptr);
        CHECK(c.stamp == 4);                                      // a miss stamps nothing
        ScanImgEntry* e1 = c.find(7, 1, 8, 0, 4);
        CHECK(e1 && e1->rows == 1 && e1->stamp == 5);             // the oldest, touched
        // the cap's boundary: held + need == cap evicts nothing, one byte more exactly one entry
        c.cap = 500;
        const size_t freed0 = pool.n_freed();
        c.make_room(100);
        CHECK(c.entries.size() == 4 && pool.n_freed() == freed0);
        c.make_room(101);
        CHECK(c.entries.size() == 3 && !has(c, 7, 2) && has(c, 7, 1));      // 2 is the least recently stamped now
        CHECK(pool.n_freed() == freed0 + 3);                      // its image, maxima and bound image
        c.make_room(201);
        CHECK(c.entries.size() == 2 && !has(c, 7, 3));            // already room for 200: one more left for the 201st byte
        CHECK(pool.n_freed() == freed0 + 5);                      // entry 3 had no bound image
        c.make_room(400);
        CHECK(c.entries.size() == 1 && has(c, 7, 1) && !has(c, 7, 4));      // the touched entry is the last one standing
        // a request above the cap empties the cache and is still served
        c.make_room(501);
        CHECK(c.entries.empty() && c.held() == 0);
        c.make_room(100000);
        c.insert(entry(7, 5, 100000, false));
        CHECK(c.entries.size() == 1 && c.held() == 100000);
        c.drop(0);
        CHECK(c.entries.empty());
    }
    {   // drop by scan set; 0 drops all
        ScanCache c([](void* p) { pool.free(p); });
        c.insert(entry(1, 1, 10, true)); c.insert(entry(2, 1, 10, false)); c.insert(entry(1, 2, 10, false)); c.insert(entry(3, 1, 10, true));
        const size_t freed0 = pool.n_freed();
        c.drop(1);
        CHECK(c.entries.size() == 2 && has(c, 2, 1) && has(c, 3, 1) && pool.n_freed() == freed0 + 5);
        c.drop(9);
        CHECK(c.entries.size() == 2 && pool.n_freed() == freed0 + 5);
        c.drop(0);
        CHECK(c.entries.empty() && pool.n_freed() == freed0 + 10);
    }
    {   // a bound image added later counts from then on, and its bytes come back on eviction
        ScanCache c([](void* p) { pool.free(p); });
        c.cap = 300;
        c.insert(entry(1, 1, 100, false));
        ScanImgEntry& second = c.insert(entry(1, 2, 100, false));
        CHECK(&second == &c.entries[1] && second.stamp == 2);      // insert returns the entry it made
        float* q = pool.alloc<float>();
        ScanImgEntry* first = c.find(1, 1, 8, 0, 4);
        CHECK(first == &c.entries[0] && first->stamp == 3);
        c.bound_image(*first, q, 100);
        CHECK(first->qbound == q && first->bytes == 200 && first->q_thr == -1.0f && c.held() == 300);
        c.make_room(0);
        CHECK(c.entries.size() == 2);
        const size_t freed0 = pool.n_freed();
        c.make_room(1);                                            // entry 2 is older than the find of entry 1
        CHECK(c.entries.size() == 1 && c.held() == 200 && pool.n_freed() == freed0 + 2);
        c.make_room(101);
        CHECK(c.entries.empty() && c.held() == 0 && pool.n_freed() == freed0 + 5 && pool.frees[q] == 1);
    }
    {   // the staged build: left before the hand-over (an allocation threw half way through the second entry) everything goes back and the cache is as it was
        ScanCache c([](void* p) { pool.free(p); });
        c.insert(entry(1, 1, 100, true));
        const uint64_t stamp0 = c.stamp;
        const size_t freed0 = pool.n_freed(), alloc0 = pool.n_alloc;
        try {
            ScanCacheStage stage(c, 3);
            ScanImgEntry& a = stage.add(5, 10, 8, 0, 4, 200, 0.1f);
            a.buf = pool.alloc<uint32_t>(); a.smax = pool.alloc<uint32_t>(); a.qbound = pool.alloc<float>();
            ScanImgEntry& b = stage.add(5, 11, 8, 0, 4, 100, -1.0f);
            b.buf = pool.alloc<uint32_t>();
            throw std::runtime_error("out of memory");
        } catch (const std::runtime_error&) {}
        CHECK(pool.n_alloc == alloc0 + 4 && pool.n_freed() == freed0 + 4);
        CHECK(c.entries.size() == 1 && c.held() == 100 && c.stamp == stamp0 && c.find(5, 10, 8, 0, 4) == nullptr);
        {   // handed over: all of them in, stamped after everything that was there, and the stage frees nothing
            const uint64_t stamp1 = c.stamp;
            ScanCacheStage stage(c, 3);
            for (int r = 10; r < 13; ++r) {
                ScanImgEntry& e = stage.add(5, r, 8, 0, 4, 100, r == 10 ? 0.1f : -1.0f);
                e.buf = pool.alloc<uint32_t>(); e.smax = pool.alloc<uint32_t>(); e.qbound = r == 10 ? pool.alloc<float>() : nullptr;
            }
            CHECK(c.entries.size() == 1 && c.held() == 100);
            stage.hand_over();
            CHECK(stage.pending.empty() && c.entries.size() == 4 && c.held() == 400);
            for (int r = 10; r < 13; ++r) {
                const ScanImgEntry& e = c.entries[(size_t)(r - 9)];
                CHECK(e.ss == 5 && e.rows == r && e.cols == 8 && e.kb == 0 && e.nb == 4 && e.bytes == 100 && e.stamp == stamp1 + (uint64_t)(r - 9) && e.buf && e.smax);
                CHECK((e.qbound != nullptr) == (r == 10) && e.q_thr == (r == 10 ? 0.1f : -1.0f));
            }
        }
        CHECK(pool.n_freed() == freed0 + 4);
        c.drop(5);
        CHECK(c.entries.size() == 1 && pool.n_freed() == freed0 + 4 + 7);
        c.drop(0);
    }
    // every buffer ever handed out was freed exactly once (FakePool::free has refused a second time and a foreign or null pointer all along)
    CHECK(pool.n_alloc == pool.frees.size() && pool.n_freed() == pool.n_alloc);
    for (const auto& kv : pool.frees) CHECK(kv.second == 1);
    std::printf("scan cache ok: %zu buffers\n", pool.n_alloc);
    return 0;
}
"""


def test_scan_cache_alone_under_host_sanitizers(tmp_path):
    src = tmp_path / "scan_cache_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "scan_cache_user"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                        "-I", os.path.join(ROOT, "lt-mapper_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scan cache ok: " in r.stdout and not r.stderr, r.stdout + r.stderr
