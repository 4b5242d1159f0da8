"""The host half of the per-workgroup owner table alone (csrc/ltm_block_table.h, no device and no HIP header): a stand-alone program compiled with g++ under
the address and undefined-behaviour sanitizers and run as a child process.  It checks that spans are contiguous and in record order, that every workgroup
of a span names its record, the block counts on both sides of a whole block, records without items, and the limit: refused when reached, with the table
left exactly as it was."""
import os
import subprocess

from conftest import ROOT

PROGRAM = r"""
#include "ltm_block_table.h"
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

using ltm::BlockSpan;
using ltm::BlockTable;

int main()
{
    {   // block counts around a whole block; spans contiguous and in record order; owner[b] == record over every span; no entry for an empty record
        const struct { uint64_t items; uint32_t per_block, blocks; } cases[] = {
            {0, 256, 0}, {1, 256, 1}, {255, 256, 1}, {256, 256, 1}, {257, 256, 2}, {1023, 1024, 1}, {1024, 1024, 1}, {1025, 1024, 2}, {2049, 1024, 3}, {0, 1024, 0}};
        const uint32_t n = (uint32_t)(sizeof cases / sizeof cases[0]);
        BlockTable t;
        BlockSpan spans[sizeof cases / sizeof cases[0]];
        uint32_t at = 0;
        for (uint32_t r = 0; r < n; ++r) {
            CHECK(t.add(100 + r, cases[r].items, cases[r].per_block, &spans[r]));
            CHECK(spans[r].block0 == at && spans[r].n_blocks == cases[r].blocks);
            at += cases[r].blocks;
            CHECK(t.size() == at && t.owner().size() == at);
        }
        CHECK(at == 12);
        for (uint32_t r = 0; r < n; ++r)
            for (uint32_t b = spans[r].block0; b < spans[r].block0 + spans[r].n_blocks; ++b) CHECK(t.owner()[b] == 100 + r);
        // every workgroup belongs to exactly one span
        uint32_t covered = 0;
        for (uint32_t r = 0; r < n; ++r) covered += spans[r].n_blocks;
        CHECK(covered == t.size());
    }
    {   // the limit is refused when REACHED; a refused add changes nothing; a record without items still fits
        BlockTable t(8);
        BlockSpan s{77, 77};
        CHECK(t.add(0, 3 * 256, 256, &s) && s.block0 == 0 && s.n_blocks == 3);
        CHECK(t.add(1, 4 * 256 - 1, 256, &s) && s.block0 == 3 && s.n_blocks == 4);
        CHECK(t.size() == 7);
        const std::vector<uint32_t> before = t.owner();
        s = BlockSpan{77, 77};
        CHECK(!t.add(2, 1, 256, &s));                       // 7 + 1 reaches 8
        CHECK(s.block0 == 77 && s.n_blocks == 77);
        CHECK(t.size() == 7 && t.owner() == before);
        CHECK(!t.add(2, 1ull << 40, 256, &s));              // far beyond it, and beyond 32 bits
        CHECK(t.size() == 7 && t.owner() == before);
        CHECK(t.add(2, 0, 256, &s) && s.block0 == 7 && s.n_blocks == 0);
        CHECK(t.size() == 7 && t.owner() == before);
        BlockTable u(8);
        CHECK(u.add(0, 7 * 1024, 1024, &s) && s.n_blocks == 7 && u.size() == 7);      // one below the limit is accepted in one piece
        BlockTable v(8);
        CHECK(!v.add(0, 7 * 1024 + 1, 1024, &s) && v.size() == 0 && v.owner().empty());
    }
    {   // the default limit: a grid stays below 2^31 - 1 workgroups (checked without building such a table)
        BlockTable t;
        BlockSpan s{5, 5};
        CHECK(!t.add(0, 0x7fffffffull * 256, 256, &s) && t.size() == 0 && s.block0 == 5);
        CHECK(!t.add(0, 0xffffffffffffffffull, 256, &s) && t.size() == 0);
        CHECK(BlockTable::kMaxBlocks == 0x7fffffffull);
    }
    std::printf("block table ok\n");
    return 0;
}
"""


def test_block_table_alone_under_host_sanitizers(tmp_path):
    src = tmp_path / "block_table_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "block_table_user"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                        "-I", os.path.join(ROOT, "lt-mapper_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "block table ok" in r.stdout and not r.stderr, r.stdout + r.stderr
