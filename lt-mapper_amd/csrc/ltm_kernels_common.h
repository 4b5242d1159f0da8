// ltm_kernels_common.h -- what the kernel translation units of libltm_hip.so share (internal; the launch wrappers are declared in ltm_kernels.h).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (bit-exact parity with the reference's non-FMA x86-64 arithmetic; see ltm_device_math.h).
//
// Data layout in HBM: clouds are float4 XYZI arrays (16 B/pt, one coalesced dwordx4 load per lane); a range image is ONE 64-bit word per pixel,
// (range_bits << 32) | point_index, so that the serial reference rule "strictly smaller range wins, lowest index wins ties" (utility.cpp:134-138) is
// a single order on uint64 and a single global_atomic_umin_x2; scan images only need the range (u32).  Images of a whole batch of keyframes are
// resident at once ([kf][row][col]); one launch covers (map tiles) x (keyframes).
#pragma once
#include "ltm_kernels.h"
#include "ltm_device_math.h"
#include "ltm_device_prims.h"

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <hip/hip_runtime.h>

namespace ltm {

static constexpr int kBlock = 256;

__host__ __device__ inline RimgGeom make_geom(Geom g)
{
    RimgGeom r;
    r.vfov = g.vfov; r.hfov = g.hfov;
    r.half_v = g.vfov / 2.0f; r.half_h = g.hfov / 2.0f;
    r.inv_v = 1.0f / g.vfov; r.inv_h = 1.0f / g.hfov;
    r.fast = g.fast != 0;
    r.eps = g.cull_eps_px;
    r.el_c0 = g.el_c[0]; r.el_c1 = g.el_c[1]; r.el_c2 = g.el_c[2]; r.el_c3 = g.el_c[3]; r.el_tclamp = g.el_tclamp; r.el_fit = g.el_fit != 0;
    r.rows = g.rows; r.cols = g.cols;
    r.frows = (float)g.rows; r.fcols = (float)g.cols;
    r.row_max = (float)(g.rows - 1); r.col_max = (float)(g.cols - 1);
    return r;
}

// What a projection launch needs that depends only on the launch (image shape, extrinsic, map size): filled once on the host by make_proj_launch and
// passed by value, so every field sits in scalar registers.  gfx950 has no scalar float unit: the same expressions evaluated in the kernels cost VALU
// issue slots and VGPRs in every one of the ~10^6 workgroups of a full-map launch.  Every float is computed with exactly the expression and operand
// order the kernels used (binary32, no contraction, correctly rounded division and square root on both sides), so the bits are the same.
static constexpr unsigned kKfPerTile = 8;      // keyframes that reuse one map tile on an XCD (4 / 16 measured no better in round 2)
struct ProjLaunch {
    RimgGeom g;
    float row_scale, col_scale;        // pixels per radian: rows * (180/pi / vfov), cols * (180/pi / hfov)
    float row_bias, col_bias;          // rows/2 + 0.5 - eps, cols/2 + 0.5 - eps (cull_candidates: rowh / colh)
    float certain_lim;                 // 1 - 2 eps
    float rmin2;                       // square of cull_min_range: nearer points take the exact path (0 with an identity base->lidar)
    uint32_t npx;                      // rows * cols
    uint32_t n_tiles, n_tg;            // 4096-point map tiles, groups of 8 tiles (tile_kf_of_block)
    uint32_t tg_magic, tg_shift;       // (b >> 6) / n_tg == mulhi(b & ~63, tg_magic) >> tg_shift for every b < 2^32
    bool steep_clamps;                 // vfov < 88: every elevation beyond +-45 deg clamps into the first / last row
    bool packable;                     // rows < 511 and cols <= 2048: row and column fit the 9 + 11 bits of a queue word (k_map_rimg_blockmin)
    // k_vote_map_cull's queue word carries the pixel as a linear index in kVoteQueuePxBits bits, all ones = "pixel not certain":
    bool vote_queueable;               // npx <= kVoteQueuePxLimit, i.e. every pixel index is below the all-ones value; other shapes take the exact path per tile
    uint32_t px_magic, px_shift;       // px / cols == mulhi(px << 6, px_magic) >> px_shift for every px < 2^26 (group_quotient_magic with d = cols): the row of a queued pixel
};
// The queue word of k_vote_map_cull: (tile in run) 4 bits | (group of 256 points in the tile) 4 bits | lane 6 bits | pixel 18 bits.  The wave is implied: a wave
// drains only what it queued.  The field widths do not depend on the run length, so neither does the condition: npx <= 2^18 - 1 = 262143 (the largest
// pixel index npx - 1 stays below the all-ones value).  With hfov 360 that admits vfov 50 up to alpha 1372 / 360 = 3.811 (191 x 1372 = 262052; 191 x 1373 = 262243
// is the first shape that does not fit) and vfov 90 x 2.5 (225 x 900 = 202500); the shipped workloads use vfov 50 with alpha <= 2.5 (125 x 900 = 112500).
static constexpr uint32_t kVoteQueuePxBits = 18u;
static constexpr uint32_t kVoteQueuePxUncertain = (1u << kVoteQueuePxBits) - 1u;
static constexpr uint32_t kVoteQueuePxLimit = kVoteQueuePxUncertain;      // largest npx of the fast path
// row and column of a queued pixel index: one multiply-high, one shift, one multiply-subtract (px < 2^18 << 2^26, so group_quotient_magic's proof covers it)
__host__ __device__ inline void vote_queue_row_col(uint32_t px, uint32_t cols, uint32_t px_magic, uint32_t px_shift, uint32_t& row, uint32_t& col)
{
    row = (uint32_t)(((uint64_t)(px << 6) * px_magic) >> 32) >> px_shift;
    col = px - row * cols;
}
// (b >> 6) / n_groups == mulhi(b & ~63, magic) >> shift for every b < 2^32:
// q = b >> 6 < 2^26 and d = n_groups <= 2^s: with m = floor(2^(26+s) / d) + 1 = (2^(26+s) + e) / d, 0 < e <= d, q m / 2^(26+s) = q/d + q e / (d 2^(26+s)) and
// q e < 2^(26+s), so the floor is floor(q / d); m < 2^27 + 1.  q m / 2^26 is the high word of (q << 6) m.
__host__ __device__ inline void group_quotient_magic(uint32_t n_groups, uint32_t& magic, uint32_t& shift)
{
    const uint32_t d = n_groups ? n_groups : 1u;
    uint32_t s = 0;
    while (((uint64_t)1 << s) < d) ++s;
    shift = s;
    magic = (uint32_t)((((uint64_t)1 << (26u + s)) / d) + 1u);
}
__host__ __device__ inline ProjLaunch make_proj_launch(Geom gg, const HostMat34& b2l, int b2l_identity, size_t M)
{
    ProjLaunch pl;
    const RimgGeom g = make_geom(gg);
    pl.g = g;
    pl.row_scale = g.frows * (57.29577951308232f / g.vfov); pl.col_scale = g.fcols * (57.29577951308232f / g.hfov);
    pl.row_bias = 0.5f * g.frows + 0.5f - g.eps; pl.col_bias = 0.5f * g.fcols + 0.5f - g.eps;
    pl.certain_lim = 1.0f - 2.0f * g.eps;
    float rmin = 0.0f;
    if (!b2l_identity) {      // see cull_min_range
        const float tx = (float)b2l.m[3], ty = (float)b2l.m[7], tz = (float)b2l.m[11];
        rmin = 0.125f * __builtin_sqrtf(tx * tx + ty * ty + tz * tz) + 1.0e-6f;
    }
    pl.rmin2 = rmin * rmin;
    pl.npx = (uint32_t)(g.rows * g.cols);
    pl.steep_clamps = g.vfov < 88.0f;
    pl.packable = g.rows < 511 && g.cols <= 2048;
    pl.vote_queueable = g.rows > 0 && g.cols > 0 && (uint64_t)g.rows * (uint64_t)g.cols <= kVoteQueuePxLimit;
    group_quotient_magic((uint32_t)g.cols, pl.px_magic, pl.px_shift);
    const size_t per_block = (size_t)kBlock * 16;
    pl.n_tiles = (uint32_t)((M + per_block - 1) / per_block);
    pl.n_tg = (pl.n_tiles + 7u) >> 3;
    group_quotient_magic(pl.n_tg, pl.tg_magic, pl.tg_shift);
    return pl;
}

// XCD-aware workgroup -> (map tile, keyframe) mapping.  Workgroup b runs on XCD b % 8 (observed dispatch rule; used for speed
// only, any other placement is still correct).  Consecutive workgroups of one XCD take the SAME map tile for kKfPerTile
// consecutive keyframes, so the tile (64 KB) is fetched from HBM / Infinity Cache once and served from that XCD's L2
// for the other keyframes: with ~224 resident workgroups per XCD the live tile set is ~28 x 64 KB << 4 MiB of L2.
// b = ((kg * n_tg + tg) * kKfPerTile + kfl) * 8 + x  ->  tile = tg * 8 + x, keyframe = kg * kKfPerTile + kfl.  The quotient by n_tg comes from the
// launch's multiply-high constant and the rest are shifts: the block index is uniform, so all of it runs on the scalar unit.
struct TileKf { uint32_t tile, kfb; bool valid; };
__host__ __device__ inline TileKf tile_kf_of_block(uint32_t b, const ProjLaunch& pl, uint32_t nb)
{
    static_assert(kKfPerTile == 8, "the shifts below are log2(8 XCDs) + log2(kKfPerTile)");
    const uint32_t x = b & 7u, kfl = (b >> 3) & (kKfPerTile - 1u), q = b >> 6;
    const uint32_t kg = (uint32_t)(((uint64_t)(b & ~63u) * pl.tg_magic) >> 32) >> pl.tg_shift;
    const uint32_t tg = q - kg * pl.n_tg;
    TileKf t;
    t.tile = tg * 8u + x;
    t.kfb = kg * kKfPerTile + kfl;
    t.valid = (t.tile < pl.n_tiles) & (t.kfb < nb);
    return t;
}
static inline unsigned tile_kf_grid(size_t n_tiles, size_t nb)
{
    const size_t n_tg = (n_tiles + 7) / 8, n_kg = (nb + kKfPerTile - 1) / kKfPerTile;
    return (unsigned)(n_tg * 8 * kKfPerTile * n_kg);
}

// The vote kernel's form of the mapping: a workgroup takes a RUN of T consecutive map tiles for one keyframe, so what depends on the keyframe only (pose,
// image bases, the LDS pixel table and its flush) is paid once per run.  Run r covers tiles [r T, min((r + 1) T, n_tiles)); the runs take the place
// of the tiles in the mapping above (same XCD placement, same 8 keyframes per run on an XCD), so T = 1 is tile_kf_of_block.
static constexpr uint32_t kMaxTileRun = 16;    // the deferred-survivor queue holds (tile in run) << 12 | (point in tile) in 16 bits
struct RunLaunch {
    uint32_t T;                        // tiles per run, 1 .. kMaxTileRun
    uint32_t n_runs, n_rg;             // runs of T tiles, groups of 8 runs
    uint32_t rg_magic, rg_shift;       // (b >> 6) / n_rg, see group_quotient_magic
};
__host__ __device__ inline RunLaunch make_run_launch(uint32_t n_tiles, uint32_t T)
{
    RunLaunch rl;
    rl.T = T < 1u ? 1u : (T > kMaxTileRun ? kMaxTileRun : T);
    rl.n_runs = n_tiles / rl.T + (n_tiles % rl.T ? 1u : 0u);
    rl.n_rg = (rl.n_runs + 7u) >> 3;
    group_quotient_magic(rl.n_rg, rl.rg_magic, rl.rg_shift);
    return rl;
}
struct RunKf { uint32_t run, kfb; bool valid; };
__host__ __device__ inline RunKf run_kf_of_block(uint32_t b, const RunLaunch& rl, uint32_t nb)
{
    static_assert(kKfPerTile == 8, "the shifts below are log2(8 XCDs) + log2(kKfPerTile)");
    const uint32_t x = b & 7u, kfl = (b >> 3) & (kKfPerTile - 1u), q = b >> 6;
    const uint32_t kg = (uint32_t)(((uint64_t)(b & ~63u) * rl.rg_magic) >> 32) >> rl.rg_shift;
    const uint32_t rg = q - kg * rl.n_rg;
    RunKf t;
    t.run = rg * 8u + x;
    t.kfb = kg * kKfPerTile + kfl;
    t.valid = (t.run < rl.n_runs) & (t.kfb < nb);
    return t;
}
static inline unsigned run_kf_grid(const RunLaunch& rl, size_t nb) { return tile_kf_grid(rl.n_runs, nb); }

inline unsigned grid_for(size_t n, int block = kBlock)
{
    size_t b = (n + block - 1) / block;
    return (unsigned)(b == 0 ? 1 : b);
}

__device__ __forceinline__ Mat34 load_mat(const double* p)
{
    Mat34 T;
#pragma unroll
    for (int i = 0; i < 12; ++i) T.m[i] = p[i];
    return T;
}
__device__ __forceinline__ Mat34 to_dev(const HostMat34& h)
{
    Mat34 T;
#pragma unroll
    for (int i = 0; i < 12; ++i) T.m[i] = h.m[i];
    return T;
}

// range-min with a relaxed pre-test: the image only ever decreases, so a stale (larger) value read
// can only let a redundant atomic through, never suppress a needed one.
__device__ __forceinline__ void img_min_u64(uint64_t* p, uint64_t v)
{
    const uint64_t cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v < cur) atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}
__device__ __forceinline__ void img_min_u32(uint32_t* p, uint32_t v)
{
    const uint32_t cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v < cur) atomicMin(p, v);
}

// keyframe of global point index gi (binary search over the offset table)
__device__ __forceinline__ size_t find_kf(const uint64_t* __restrict__ offsets, size_t lo, size_t hi, uint64_t gi)
{
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= gi) lo = mid; else hi = mid;
    }
    return lo;
}

// the sum over the 64 lanes in 64 bits: a lane's count fits 32 bits, the sum of 64 of them need not
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ uint32_t ballot_count(bool b) { return (uint32_t)__popcll(__ballot(b)); }
// the counters of a thread into the call's: one atomic per wavefront and counter
__device__ __forceinline__ void count_up(unsigned long long* __restrict__ stats, int slot, uint32_t v)
{
    const unsigned long long s = wave_sum64(v);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(stats + slot, s);
}

} // namespace ltm
