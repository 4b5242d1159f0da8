// ltm_device_prims.h -- arithmetic that several kernel units (and, for the keys, the host side of the C ABI) share, stated once: the order-preserving
// float <-> uint32 key, the 21-bit Morton interleave, the octree key of a point and the bounding-box accumulator of the box reductions.
// Included by ltm_kernels_common.h (kernels) and ltm_internal.h (host: the keys only).
#pragma once
#include "ltm_kernels.h"

#include <hip/hip_runtime.h>

namespace ltm {

// Order-preserving float <-> uint32 key: a < b as floats (with -0.0 below +0.0) iff key(a) < key(b) as unsigned integers, so integer atomicMin / atomicMax
// reduce floats.  No float maps to key 0 or ~0 except the two NaNs with all mantissa bits set: ~0 / 0 serve as the empty min / max.
__host__ __device__ inline uint32_t ordered_key(float f)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ordered_unkey(uint32_t k)
{
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// 21 bits -> every third bit; morton3: x is the most significant bit of each level triple (octree child index = x<<2 | y<<1 | z)
__device__ __forceinline__ uint64_t morton_spread21(uint32_t v)
{
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
__device__ __forceinline__ uint64_t morton3(uint32_t kx, uint32_t ky, uint32_t kz)
{
    return (morton_spread21(kx) << 2) | (morton_spread21(ky) << 1) | morton_spread21(kz);
}
// PCL genOctreeKeyforPoint: key = (unsigned)(((double)p - min) / resolution) per axis, interleaved
__device__ __forceinline__ uint64_t octree_code(const float4 p, const OctreeFrame& f)
{
    const uint32_t kx = (uint32_t)(((double)p.x - f.minx) / f.res);
    const uint32_t ky = (uint32_t)(((double)p.y - f.miny) / f.res);
    const uint32_t kz = (uint32_t)(((double)p.z - f.minz) / f.res);
    return morton3(kx, ky, kz);
}

// Bounding box of the points a thread has seen, as ordered keys.  After the kernel's own loop: wave_reduce() (every lane of the wave), then commit()
// (every thread of the workgroup of kWaves wavefronts): LDS stage across the waves, then ONE set of 6 atomics per workgroup on bbox[0..6) = min xyz, max xyz.
struct BoxAcc {
    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    __device__ __forceinline__ void add(const float4 p)
    {
        const uint32_t e[3] = {ordered_key(p.x), ordered_key(p.y), ordered_key(p.z)};
#pragma unroll
        for (int d = 0; d < 3; ++d) { mn[d] = min(mn[d], e[d]); mx[d] = max(mx[d], e[d]); }
    }
    __device__ __forceinline__ void wave_reduce()
    {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                mn[d] = min(mn[d], (uint32_t)__shfl_xor((int)mn[d], off, 64));
                mx[d] = max(mx[d], (uint32_t)__shfl_xor((int)mx[d], off, 64));
            }
        }
    }
    // skip_empty: no atomics from a workgroup that saw no point (its box is still the empty one)
    template <int kWaves>
    __device__ __forceinline__ void commit(uint32_t* __restrict__ bbox, bool skip_empty = false)
    {
        __shared__ uint32_t smn[3][kWaves], smx[3][kWaves];
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int d = 0; d < 3; ++d) { smn[d][wave] = mn[d]; smx[d][wave] = mx[d]; }
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const int d = threadIdx.x;
            uint32_t lo = smn[d][0], hi = smx[d][0];
            for (int w = 1; w < kWaves; ++w) { lo = min(lo, smn[d][w]); hi = max(hi, smx[d][w]); }
            if (!skip_empty || lo != 0xffffffffu || hi != 0u) { atomicMin(bbox + d, lo); atomicMax(bbox + 3 + d, hi); }
        }
    }
};

} // namespace ltm
