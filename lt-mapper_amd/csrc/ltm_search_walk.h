// ltm_search_walk.h -- the device side of the search index that more than one kernel unit uses: the Morton code of a point under the index's frame,
// the order of (distance, index) pairs, the lower bound of the distance to a node's box, the stackless walk of the implicit box tree and the kNN
// seed (the index itself is described in ltm_k_search.hip, which builds it; ltm_k_icp.hip walks it for its correspondences).  Everything has
// internal linkage: each unit that includes this gets its own copies, inlined into its kernels.
#pragma once
#include "ltm_kernels_common.h"
namespace ltm {
namespace {

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }
__device__ __forceinline__ uint32_t quant21(float v, double o, double scale)
{
    const double t = floor(((double)v - o) * scale);
    return (uint32_t)fmin(fmax(t, 0.0), 2097151.0);
}
__device__ __forceinline__ uint64_t search_key(const SearchFrame& f, float x, float y, float z)
{
    if (!finite3(x, y, z)) return ~0ull;
    return morton3(quant21(x, f.ox, f.scale), quant21(y, f.oy, f.scale), quant21(z, f.oz, f.scale));
}
// (d, i) goes before (bd, bi): smaller distance, then smaller target index
__device__ __forceinline__ bool pair_less(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

// lower bound of the squared distance from q to the node's box (double; +inf for an empty box)
__device__ __forceinline__ double box_lb(const float4* __restrict__ box, uint32_t node, float qx, float qy, float qz)
{
    const float4 lo = box[2 * node], hi = box[2 * node + 1];
    const double gx = fmax(fmax((double)lo.x - (double)qx, (double)qx - (double)hi.x), 0.0);
    const double gy = fmax(fmax((double)lo.y - (double)qy, (double)qy - (double)hi.y), 0.0);
    const double gz = fmax(fmax((double)lo.z - (double)qz, (double)qz - (double)hi.z), 0.0);
    return (gx * gx + gy * gy + gz * gz) * (1.0 - 1.0e-6);
}

// Stackless depth-first walk of the implicit tree.  skip(lb) decides with the CURRENT state of the caller's result; leaves in
// [skip_a, skip_b] were visited already (the kNN seed) and are not visited again.
template <class Skip, class Visit>
__device__ __forceinline__ void walk(const SearchTree& t, float qx, float qy, float qz, uint32_t skip_a, uint32_t skip_b, Skip skip, Visit visit)
{
    uint32_t node = 1;
    while (true) {
        if (node < t.P) {
            if (!skip(box_lb(t.box, node, qx, qy, qz))) { node <<= 1; continue; }
        } else {
            const uint32_t l = node - t.P;
            if (l < t.L && !(l >= skip_a && l <= skip_b) && !skip(box_lb(t.box, node, qx, qy, qz))) visit(l);
        }
        while (node & 1u) node >>= 1;      // a right child: climb until a left child (the root climbs to 0: done)
        if (node == 0) break;
        ++node;
    }
}

// first position in the sorted codes whose code is >= key
__device__ __forceinline__ uint32_t lower_bound_key(const uint64_t* __restrict__ keys, uint32_t n, uint64_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// kNN seed: the leaves around the query's position in Morton order that hold at least kk points
__device__ __forceinline__ void seed_leaves(const SearchTree& t, uint64_t qkey, uint32_t kk, uint32_t& a, uint32_t& b)
{
    const uint32_t p = lower_bound_key(t.keys, t.Mf, qkey);
    const uint32_t half = kk / 2;
    uint32_t start = p > half ? p - half : 0u;
    if (start + kk > t.Mf) start = t.Mf - kk;
    a = start / kSearchLeaf;
    b = (start + kk - 1) / kSearchLeaf;
}

} // namespace
} // namespace ltm
