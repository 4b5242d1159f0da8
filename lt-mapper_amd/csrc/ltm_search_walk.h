// ltm_search_walk.h -- the device side of the search index that more than one kernel unit uses: the Morton code of a point under the index's frame,
// the lower bound of the distance to a node's box, the stackless walk of the implicit box tree, the scan of a leaf's points, the kNN seed and the
// collect (seed leaves, then the walk, into a list of ltm_knn_list.h), and the segmented order by code of the batched
// builds (the index itself is described in ltm_k_search.hip, which builds it; ltm_k_icp.hip walks it for its correspondences).  Everything has
// internal linkage: each unit that includes this gets its own copies, inlined into its kernels.
#pragma once
#include "ltm_kernels_common.h"
#include "ltm_box_bound.h"
#include "ltm_knn_list.h"
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

// lower bound of the float squared distance from q to every point of the node's box (double; +inf for an empty box): ltm_box_bound.h
__device__ __forceinline__ double box_lb(const float4* __restrict__ box, uint32_t node, float qx, float qy, float qz)
{
    const float4 lo = box[2 * node], hi = box[2 * node + 1];
    return box_lower_bound(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qx, qy, qz);
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

// the sorted positions [a, b) of leaf l of an index of Mf finite points
__device__ __forceinline__ void leaf_span(uint32_t l, uint32_t Mf, uint32_t& a, uint32_t& b) { a = l * kSearchLeaf; b = min(a + (uint32_t)kSearchLeaf, Mf); }
// The points of leaf l: f(j, p, d2) with the sorted position, the point and its float distance to q (sqdist_l2simple), in ascending position.  An f that
// returns bool ends the scan by returning false
template <class F>
__device__ __forceinline__ void for_leaf_points(const SearchTree& t, uint32_t l, float qx, float qy, float qz, F f)
{
    uint32_t a, b;
    leaf_span(l, t.Mf, a, b);
    for (uint32_t j = a; j < b; ++j) {
        const float4 p = t.pts[j];
        const float d = sqdist_l2simple(qx, qy, qz, p.x, p.y, p.z);
        if constexpr (std::is_void_v<decltype(f(j, p, d))>) f(j, p, d);
        else if (!f(j, p, d)) break;
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
// The kk nearest target points of q into a KnnListReg (ltm_knn_list.h; initialised by the caller, 1 <= kk <= t.Mf), given as list.slots(): the seed leaves
// around seed_key, the code of q under the index's frame, then the walk that skips a box only when its bound is STRICTLY above the current kk-th distance
template <class Slots>
__device__ __forceinline__ void knn_collect(const SearchTree& t, uint64_t seed_key, uint32_t kk, float qx, float qy, float qz, Slots s)
{
    auto visit = [&, s](uint32_t l) {
        for_leaf_points(t, l, qx, qy, qz, [&, s](uint32_t j, const float4&, float d) { s.push(d, (int)t.idx[j], j); });
    };
    uint32_t sa, sb;
    seed_leaves(t, seed_key, kk, sa, sb);
    for (uint32_t l = sa; l <= sb; ++l) visit(l);
    walk(t, qx, qy, qz, sa, sb, [s](double lb) { return lb > (double)s.kth(); }, visit);
}

// ---------------------------------------------------------------------------------------- segmented order by code
// "Every record's points in Morton order under that record's frame" ("batches"): codes, one segmented sort, gather.  Rec is a SegSource; a
// workgroup of kSegBlock threads takes kSegBlock * PER_THREAD points of one record.  keys[first + j] = code of point j (non-finite: ~0), idx[first + j] = j
static constexpr int kSegBlock = 256;
template <class Rec, int PER_THREAD>
__global__ void __launch_bounds__(kSegBlock)
k_seg_keys(const Rec* __restrict__ recs, const uint32_t* __restrict__ owner, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx)
{
    uint32_t base;
    const Rec& S = block_record<kSegBlock * PER_THREAD>(recs, owner, base);
#pragma unroll
    for (int it = 0; it < PER_THREAD; ++it) {
        const uint32_t local = base + it * kSegBlock + threadIdx.x;
        if (local >= S.n) continue;
        const float4 p = S.src[local];
        keys[S.first + local] = search_key(S.f, p.x, p.y, p.z);
        idx[S.first + local] = local;
    }
}
// sorted[first + j] = src[order[first + j]] for the first n_gather sorted positions of every record
template <class Rec, int PER_THREAD>
__global__ void __launch_bounds__(kSegBlock)
k_seg_gather(const Rec* __restrict__ recs, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ order, float4* __restrict__ sorted)
{
    uint32_t base;
    const Rec& S = block_record<kSegBlock * PER_THREAD>(recs, owner, base);
#pragma unroll
    for (int it = 0; it < PER_THREAD; ++it) {
        const uint32_t local = base + it * kSegBlock + threadIdx.x;
        if (local >= S.n_gather) continue;
        const uint32_t j = order[S.first + local];
        if (j < S.n) sorted[S.first + local] = S.src[j];
    }
}
// the full 63-bit code leaves no room for a record prefix in a 64-bit key: a segmented sort (not stable: equal codes may change places, no result depends on it)
template <class Rec, int PER_THREAD>
hipError_t seg_order_by_code(const Rec* recs, const uint32_t* owner, uint32_t n_blocks, size_t n_recs, const uint64_t* offsets, size_t total, uint64_t* keys,
                             uint64_t* keys_sorted, uint32_t* idx, uint32_t* order, float4* sorted, void* temp, size_t temp_bytes, hipStream_t s)
{
    if (!n_blocks || !total) return hipSuccess;
    k_seg_keys<Rec, PER_THREAD><<<dim3(n_blocks), dim3(kSegBlock), 0, s>>>(recs, owner, keys, idx);
    hipError_t e = seg_sort_pairs_u64(keys, keys_sorted, idx, order, total, n_recs, offsets, temp, temp_bytes, s);
    if (e != hipSuccess) return e;
    k_seg_gather<Rec, PER_THREAD><<<dim3(n_blocks), dim3(kSegBlock), 0, s>>>(recs, owner, order, sorted);
    return hipGetLastError();
}

} // namespace
} // namespace ltm
