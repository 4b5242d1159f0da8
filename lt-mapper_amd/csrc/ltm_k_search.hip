// ltm_k_search.hip -- exact k-nearest-neighbour and radius search over a device-resident cloud: the counterpart of the reference's
// pcl::KdTreeFLANN members (Session.cpp:18-23, built at :404,457,489, queried at :471,592,627).
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
//
// Index: the finite target points sorted by a 63-bit Morton code (21 bits per axis over their bounding box), cut into leaves of kSearchLeaf
// consecutive points, and an IMPLICIT complete binary tree of axis-aligned boxes over the leaves (node 1 is the root, node v has children 2v and
// 2v+1, leaf l is node P + l with P the leaf count rounded up to a power of two; padding leaves hold an empty box).  Built with one radix sort
// and log2(P) + 1 box passes, traversed without a stack (the implicit layout gives the next node by bit arithmetic).  A uniform grid walked in
// Chebyshev shells was the first plan; its cost grows with the number of empty shells between a query and its k-th neighbour, which is
// unbounded for clusters kilometres apart or queries far outside the map -- the box tree's is not.
//
// Exactness: the distance of a returned pair is FLANN's L2_Simple in float, ((dx*dx)+dy*dy)+dz*dz without contraction (sqdist_l2simple);
// a box is skipped only when the lower bound of the distance to it (box_lower_bound, ltm_box_bound.h: computed in double, shrunk by a relative
// 1e-6 because the float evaluation is within 3e-7 relative of the exact value, then by an absolute 2^-148 because a square that underflows
// loses up to 2^-150 whatever its size, clamped at 0) is STRICTLY above the current k-th distance (kNN) or not below r2 (radius): no point
// that could enter the result, a tie included, is ever skipped, down to clouds so small that every float distance is 0 and up to
// coordinates whose distances overflow to +inf (which sort last, by index).  Ties are ordered by the smaller target index.
#include "ltm_kernels_common.h"
#include "ltm_search_walk.h"      // search_key, pair_less (ltm_knn_list.h), walk, seed_leaves, for_leaf_points, seg_order_by_code
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
namespace ltm {

// ------------------------------------------------------------------------------------------------------------- build
__global__ void __launch_bounds__(kBlock)
k_search_bbox(const float4* __restrict__ pts, size_t n, uint32_t* __restrict__ out)      // out[0..6): box of the finite points (bbox_init), out[6]: their number
{
    BoxAcc box;
    uint32_t cnt = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float4 p = pts[i];
        if (!finite3(p.x, p.y, p.z)) continue;
        box.add(p);
        ++cnt;
    }
    box.wave_reduce();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, off, 64);
    if ((threadIdx.x & 63u) == 0) atomicAdd(&out[6], cnt);
    box.commit<kBlock / 64>(out);
}
hipError_t search_bbox(const float4* pts, size_t n, uint32_t* bbox8, hipStream_t s)
{
    if (!n) return hipSuccess;
    k_search_bbox<<<dim3((unsigned)std::min<size_t>(grid_for(n, kBlock * 8), 1024)), dim3(kBlock), 0, s>>>(pts, n, bbox8);
    return hipGetLastError();
}

__global__ void __launch_bounds__(kBlock)
k_search_keys(const float4* __restrict__ pts, size_t n, SearchFrame f, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    keys[i] = search_key(f, p.x, p.y, p.z);
    idx[i] = (uint32_t)i;
}
hipError_t search_keys(const float4* pts, size_t n, SearchFrame f, uint64_t* keys, uint32_t* idx, hipStream_t s)
{
    if (!n) return hipSuccess;
    k_search_keys<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(pts, n, f, keys, idx);
    return hipGetLastError();
}

// leaf boxes (node P + l); padding leaves get the empty box (+inf, -inf)
__global__ void __launch_bounds__(kBlock)
k_search_leaf_boxes(const float4* __restrict__ pts, uint32_t Mf, uint32_t L, uint32_t P, float4* __restrict__ box)
{
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= P) return;
    const float inf = __builtin_inff();
    float4 lo = make_float4(inf, inf, inf, 0.0f), hi = make_float4(-inf, -inf, -inf, 0.0f);
    if (l < L) {
        uint32_t a, b; leaf_span(l, Mf, a, b);
        for (uint32_t j = a; j < b; ++j) {
            const float4 p = pts[j];
            lo.x = fminf(lo.x, p.x); lo.y = fminf(lo.y, p.y); lo.z = fminf(lo.z, p.z);
            hi.x = fmaxf(hi.x, p.x); hi.y = fmaxf(hi.y, p.y); hi.z = fmaxf(hi.z, p.z);
        }
    }
    box[2 * (P + l)] = lo;
    box[2 * (P + l) + 1] = hi;
}
// one level of inner nodes [lvl, 2 lvl): union of the children's boxes
__global__ void __launch_bounds__(kBlock)
k_search_inner_boxes(uint32_t lvl, float4* __restrict__ box)
{
    const uint32_t v = lvl + blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= 2 * lvl) return;
    const float4 l0 = box[4 * v], h0 = box[4 * v + 1], l1 = box[4 * v + 2], h1 = box[4 * v + 3];
    box[2 * v] = make_float4(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z), 0.0f);
    box[2 * v + 1] = make_float4(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z), 0.0f);
}
hipError_t search_tree_boxes(const float4* sorted_pts, uint32_t Mf, uint32_t L, uint32_t P, float4* box, hipStream_t s)
{
    if (!P) return hipSuccess;
    k_search_leaf_boxes<<<dim3(grid_for(P)), dim3(kBlock), 0, s>>>(sorted_pts, Mf, L, P, box);
    for (uint32_t lvl = P >> 1; lvl >= 1; lvl >>= 1) k_search_inner_boxes<<<dim3(grid_for(lvl)), dim3(kBlock), 0, s>>>(lvl, box);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------- batched build
// One index per keyframe of a scan set (ltm_search_build_scanset), the stages of the build above in segmented form: the grid of the first three kernels is
// over chunks of kSearchSegChunk points of the batch's owner table (ltm_block_table.h), the order by code is the shared one of ltm_search_walk.h.
static constexpr int kSegPerThread = kSearchSegChunk / kBlock;
__global__ void __launch_bounds__(kBlock)
k_search_bbox_seg_init(uint32_t* __restrict__ b, size_t n_words)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_words) b[i] = (i & 7u) < 3u ? 0xffffffffu : 0u;
}
__global__ void __launch_bounds__(kBlock)
k_search_bbox_seg(const SearchSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, uint32_t* __restrict__ out)
{
    __shared__ uint32_t scnt[kBlock / 64];
    uint32_t base, si;
    const SearchSeg& S = block_record<kSearchSegChunk>(segs, block_seg, base, &si);
    BoxAcc box;
    uint32_t cnt = 0;
#pragma unroll
    for (int it = 0; it < kSegPerThread; ++it) {
        const uint32_t local = base + it * kBlock + threadIdx.x;
        if (local >= S.n) continue;
        const float4 p = S.src[local];
        if (!finite3(p.x, p.y, p.z)) continue;
        box.add(p);
        ++cnt;
    }
    box.wave_reduce();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, off, 64);
    if ((threadIdx.x & 63u) == 0) scnt[threadIdx.x >> 6] = cnt;
    box.commit<kBlock / 64>(out + 8 * (size_t)si, true);      // (its barrier orders scnt as well) one set of atomics per workgroup, for its one segment
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (int w = 0; w < kBlock / 64; ++w) c += scnt[w];
        if (c) atomicAdd(&out[8 * (size_t)si + 6], c);
    }
}
hipError_t search_bbox_seg(const SearchSeg* segs, size_t n_segs, const uint32_t* block_seg, uint32_t n_blocks, uint32_t* bbox8, hipStream_t s)
{
    if (!n_segs) return hipSuccess;
    k_search_bbox_seg_init<<<dim3(grid_for(n_segs * 8)), dim3(kBlock), 0, s>>>(bbox8, n_segs * 8);
    if (n_blocks) k_search_bbox_seg<<<dim3(n_blocks), dim3(kBlock), 0, s>>>(segs, block_seg, bbox8);
    return hipGetLastError();
}
size_t seg_sort_pairs_temp_bytes(size_t n, size_t n_segs)
{
    size_t b = 0;
    (void)rocprim::segmented_radix_sort_pairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                              (unsigned)n, (unsigned)n_segs, (const uint64_t*)nullptr, (const uint64_t*)nullptr, 0, 64);
    return std::max<size_t>(b, 16);
}
hipError_t seg_sort_pairs_u64(const uint64_t* keys, uint64_t* keys_sorted, const uint32_t* vals, uint32_t* vals_sorted, size_t n, size_t n_segs,
                              const uint64_t* offsets, void* temp, size_t temp_bytes, hipStream_t s)
{
    return rocprim::segmented_radix_sort_pairs(temp, temp_bytes, keys, keys_sorted, vals, vals_sorted, (unsigned)n, (unsigned)n_segs, offsets, offsets + 1, 0, 64, s);
}
hipError_t search_order_seg(const SearchSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, size_t n_segs, const uint64_t* offsets, size_t total,
                            uint64_t* keys, uint64_t* keys_sorted, uint32_t* idx, uint32_t* order, float4* sorted, void* temp, size_t temp_bytes, hipStream_t s)
{
    return seg_order_by_code<SearchSeg, kSegPerThread>(segs, block_seg, n_blocks, n_segs, offsets, total, keys, keys_sorted, idx, order, sorted, temp, temp_bytes, s);
}
// all box trees in one launch, one workgroup per segment: the leaf boxes, then the inner levels bottom-up with a barrier between two levels (a level reads
// what the same workgroup wrote one level below).  The same min / max over the same leaves as k_search_leaf_boxes / k_search_inner_boxes.
static constexpr int kTreeBlock = 1024;
__global__ void __launch_bounds__(kTreeBlock)
k_search_tree_boxes_seg(const SearchSeg* __restrict__ segs, const float4* __restrict__ sorted, float4* __restrict__ box_all)
{
    const SearchSeg& S = segs[blockIdx.x];
    const uint32_t Mf = S.n_gather, L = S.L, P = S.P;
    if (!P) return;
    const float4* __restrict__ pts = sorted + S.first;
    float4* box = box_all + S.box0;
    const float inf = __builtin_inff();
    for (uint32_t l = threadIdx.x; l < P; l += kTreeBlock) {
        float4 lo = make_float4(inf, inf, inf, 0.0f), hi = make_float4(-inf, -inf, -inf, 0.0f);
        if (l < L) {
            uint32_t a, b; leaf_span(l, Mf, a, b);
            for (uint32_t j = a; j < b; ++j) {
                const float4 p = pts[j];
                lo.x = fminf(lo.x, p.x); lo.y = fminf(lo.y, p.y); lo.z = fminf(lo.z, p.z);
                hi.x = fmaxf(hi.x, p.x); hi.y = fmaxf(hi.y, p.y); hi.z = fmaxf(hi.z, p.z);
            }
        }
        box[2 * (P + l)] = lo;
        box[2 * (P + l) + 1] = hi;
    }
    for (uint32_t lvl = P >> 1; lvl >= 1; lvl >>= 1) {
        __threadfence_block();
        __syncthreads();
        for (uint32_t v = lvl + threadIdx.x; v < 2 * lvl; v += kTreeBlock) {
            const float4 l0 = box[4 * v], h0 = box[4 * v + 1], l1 = box[4 * v + 2], h1 = box[4 * v + 3];
            box[2 * v] = make_float4(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z), 0.0f);
            box[2 * v + 1] = make_float4(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z), 0.0f);
        }
    }
}
hipError_t search_tree_boxes_seg(const SearchSeg* segs, size_t n_segs, const float4* sorted, float4* box, hipStream_t s)
{
    if (!n_segs) return hipSuccess;
    k_search_tree_boxes_seg<<<dim3((unsigned)n_segs), dim3(kTreeBlock), 0, s>>>(segs, sorted, box);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------- query order
// queries sorted by their code under the index's frame: the lanes of a wavefront then walk the same part of the tree (temp: sort_temp_bytes(n))
hipError_t search_query_order(const float4* query, size_t n, SearchFrame f, uint64_t* keys, uint64_t* keys_sorted, uint32_t* idx, uint32_t* order,
                              void* temp, size_t temp_bytes, hipStream_t s)
{
    if (!n) return hipSuccess;
    hipError_t e = search_keys(query, n, f, keys, idx, s);
    if (e != hipSuccess) return e;
    return sort_pairs_u64(keys, keys_sorted, idx, order, n, 64, temp, temp_bytes, s);
}

// ----------------------------------------------------------------------------------------------------------- kNN
// (These two kernels write out the list of ltm_knn_list.h and the collect of ltm_search_walk.h: built on knn_collect they gave the same bytes from the same
// registers and ran 11 % (k = 8) to 15 % (k = 32) slower, DESIGN.md 4.4a.  tests/test_gpu_knn_list_consumers.py holds the copies together.)
// KT in {1, 2, 4, 8, 16}: the KT best (d2, index) pairs live in registers, kept sorted by an insertion network.  For kk < KT the first
// KT - kk slots hold a sentinel of distance -1 that every candidate sorts after, so slot KT-1 is always the kk-th distance.
template <int KT>
__global__ void __launch_bounds__(kBlock)
k_knn_search_reg(const float4* __restrict__ query, size_t n, const uint32_t* __restrict__ order, const uint64_t* __restrict__ qkeys_sorted,
                 SearchTree t, int k, int kk, int32_t* __restrict__ out_idx, float* __restrict__ out_d2)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint32_t qi = order[q];
    const float4 qp = query[qi];
    float bd[KT];
    int bi[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) { const bool sent = j < KT - kk; bd[j] = sent ? -1.0f : __builtin_inff(); bi[j] = sent ? -1 : INT_MAX; }
    const bool ok = kk > 0 && finite3(qp.x, qp.y, qp.z);
    if (ok) {
        auto push = [&](float d, int i) {
            if (!pair_less(d, i, bd[KT - 1], bi[KT - 1])) return;
#pragma unroll
            for (int j = KT - 1; j > 0; --j) {
                const bool before_prev = pair_less(d, i, bd[j - 1], bi[j - 1]);
                const bool before_this = pair_less(d, i, bd[j], bi[j]);
                const float nd = before_prev ? bd[j - 1] : (before_this ? d : bd[j]);
                const int ni = before_prev ? bi[j - 1] : (before_this ? i : bi[j]);
                bd[j] = nd; bi[j] = ni;
            }
            if (pair_less(d, i, bd[0], bi[0])) { bd[0] = d; bi[0] = i; }
        };
        auto visit = [&](uint32_t l) {
            const uint32_t a = l * kSearchLeaf, b = min(a + (uint32_t)kSearchLeaf, t.Mf);
            for (uint32_t j = a; j < b; ++j) {
                const float4 p = t.pts[j];
                push(sqdist_l2simple(qp.x, qp.y, qp.z, p.x, p.y, p.z), (int)t.idx[j]);
            }
        };
        uint32_t sa, sb;
        seed_leaves(t, qkeys_sorted[q], (uint32_t)kk, sa, sb);
        for (uint32_t l = sa; l <= sb; ++l) visit(l);
        walk(t, qp.x, qp.y, qp.z, sa, sb, [&](double lb) { return lb > (double)bd[KT - 1]; }, visit);
    }
    int32_t* oi = out_idx + (size_t)qi * (size_t)k;
    float* od = out_d2 + (size_t)qi * (size_t)k;
#pragma unroll
    for (int j = 0; j < KT; ++j) {
        const int r = j - (KT - kk);      // row position of slot j
        if (r >= 0) { oi[r] = ok ? bi[j] : -1; od[r] = ok ? bd[j] : __builtin_inff(); }
    }
    for (int r = ok ? kk : 0; r < k; ++r) { oi[r] = -1; od[r] = __builtin_inff(); }
}

// 16 < k <= 64: the lists in LDS, [slot][lane] (one wavefront per workgroup: 64 x 64 x 8 B = 32 KB)
static constexpr int kLdsBlock = 64;
__global__ void __launch_bounds__(kLdsBlock)
k_knn_search_lds(const float4* __restrict__ query, size_t n, const uint32_t* __restrict__ order, const uint64_t* __restrict__ qkeys_sorted,
                 SearchTree t, int k, int kk, int32_t* __restrict__ out_idx, float* __restrict__ out_d2)
{
    __shared__ float sd[kMaxSearchK][kLdsBlock];
    __shared__ int si[kMaxSearchK][kLdsBlock];
    const int lane = (int)threadIdx.x;
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint32_t qi = order[q];
    const float4 qp = query[qi];
    const bool ok = kk > 0 && finite3(qp.x, qp.y, qp.z);
    int cnt = 0;
    if (ok) {
        float kth = __builtin_inff();
        auto push = [&](float d, int i) {
            int j;
            if (cnt < kk) j = cnt++;
            else if (pair_less(d, i, sd[kk - 1][lane], si[kk - 1][lane])) j = kk - 1;
            else return;
            while (j > 0 && pair_less(d, i, sd[j - 1][lane], si[j - 1][lane])) { sd[j][lane] = sd[j - 1][lane]; si[j][lane] = si[j - 1][lane]; --j; }
            sd[j][lane] = d; si[j][lane] = i;
            if (cnt == kk) kth = sd[kk - 1][lane];
        };
        auto visit = [&](uint32_t l) {
            const uint32_t a = l * kSearchLeaf, b = min(a + (uint32_t)kSearchLeaf, t.Mf);
            for (uint32_t j = a; j < b; ++j) {
                const float4 p = t.pts[j];
                push(sqdist_l2simple(qp.x, qp.y, qp.z, p.x, p.y, p.z), (int)t.idx[j]);
            }
        };
        uint32_t sa, sb;
        seed_leaves(t, qkeys_sorted[q], (uint32_t)kk, sa, sb);
        for (uint32_t l = sa; l <= sb; ++l) visit(l);
        walk(t, qp.x, qp.y, qp.z, sa, sb, [&](double lb) { return lb > (double)kth; }, visit);
    }
    int32_t* oi = out_idx + (size_t)qi * (size_t)k;
    float* od = out_d2 + (size_t)qi * (size_t)k;
    for (int r = 0; r < cnt; ++r) { oi[r] = si[r][lane]; od[r] = sd[r][lane]; }
    for (int r = cnt; r < k; ++r) { oi[r] = -1; od[r] = __builtin_inff(); }
}

hipError_t knn_search(const float4* query, size_t n, const uint32_t* order, const uint64_t* qkeys_sorted, SearchTree t, int k,
                      int32_t* out_idx, float* out_d2, hipStream_t s)
{
    if (!n) return hipSuccess;
    if (k < 1 || k > kMaxSearchK) return hipErrorInvalidValue;
    const int kk = (int)std::min<size_t>((size_t)k, t.Mf);
    knn_list_dispatch<true>(k, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if constexpr (KT == 0) k_knn_search_lds<<<dim3(grid_for(n, kLdsBlock)), dim3(kLdsBlock), 0, s>>>(query, n, order, qkeys_sorted, t, k, kk, out_idx, out_d2);
        else k_knn_search_reg<KT><<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(query, n, order, qkeys_sorted, t, k, kk, out_idx, out_d2);
    });
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------------------- radius
// count pass: count[qi] = number of target points with d2 < r2 (0 for a non-finite query)
__global__ void __launch_bounds__(kBlock)
k_radius_count(const float4* __restrict__ query, size_t n, const uint32_t* __restrict__ order, SearchTree t, float r2, uint32_t* __restrict__ count)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint32_t qi = order[q];
    const float4 qp = query[qi];
    uint32_t c = 0;
    if (t.Mf && finite3(qp.x, qp.y, qp.z)) {
        walk(t, qp.x, qp.y, qp.z, 1u, 0u, [&](double lb) { return lb >= (double)r2; }, [&](uint32_t l) {
            for_leaf_points(t, l, qp.x, qp.y, qp.z, [&](uint32_t, const float4&, float d) { c += d < r2 ? 1u : 0u; });
        });
    }
    count[qi] = c;
}
// fill pass: the same walk writes (d2 bits << 32 | index) of every hit at offsets[qi] (d2 >= 0: the bits order as the floats)
__global__ void __launch_bounds__(kBlock)
k_radius_fill(const float4* __restrict__ query, size_t n, const uint32_t* __restrict__ order, SearchTree t, float r2, const uint64_t* __restrict__ offsets,
              uint64_t* __restrict__ pairs)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint32_t qi = order[q];
    const float4 qp = query[qi];
    uint64_t o = offsets[qi];
    const uint64_t end = offsets[qi + 1];
    if (o == end) return;
    walk(t, qp.x, qp.y, qp.z, 1u, 0u, [&](double lb) { return lb >= (double)r2; }, [&](uint32_t l) {
        for_leaf_points(t, l, qp.x, qp.y, qp.z, [&](uint32_t j, const float4&, float d) {
            if (d < r2 && o < end) pairs[o++] = ((uint64_t)__float_as_uint(d) << 32) | t.idx[j];
        });
    });
}
// row q: the first min(count, max_nn) pairs of the sorted row -> idx / d2 at out_off[q]
__global__ void __launch_bounds__(kBlock)
k_radius_split(size_t n, const uint64_t* __restrict__ full_off, const uint64_t* __restrict__ out_off, const uint64_t* __restrict__ sorted,
               int32_t* __restrict__ out_idx, float* __restrict__ out_d2)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint64_t a = full_off[q], o = out_off[q], m = out_off[q + 1] - o;
    for (uint64_t j = 0; j < m; ++j) {
        const uint64_t v = sorted[a + j];
        out_idx[o + j] = (int32_t)(uint32_t)v;
        out_d2[o + j] = __uint_as_float((uint32_t)(v >> 32));
    }
}
// off[0..n] = exclusive scan of min(count, cap) (cap 0 = no cap), total in off[n]
struct CapCount {
    uint32_t cap;
    __host__ __device__ uint64_t operator()(uint32_t c) const { return (uint64_t)(cap && c > cap ? cap : c); }
};
__global__ void k_scan_tail(const uint32_t* __restrict__ count, size_t n, uint32_t cap, uint64_t* __restrict__ off)
{
    const uint32_t c = count[n - 1];
    off[n] = off[n - 1] + (uint64_t)(cap && c > cap ? cap : c);
}
size_t radius_scan_temp_bytes(size_t n)
{
    size_t b = 0;
    auto it = rocprim::make_transform_iterator((const uint32_t*)nullptr, CapCount{0});
    (void)rocprim::exclusive_scan(nullptr, b, it, (uint64_t*)nullptr, (uint64_t)0, n, rocprim::plus<uint64_t>());
    return std::max<size_t>(b, 16);
}
hipError_t radius_offsets(const uint32_t* count, size_t n, uint32_t cap, uint64_t* off, void* temp, size_t temp_bytes, hipStream_t s)
{
    if (!n) return hipMemsetAsync(off, 0, sizeof(uint64_t), s);
    auto it = rocprim::make_transform_iterator(count, CapCount{cap});
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, it, off, (uint64_t)0, n, rocprim::plus<uint64_t>(), s);
    if (e != hipSuccess) return e;
    k_scan_tail<<<1, 1, 0, s>>>(count, n, cap, off);
    return hipGetLastError();
}
hipError_t radius_count(const float4* query, size_t n, const uint32_t* order, SearchTree t, float r2, uint32_t* count, hipStream_t s)
{
    if (!n) return hipSuccess;
    k_radius_count<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(query, n, order, t, r2, count);
    return hipGetLastError();
}
size_t radius_sort_temp_bytes(size_t total, size_t n)
{
    size_t b = 0;
    (void)rocprim::segmented_radix_sort_keys(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (unsigned)total, (unsigned)n, (const uint64_t*)nullptr,
                                             (const uint64_t*)nullptr, 0, 64);
    return std::max<size_t>(b, 16);
}
hipError_t radius_fill(const float4* query, size_t n, const uint32_t* order, SearchTree t, float r2, const uint64_t* full_off, uint64_t total_full,
                       const uint64_t* out_off, uint64_t* pairs, uint64_t* pairs_sorted, int32_t* out_idx, float* out_d2, void* temp, size_t temp_bytes, hipStream_t s)
{
    if (!n || !total_full) return hipSuccess;
    k_radius_fill<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(query, n, order, t, r2, full_off, pairs);
    hipError_t e = rocprim::segmented_radix_sort_keys(temp, temp_bytes, pairs, pairs_sorted, (unsigned)total_full, (unsigned)n, full_off, full_off + 1, 0, 64, s);
    if (e != hipSuccess) return e;
    k_radius_split<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(n, full_off, out_off, pairs_sorted, out_idx, out_d2);
    return hipGetLastError();
}

// rows of an empty target / of no query at all: index -1, distance +inf
__global__ void __launch_bounds__(kBlock)
k_knn_empty_rows(size_t n, int32_t* __restrict__ idx, float* __restrict__ d2)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { idx[i] = -1; d2[i] = __builtin_inff(); }
}
hipError_t knn_empty_rows(size_t n, int32_t* idx, float* d2, hipStream_t s)
{
    if (!n) return hipSuccess;
    k_knn_empty_rows<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(n, idx, d2);
    return hipGetLastError();
}

} // namespace ltm
