// ltm_k_cluster.hip -- Euclidean cluster extraction over the targets of search indices: connected components under a distance tolerance with a size filter,
// the counterpart of pcl::EuclideanClusterExtraction.  The reference does not call it; the semantics are stated in include/ltm.h, "clusters".
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
//
// Hook pass: one thread per finite target point in the index's own (Morton) order -- the lanes of a wavefront are neighbours in space and walk the same part
// of the box tree, no query sort.  All indices of a call go through ONE launch over the batch's owner table (ltm_block_table.h).  The thread walks the implicit tree with skip(lb) = lb >= r2 and, in a visited leaf, tests only the points at a
// LOWER sorted position: every edge is seen once, from its higher end.  The walk is the stackless one of ltm_search_walk.h with one addition: the leaves
// come in ascending position, so it ends at the first node whose leaves all lie at or above the thread's own position (half of every walk).  On
// d2 < r2 the two points are united in the lock-free union-find of ltm_unionfind.h over positions local to the index.
//
// Why it is correct on this hardware and why it terminates: the header of ltm_unionfind.h.  In short -- a root is only ever hooked under a SMALLER root by a
// device-scope atomicCAS, which is performed in memory beyond the XCDs' L2s; a failed CAS restarts from the value it returned (strictly smaller: at most
// a + b retries for unite(a, b), nobody waits for anybody); find() may read stale parents (a stale parent is still an ancestor) and compresses paths with
// plain stores of values it has read, which only ever touch non-roots.  The flatten pass is a launch of its own, so the kernel boundary orders it after all
// hooks and makes every store visible: root[i] = find(i) is then the smallest sorted position of i's component, whatever the schedule was.
//
// Clique leaves: a leaf (kSearchLeaf consecutive points) whose box diagonal, squared in double, enlarged by a relative 1e-6 (the float distance is within
// 3e-7 relative of the exact one) and by 2^-148 (squares that underflow round up by half a denormal each), is below r2 is a clique: box_is_clique of
// ltm_box_bound.h, host and device.  The init pass points all its positions at its first one with plain stores (nothing else runs),
// a walk that finds one hit in such a leaf stops scanning it, and a thread does not scan its own clique leaf at all.
//
// Bookkeeping, integer atomics only: size and lowest original index per root; the roots that pass the size filter are compacted, sorted per index by
// (size descending, lowest original index) and numbered; labels in original order; one sort of (cluster, original index) gives the CSR; boxes and centroids
// come from a segmented pass over the CSR in a fixed shape (256-point chunks summed by a tree, chunk sums combined 64 at a time by a tree, groups in
// order), so that two runs give the same bytes.
#include "ltm_kernels_common.h"
#include "ltm_search_walk.h"      // box_lb
#include "ltm_unionfind.h"
#include <rocprim/device/device_scan.hpp>
namespace ltm {

namespace {

__device__ __forceinline__ bool leaf_is_clique(const float4* __restrict__ box, uint32_t node, float r2)
{
    const float4 lo = box[2 * node], hi = box[2 * node + 1];
    return box_is_clique(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, r2);
}

// the walk of ltm_search_walk.h restricted to sorted positions below j: the depth-first order visits the leaves in ascending position, so the walk is
// over at the first node whose first position is not below j
template <class Visit>
__device__ __forceinline__ void walk_below(const SearchTree& t, uint32_t logP, uint32_t j, float qx, float qy, float qz, double r2, Visit visit)
{
    uint32_t node = 1;
    while (true) {
        const uint32_t level = 31u - (uint32_t)__clz((int)node);
        const uint32_t first = ((node << (logP - level)) - t.P) * (uint32_t)kSearchLeaf;
        if (first >= j) break;
        if (node < t.P) {
            if (!(box_lb(t.box, node, qx, qy, qz) >= r2)) { node <<= 1; continue; }
        } else {
            const uint32_t l = node - t.P;
            if (l < t.L && !(box_lb(t.box, node, qx, qy, qz) >= r2)) visit(l);
        }
        while (node & 1u) node >>= 1;
        if (node == 0) break;
        ++node;
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
    return v;
}

// first c in [0, n) with off[c + 1] > x (off ascending, off[0] = 0, x < off[n])
template <class T>
__device__ __forceinline__ uint32_t upper_segment(const T* __restrict__ off, uint32_t n, T x)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

} // namespace

// parent: every position its own root, the positions of a clique leaf under the leaf's first one; size 0, lowest index none, cluster none
__global__ void __launch_bounds__(kClusterBlock)
k_cluster_init(const ClusterSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, float r2, int clique_on, uint32_t* __restrict__ parent,
               uint32_t* __restrict__ size, uint32_t* __restrict__ minidx, int32_t* __restrict__ cid)
{
    uint32_t j;
    const ClusterSeg& S = block_record<kClusterBlock>(segs, block_seg, j);
    j += threadIdx.x;
    if (j >= S.t.Mf) return;
    const uint32_t l = j / kSearchLeaf;
    const bool cl = clique_on && leaf_is_clique(S.t.box, S.t.P + l, r2);
    parent[S.fbase + j] = cl ? l * kSearchLeaf : j;
    size[S.fbase + j] = 0u;
    minidx[S.fbase + j] = 0xffffffffu;
    cid[S.fbase + j] = -1;
}

// stats: pairs tested, edges found, leaves visited, clique leaves among them, clique early exits, hook retries
__global__ void __launch_bounds__(kClusterBlock)
k_cluster_hook(const ClusterSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, float r2, int clique_on, uint32_t* __restrict__ parent_all,
               unsigned long long* __restrict__ stats)
{
    uint32_t j;
    const ClusterSeg& S = block_record<kClusterBlock>(segs, block_seg, j);
    j += threadIdx.x;
    const SearchTree t = S.t;
    uint32_t cnt[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (j < t.Mf) {
        uint32_t* parent = parent_all + S.fbase;
        const float4 q = t.pts[j];
        const uint32_t own = j / kSearchLeaf;
        uint32_t rj = j;      // j or an ancestor of j: where the next unite starts
        walk_below(t, S.logP, j, q.x, q.y, q.z, (double)r2, [&](uint32_t l) {
            const uint32_t a = l * kSearchLeaf, b = min(min(a + (uint32_t)kSearchLeaf, t.Mf), j);
            const bool cl = clique_on && leaf_is_clique(t.box, t.P + l, r2);
            ++cnt[2];
            if (cl) { ++cnt[3]; if (l == own) return; }      // the init pass united the thread's own clique leaf
            for (uint32_t p = a; p < b; ++p) {
                const float4 o = t.pts[p];
                ++cnt[0];
                if (sqdist_l2simple(q.x, q.y, q.z, o.x, o.y, o.z) < r2) {
                    ++cnt[1];
                    rj = uf::unite(parent, rj, p, &cnt[5]);
                    if (cl) { ++cnt[4]; break; }
                }
            }
        });
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned long long v = wave_sum64(cnt[k]);
        if ((threadIdx.x & 63u) == 0 && v) atomicAdd(stats + k, v);
    }
}

// root[i] = find(i); size and lowest original index per root (one pair of atomics per wavefront where all its points share a root)
__global__ void __launch_bounds__(kClusterBlock)
k_cluster_flatten(const ClusterSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, const uint32_t* __restrict__ parent, uint32_t* __restrict__ root,
                  uint32_t* __restrict__ size, uint32_t* __restrict__ minidx)
{
    uint32_t j;
    const ClusterSeg& S = block_record<kClusterBlock>(segs, block_seg, j);
    j += threadIdx.x;
    const bool active = j < S.t.Mf;
    uint32_t r = 0xffffffffu, oi = 0xffffffffu;
    if (active) {
        r = uf::find(parent + S.fbase, j);
        root[S.fbase + j] = r;
        oi = S.t.idx[j];
    }
    const uint32_t r0 = (uint32_t)__shfl((int)r, 0, 64);
    if (__all(!active || r == r0)) {
        const uint32_t n = (uint32_t)__popcll(__ballot(active));
        const uint32_t mn = wave_min(oi);
        if ((threadIdx.x & 63u) == 0 && n) { atomicAdd(size + S.fbase + r0, n); atomicMin(minidx + S.fbase + r0, mn); }
    } else if (active) {
        atomicAdd(size + S.fbase + r, 1u);
        atomicMin(minidx + S.fbase + r, oi);
    }
}

// keep[i] = 1 for a root whose component passes the size filter; counts[2 seg] += clusters kept, counts[2 seg + 1] += their points
__global__ void __launch_bounds__(kClusterBlock)
k_cluster_roots(const ClusterSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, const uint32_t* __restrict__ root, const uint32_t* __restrict__ size,
                uint32_t min_size, uint32_t max_size, uint8_t* __restrict__ keep, unsigned long long* __restrict__ counts)
{
    uint32_t j, si;
    const ClusterSeg& S = block_record<kClusterBlock>(segs, block_seg, j, &si);
    j += threadIdx.x;
    uint32_t k = 0, n = 0;
    if (j < S.t.Mf) {
        const uint32_t sz = size[S.fbase + j];
        k = root[S.fbase + j] == j && sz >= min_size && sz <= max_size ? 1u : 0u;
        n = k ? sz : 0u;
        keep[S.fbase + j] = (uint8_t)k;
    }
    k = wave_sum(k);
    const unsigned long long n64 = wave_sum64(n);
    if ((threadIdx.x & 63u) == 0 && k) { atomicAdd(counts + 2 * (size_t)si, (unsigned long long)k); atomicAdd(counts + 2 * (size_t)si + 1, n64); }
}

// the kept roots in position order: key = (~size, lowest original index), value = global position
__global__ void __launch_bounds__(kClusterBlock)
k_cluster_compact(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ pos, size_t n, const uint32_t* __restrict__ size, const uint32_t* __restrict__ minidx,
                  uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    keys[pos[i]] = ((uint64_t)(~size[i]) << 32) | minidx[i];
    vals[pos[i]] = (uint32_t)i;
}

// cluster c of the batch (sorted): its root learns its number; size, lowest index, index of the batch, 256-point chunks
__global__ void __launch_bounds__(kClusterBlock)
k_cluster_assign(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t nc, const uint64_t* __restrict__ coff, uint32_t n_segs,
                 int32_t* __restrict__ cid, uint32_t* __restrict__ csize, int32_t* __restrict__ cfirst, uint32_t* __restrict__ cseg, uint32_t* __restrict__ cchunks)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nc) return;
    if (c == nc) { csize[c] = 0u; cchunks[c] = 0u; return; }      // the scans run over nc + 1 entries
    const uint64_t key = keys[c];
    const uint32_t sz = ~(uint32_t)(key >> 32);
    cid[vals[c]] = (int32_t)c;
    csize[c] = sz;
    cfirst[c] = (int32_t)(uint32_t)key;
    cseg[c] = upper_segment(coff, n_segs, (uint64_t)c);
    cchunks[c] = (sz + kClusterChunk - 1) / kClusterChunk;
}

// labels in original order; every clustered point as (cluster << 32 | original index, global position) in any order (the sort that follows fixes it)
__global__ void __launch_bounds__(kClusterBlock)
k_cluster_labels(const ClusterSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, const uint32_t* __restrict__ root, const int32_t* __restrict__ cid,
                 const uint64_t* __restrict__ coff, int32_t* __restrict__ labels, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ cursor)
{
    uint32_t j, si;
    const ClusterSeg& S = block_record<kClusterBlock>(segs, block_seg, j, &si);
    j += threadIdx.x;
    int32_t c = -1;
    uint32_t oi = 0;
    if (j < S.t.Mf) {
        c = cid[S.fbase + root[S.fbase + j]];
        oi = S.t.idx[j];
        if (c >= 0 && oi < S.n_target) labels[S.tbase + oi] = c - (int32_t)coff[si];
    }
    const unsigned long long m = __ballot(c >= 0);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(cursor, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, 0, 64);
    if (c >= 0) {
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        keys[at] = ((uint64_t)(uint32_t)c << 32) | oi;
        vals[at] = (uint32_t)(S.fbase + j);
    }
}

// one 256-point chunk of one cluster's CSR row: point indices out, box (ordered keys) and coordinate sums (double, tree over the chunk: pairs 128 apart, 64, ... 1)
__global__ void __launch_bounds__(kClusterChunk)
k_cluster_partials(const ClusterSeg* __restrict__ segs, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t nc,
                   const uint32_t* __restrict__ csize, const uint32_t* __restrict__ cseg, const uint32_t* __restrict__ goff, const uint32_t* __restrict__ choff,
                   int32_t* __restrict__ idx_out, double* __restrict__ psum, uint32_t* __restrict__ pbox)
{
    __shared__ double ss[3][kClusterChunk];
    __shared__ uint32_t sb[6][kClusterChunk];
    if (blockIdx.x >= choff[nc]) return;
    const uint32_t c = upper_segment(choff, nc, (uint32_t)blockIdx.x);
    const uint32_t at = (blockIdx.x - choff[c]) * kClusterChunk + threadIdx.x;
    const uint32_t tid = threadIdx.x;
    double x = 0.0, y = 0.0, z = 0.0;
    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    if (at < csize[c]) {
        const uint32_t i = goff[c] + at;
        const ClusterSeg& S = segs[cseg[c]];
        const float4 p = S.t.pts[vals[i] - S.fbase];
        idx_out[i] = (int32_t)(uint32_t)keys[i];
        x = (double)p.x; y = (double)p.y; z = (double)p.z;
        mn[0] = mx[0] = ordered_key(p.x); mn[1] = mx[1] = ordered_key(p.y); mn[2] = mx[2] = ordered_key(p.z);
    }
    ss[0][tid] = x; ss[1][tid] = y; ss[2][tid] = z;
#pragma unroll
    for (int d = 0; d < 3; ++d) { sb[d][tid] = mn[d]; sb[3 + d][tid] = mx[d]; }
    for (uint32_t s = kClusterChunk / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                ss[d][tid] = ss[d][tid] + ss[d][tid + s];
                sb[d][tid] = min(sb[d][tid], sb[d][tid + s]);
                sb[3 + d][tid] = max(sb[3 + d][tid], sb[3 + d][tid + s]);
            }
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) psum[3 * (size_t)blockIdx.x + d] = ss[d][0];
#pragma unroll
        for (int d = 0; d < 6; ++d) pbox[6 * (size_t)blockIdx.x + d] = sb[d][0];
    }
}

// one wavefront per cluster: chunk sums 64 at a time (pairs 32 apart, 16, ... 1), the groups added in order; box; the handle's CSR offsets
__global__ void __launch_bounds__(kClusterBlock)
k_cluster_finish(uint32_t nc, const uint32_t* __restrict__ csize, const int32_t* __restrict__ cfirst, const uint32_t* __restrict__ cseg,
                 const uint32_t* __restrict__ goff, const uint32_t* __restrict__ choff, const uint64_t* __restrict__ coff, const double* __restrict__ psum,
                 const uint32_t* __restrict__ pbox, uint32_t* __restrict__ sizes_out, int32_t* __restrict__ first_out, float* __restrict__ box_out,
                 double* __restrict__ centroid_out, uint64_t* __restrict__ offsets_out)
{
    const uint32_t c = blockIdx.x * (kClusterBlock / 64) + (threadIdx.x >> 6);
    if (c >= nc) return;      // whole wavefronts leave together
    const uint32_t lane = threadIdx.x & 63u;
    double sum[3] = {0.0, 0.0, 0.0};
    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    for (uint32_t g = choff[c]; g < choff[c + 1]; g += 64u) {
        const uint32_t b = g + lane;
        const bool in = b < choff[c + 1];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double v = in ? psum[3 * (size_t)b + d] : 0.0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
            sum[d] = sum[d] + v;
            if (in) { mn[d] = min(mn[d], pbox[6 * (size_t)b + d]); mx[d] = max(mx[d], pbox[6 * (size_t)b + 3 + d]); }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) { mn[d] = wave_min(mn[d]); mx[d] = ~wave_min(~mx[d]); }
    if (lane != 0) return;
    const uint32_t sz = csize[c], si = cseg[c];
    sizes_out[c] = sz;
    first_out[c] = cfirst[c];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        box_out[6 * (size_t)c + d] = ordered_unkey(mn[d]);
        box_out[6 * (size_t)c + 3 + d] = ordered_unkey(mx[d]);
        centroid_out[3 * (size_t)c + d] = sum[d] / (double)sz;
    }
    const uint32_t c0 = (uint32_t)coff[si];
    offsets_out[(size_t)c + si] = (uint64_t)(goff[c] - goff[c0]);
    if ((uint64_t)c + 1 == coff[si + 1]) offsets_out[(size_t)c + 1 + si] = (uint64_t)(goff[c + 1] - goff[c0]);
}

hipError_t cluster_hook(const ClusterSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, float r2, int clique_on, uint32_t* parent, uint32_t* root,
                        uint32_t* size, uint32_t* minidx, int32_t* cid, unsigned long long* stats6, hipStream_t s)
{
    if (!n_blocks) return hipSuccess;
    k_cluster_init<<<dim3(n_blocks), dim3(kClusterBlock), 0, s>>>(segs, block_seg, r2, clique_on, parent, size, minidx, cid);
    k_cluster_hook<<<dim3(n_blocks), dim3(kClusterBlock), 0, s>>>(segs, block_seg, r2, clique_on, parent, stats6);
    k_cluster_flatten<<<dim3(n_blocks), dim3(kClusterBlock), 0, s>>>(segs, block_seg, parent, root, size, minidx);
    return hipGetLastError();
}

hipError_t cluster_roots(const ClusterSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, const uint32_t* root, const uint32_t* size, uint32_t min_size,
                         uint32_t max_size, uint8_t* keep, unsigned long long* counts, hipStream_t s)
{
    if (!n_blocks) return hipSuccess;
    k_cluster_roots<<<dim3(n_blocks), dim3(kClusterBlock), 0, s>>>(segs, block_seg, root, size, min_size, max_size, keep, counts);
    return hipGetLastError();
}

size_t cluster_temp_bytes(size_t n_clusters, size_t n_segs)
{
    size_t b = 0;
    (void)rocprim::exclusive_scan(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n_clusters + 1, rocprim::plus<uint32_t>());
    return std::max(seg_sort_pairs_temp_bytes(n_clusters, n_segs), b);
}

hipError_t cluster_number(const uint8_t* keep, const uint32_t* pos, size_t total, const uint32_t* size, const uint32_t* minidx, uint32_t n_clusters,
                          const uint64_t* coff, uint32_t n_segs, uint64_t* keys, uint64_t* keys_sorted, uint32_t* vals, uint32_t* vals_sorted, int32_t* cid,
                          uint32_t* csize, int32_t* cfirst, uint32_t* cseg, uint32_t* cchunks, uint32_t* goff, uint32_t* choff, void* temp, size_t temp_bytes,
                          hipStream_t s)
{
    if (!n_clusters) return hipSuccess;
    k_cluster_compact<<<dim3(grid_for(total)), dim3(kClusterBlock), 0, s>>>(keep, pos, total, size, minidx, keys, vals);
    hipError_t e = seg_sort_pairs_u64(keys, keys_sorted, vals, vals_sorted, n_clusters, n_segs, coff, temp, temp_bytes, s);
    if (e != hipSuccess) return e;
    k_cluster_assign<<<dim3(grid_for((size_t)n_clusters + 1)), dim3(kClusterBlock), 0, s>>>(keys_sorted, vals_sorted, n_clusters, coff, n_segs, cid, csize, cfirst, cseg,
                                                                                             cchunks);
    e = rocprim::exclusive_scan(temp, temp_bytes, csize, goff, 0u, (size_t)n_clusters + 1, rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(temp, temp_bytes, cchunks, choff, 0u, (size_t)n_clusters + 1, rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t cluster_labels(const ClusterSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, const uint32_t* root, const int32_t* cid, const uint64_t* coff,
                          int32_t* labels, uint64_t* keys, uint32_t* vals, uint32_t* cursor, hipStream_t s)
{
    if (!n_blocks) return hipSuccess;
    hipError_t e = hipMemsetAsync(cursor, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    k_cluster_labels<<<dim3(n_blocks), dim3(kClusterBlock), 0, s>>>(segs, block_seg, root, cid, coff, labels, keys, vals, cursor);
    return hipGetLastError();
}

hipError_t cluster_finish(const ClusterSeg* segs, const uint64_t* keys_sorted, const uint32_t* vals_sorted, uint32_t n_clusters, size_t n_points, const uint32_t* csize,
                          const int32_t* cfirst, const uint32_t* cseg, const uint32_t* goff, const uint32_t* choff, const uint64_t* coff, double* psum, uint32_t* pbox,
                          int32_t* idx_out, uint32_t* sizes_out, int32_t* first_out, float* box_out, double* centroid_out, uint64_t* offsets_out, hipStream_t s)
{
    if (!n_clusters) return hipSuccess;
    const size_t max_chunks = cluster_max_chunks(n_clusters, n_points);
    k_cluster_partials<<<dim3((unsigned)max_chunks), dim3(kClusterChunk), 0, s>>>(segs, keys_sorted, vals_sorted, n_clusters, csize, cseg, goff, choff, idx_out, psum,
                                                                                 pbox);
    k_cluster_finish<<<dim3(grid_for(n_clusters, kClusterBlock / 64)), dim3(kClusterBlock), 0, s>>>(n_clusters, csize, cfirst, cseg, goff, choff, coff, psum, pbox,
                                                                                                    sizes_out, first_out, box_out, centroid_out, offsets_out);
    return hipGetLastError();
}

} // namespace ltm
