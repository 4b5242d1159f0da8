// ltm_k_outlier.hip -- statistical and radius outlier removal over the targets of search indices: the counterparts of pcl::StatisticalOutlierRemoval
// (setMeanK, setStddevMulThresh) and pcl::RadiusOutlierRemoval (setRadiusSearch, setMinNeighborsInRadius).  The reference calls neither; the arithmetic is
// stated in include/ltm.h, "outlier filters".
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
//
// A fixed sequence of launches for the whole batch, every record (one listed index) found through the batch's owner tables (ltm_block_table.h): one table
// over the FINITE points of the records in their index's Morton order, one over the 256-position chunks of the records' targets in original order.
//   k_outlier_rows   the records' rows zeroed, the records counted
//   k_sor_distances  one thread per finite point in Morton order: the lanes of a wavefront are neighbours in space and walk the same part of the box tree,
//                    and the kNN seed is the point's own stored code (the form of ltm_k_normals.hip).  The lists hold d2 ONLY -- equal d2 give equal terms
//                    of the sum, so no index breaks a tie -- in 4 / 8 / 16 registers, or for 17 .. 64 slots in LDS [slot][lane], 4 bytes per entry: 16 KB
//                    for the one wavefront of a workgroup.  After the walk: the ascending sum of double square roots past the first slot, one divide, one
//                    rounding to float, one store at the point's ORIGINAL position.
//   k_sor_moments    one workgroup per chunk of 256 original positions: sum d and sum d d in double by a binary tree (the shape of "clusters")
//   k_sor_combine    one wavefront per record: chunk sums 64 at a time by a shuffle tree, groups in order; mean, stddev and threshold into the record's row
//   k_sor_labels     one pass over the finite points: label and, by ballot, one integer atomic per wavefront for n_kept
//   k_ror_count      one thread per finite point: its own leaf first, then the walk with the skip rule of ltm_radius_search / "clusters" (lb >= r2), over
//                    as soon as min_neighbors are counted; count and label at the original position, n_kept as above
// No floating-point atomics: every value is a function of its record and the parameters alone.  Non-finite positions keep the zeros of the preceding fill.
#include "ltm_kernels_common.h"
#include "ltm_search_walk.h"      // walk, seed_leaves, for_leaf_points
namespace ltm {

// d_i from the ascending list: S = sum of sqrt((double)d2) past the first slot, in order; (float)(S / mean_k)
__device__ __forceinline__ double sor_term(float d2) { return sqrt((double)d2); }

// KT in {4, 8, 16} slots of one float, kept ascending by the insertion network of KnnListReg (ltm_knn_list.h) without its index words, written out here like the
// LDS form below (on knn_collect: 1.1 % slower per batch, 4.6 % with one call per index) (sentinels of distance -1 in the
// first KT - kk slots).  A candidate equal to the last slot is not inserted: it would change nothing
template <int KT>
__global__ void __launch_bounds__(kOutlierBlock)
k_sor_distances_reg(const OutlierSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, int mean_k, float* __restrict__ dist,
                    unsigned long long* __restrict__ stats)
{
    uint32_t j0;
    const OutlierSeg& S = block_record<kOutlierBlock>(segs, block_seg, j0);
    j0 += threadIdx.x;
    const SearchTree t = S.t;
    uint32_t evals = 0;
    const bool active = j0 < t.Mf;
    if (active) {
        const int kk = (int)min((uint32_t)mean_k + 1u, t.Mf);
        const float4 qp = t.pts[j0];
        float bd[KT];
#pragma unroll
        for (int j = 0; j < KT; ++j) bd[j] = j < KT - kk ? -1.0f : __builtin_inff();
        auto push = [&](float d) {
            if (!(d < bd[KT - 1])) return;
#pragma unroll
            for (int j = KT - 1; j > 0; --j) {
                const bool before_prev = d < bd[j - 1];
                const bool before_this = d < bd[j];
                bd[j] = before_prev ? bd[j - 1] : (before_this ? d : bd[j]);
            }
            if (d < bd[0]) bd[0] = d;
        };
        auto visit = [&](uint32_t l) {
            const uint32_t a = l * kSearchLeaf, b = min(a + (uint32_t)kSearchLeaf, t.Mf);
            evals += b - a;
            for (uint32_t j = a; j < b; ++j) {
                const float4 p = t.pts[j];
                push(sqdist_l2simple(qp.x, qp.y, qp.z, p.x, p.y, p.z));
            }
        };
        uint32_t sa, sb;
        seed_leaves(t, t.keys[j0], (uint32_t)kk, sa, sb);
        for (uint32_t l = sa; l <= sb; ++l) visit(l);
        walk(t, qp.x, qp.y, qp.z, sa, sb, [&](double lb) { return lb > (double)bd[KT - 1]; }, visit);
        double sum = 0.0;
#pragma unroll
        for (int j = 1; j < KT; ++j)
            if (j > KT - kk) sum = sum + sor_term(bd[j]);
        dist[S.tbase + t.idx[j0]] = (float)(sum / (double)mean_k);
    }
    count_up(stats, 0, active ? 1u : 0u);
    count_up(stats, 1, evals);
}

// 17 .. 64 slots: the lists in LDS, [slot][lane], one wavefront per workgroup (64 x 64 x 4 B = 16 KB) (on knn_collect: 1.4 % slower)
__global__ void __launch_bounds__(kOutlierBlockLds)
k_sor_distances_lds(const OutlierSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, int mean_k, float* __restrict__ dist,
                    unsigned long long* __restrict__ stats)
{
    __shared__ float sd[kOutlierMaxSlots][kOutlierBlockLds];
    uint32_t j0;
    const OutlierSeg& S = block_record<kOutlierBlockLds>(segs, block_seg, j0);
    j0 += threadIdx.x;
    const SearchTree t = S.t;
    const int lane = (int)threadIdx.x;
    uint32_t evals = 0;
    const bool active = j0 < t.Mf;
    if (active) {
        const int kk = (int)min((uint32_t)min(mean_k + 1, kOutlierMaxSlots), t.Mf);
        const float4 qp = t.pts[j0];
        int cnt = 0;
        float kth = __builtin_inff();
        auto push = [&](float d) {
            int j;
            if (cnt < kk) j = cnt++;
            else if (d < kth) j = kk - 1;
            else return;
            while (j > 0 && d < sd[j - 1][lane]) {
                sd[j][lane] = sd[j - 1][lane];
                --j;
            }
            sd[j][lane] = d;
            if (cnt == kk) kth = sd[kk - 1][lane];
        };
        auto visit = [&](uint32_t l) {
            const uint32_t a = l * kSearchLeaf, b = min(a + (uint32_t)kSearchLeaf, t.Mf);
            evals += b - a;
            for (uint32_t j = a; j < b; ++j) {
                const float4 p = t.pts[j];
                push(sqdist_l2simple(qp.x, qp.y, qp.z, p.x, p.y, p.z));
            }
        };
        uint32_t sa, sb;
        seed_leaves(t, t.keys[j0], (uint32_t)kk, sa, sb);
        for (uint32_t l = sa; l <= sb; ++l) visit(l);
        walk(t, qp.x, qp.y, qp.z, sa, sb, [&](double lb) { return lb > (double)kth; }, visit);
        double sum = 0.0;
        for (int j = 1; j < cnt; ++j) sum = sum + sor_term(sd[j][lane]);      // cnt == kk: the index holds at least kk points
        dist[S.tbase + t.idx[j0]] = (float)(sum / (double)mean_k);
    }
    count_up(stats, 0, active ? 1u : 0u);
    count_up(stats, 1, evals);
}

// the records' rows zeroed (an index without a finite point keeps them), and the records counted
__global__ void __launch_bounds__(kOutlierBlock)
k_outlier_rows(uint32_t n_recs, OutlierRec* __restrict__ out, unsigned long long* __restrict__ stats)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_recs) { out[r].mean = 0.0; out[r].stddev = 0.0; out[r].threshold = 0.0; out[r].n_kept = 0u; out[r].pad = 0u; }
    if (r == 0u) atomicAdd(stats + 3, (unsigned long long)n_recs);
}

// partials[2 c], partials[2 c + 1]: sum d and sum d d over chunk c of the batch (256 consecutive original positions of one record, zeros past its end)
__global__ void __launch_bounds__(kOutlierChunk)
k_sor_moments(const OutlierSeg* __restrict__ segs, const uint32_t* __restrict__ chunk_seg, const float* __restrict__ dist, double* __restrict__ partials)
{
    __shared__ double sm[2][kOutlierChunk];
    const OutlierSeg& S = segs[chunk_seg[blockIdx.x]];
    const uint32_t tid = threadIdx.x, i = (blockIdx.x - S.tspan.block0) * (uint32_t)kOutlierChunk + tid;
    const double d = i < S.n_target ? (double)dist[S.tbase + i] : 0.0;
    sm[0][tid] = d;
    sm[1][tid] = d * d;
    for (uint32_t s = kOutlierChunk / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) {
            sm[0][tid] = sm[0][tid] + sm[0][tid + s];
            sm[1][tid] = sm[1][tid] + sm[1][tid + s];
        }
    }
    if (tid == 0) { partials[2 * (size_t)blockIdx.x] = sm[0][0]; partials[2 * (size_t)blockIdx.x + 1] = sm[1][0]; }
}

__global__ void __launch_bounds__(64)
k_sor_combine(const OutlierSeg* __restrict__ segs, double stddev_mul, const double* __restrict__ partials, OutlierRec* __restrict__ out)
{
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint32_t n_chunks = segs[r].tspan.n_blocks, chunk0 = segs[r].tspan.block0;
    double sum = 0.0, sq = 0.0;
    for (uint32_t g = 0; g < n_chunks; g += 64u) {
        const uint32_t b = g + lane;
        const bool in = b < n_chunks;
        double v = in ? partials[2 * (size_t)(chunk0 + b)] : 0.0;
        double w = in ? partials[2 * (size_t)(chunk0 + b) + 1] : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { v = v + __shfl_xor(v, off, 64); w = w + __shfl_xor(w, off, 64); }
        sum = sum + v;
        sq = sq + w;
    }
    if (lane != 0u) return;
    const uint32_t nf = segs[r].t.Mf;
    double mean = 0.0, stddev = 0.0;
    if (nf >= 1u) {
        const double n = (double)nf;
        mean = sum / n;
        if (nf >= 2u) {
            const double var = (sq - (sum * sum) / n) / (n - 1.0);
            stddev = sqrt(var > 0.0 ? var : 0.0);      // a negative rounding residue, or NaN, counts as no spread
        }
    }
    out[r].mean = mean;
    out[r].stddev = stddev;
    out[r].threshold = nf ? mean + stddev_mul * stddev : 0.0;
}

// the table and workgroup size of the distances kernel: BLOCK finite points per workgroup
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
k_sor_labels(const OutlierSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, const float* __restrict__ dist, OutlierRec* out,
             uint8_t* __restrict__ labels)
{
    uint32_t j, r;
    const OutlierSeg& S = block_record<BLOCK>(segs, block_seg, j, &r);
    j += threadIdx.x;
    const double thr = out[r].threshold;
    bool keep = false;
    if (j < S.t.Mf) {
        const uint64_t at = S.tbase + S.t.idx[j];
        keep = (double)dist[at] <= thr;
        labels[at] = keep ? 1 : 0;
    }
    const uint32_t n = ballot_count(keep);
    if (n && (threadIdx.x & 63u) == 0u) atomicAdd(&out[r].n_kept, n);
}

__global__ void __launch_bounds__(kOutlierBlock)
k_ror_count(const OutlierSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, float r2, uint32_t min_neighbors, uint32_t* __restrict__ counts,
            uint8_t* __restrict__ labels, OutlierRec* out, unsigned long long* __restrict__ stats)
{
    uint32_t j0, r;
    const OutlierSeg& S = block_record<kOutlierBlock>(segs, block_seg, j0, &r);
    j0 += threadIdx.x;
    const SearchTree t = S.t;
    const bool active = j0 < t.Mf;
    uint32_t evals = 0, early = 0;
    bool keep = false;
    if (active) {
        const float4 qp = t.pts[j0];
        uint32_t cnt = 0;
        auto visit = [&](uint32_t l) {      // entered with cnt < min_neighbors only: the walk refuses every node once they are reached
            for_leaf_points(t, l, qp.x, qp.y, qp.z, [&](uint32_t, const float4&, float d) {
                ++evals;
                if (d < r2) ++cnt;
                return cnt < min_neighbors;
            });
        };
        const uint32_t own = j0 / kSearchLeaf;
        visit(own);      // the point itself is in it
        walk(t, qp.x, qp.y, qp.z, own, own,
             [&](double lb) {
                 if (cnt >= min_neighbors) { early = 1u; return true; }      // enough: every node from here on is refused
                 return lb >= (double)r2;
             },
             visit);
        keep = cnt == min_neighbors;
        const uint64_t at = S.tbase + t.idx[j0];
        counts[at] = cnt;
        labels[at] = keep ? 1 : 0;
    }
    const uint32_t n = ballot_count(keep);
    if (n && (threadIdx.x & 63u) == 0u) atomicAdd(&out[r].n_kept, n);
    count_up(stats, 0, active ? 1u : 0u);
    count_up(stats, 1, evals);
    count_up(stats, 2, early);
}

int outlier_sor_block(int mean_k) { return mean_k + 1 > kKnnListRegSlots ? kOutlierBlockLds : kOutlierBlock; }

hipError_t outlier_statistical(const OutlierSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, const uint32_t* chunk_seg, uint32_t n_chunks, uint32_t n_recs,
                               int mean_k, double stddev_mul, float* dist, double* partials, OutlierRec* out, uint8_t* labels, unsigned long long* stats4,
                               hipStream_t s)
{
    if (!n_recs) return hipSuccess;
    if (mean_k < 1 || mean_k > kOutlierMaxSlots - 1) return hipErrorInvalidValue;
    const int slots = mean_k + 1;
    k_outlier_rows<<<dim3(grid_for(n_recs, kOutlierBlock)), dim3(kOutlierBlock), 0, s>>>(n_recs, out, stats4);
    if (n_blocks) {
        knn_list_dispatch<false>(slots, [&](auto kt) {
            constexpr int KT = decltype(kt)::value;
            if constexpr (KT == 0) k_sor_distances_lds<<<dim3(n_blocks), dim3(kOutlierBlockLds), 0, s>>>(segs, block_seg, mean_k, dist, stats4);
            else k_sor_distances_reg<KT><<<dim3(n_blocks), dim3(kOutlierBlock), 0, s>>>(segs, block_seg, mean_k, dist, stats4);
        });
    }
    if (n_chunks) k_sor_moments<<<dim3(n_chunks), dim3(kOutlierChunk), 0, s>>>(segs, chunk_seg, dist, partials);
    k_sor_combine<<<dim3(n_recs), dim3(64), 0, s>>>(segs, stddev_mul, partials, out);
    if (n_blocks) {
        if (slots > kKnnListRegSlots) k_sor_labels<kOutlierBlockLds><<<dim3(n_blocks), dim3(kOutlierBlockLds), 0, s>>>(segs, block_seg, dist, out, labels);
        else k_sor_labels<kOutlierBlock><<<dim3(n_blocks), dim3(kOutlierBlock), 0, s>>>(segs, block_seg, dist, out, labels);
    }
    return hipGetLastError();
}

hipError_t outlier_radius(const OutlierSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, uint32_t n_recs, float r2, uint32_t min_neighbors,
                          uint32_t* counts, OutlierRec* out, uint8_t* labels, unsigned long long* stats4, hipStream_t s)
{
    if (!n_recs) return hipSuccess;
    if (min_neighbors < 1u) return hipErrorInvalidValue;
    k_outlier_rows<<<dim3(grid_for(n_recs, kOutlierBlock)), dim3(kOutlierBlock), 0, s>>>(n_recs, out, stats4);
    if (n_blocks) k_ror_count<<<dim3(n_blocks), dim3(kOutlierBlock), 0, s>>>(segs, block_seg, r2, min_neighbors, counts, labels, out, stats4);
    return hipGetLastError();
}

} // namespace ltm
