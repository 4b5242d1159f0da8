// ltm_k_fpfh.hip -- Fast Point Feature Histograms over the targets of search indices: the counterpart of pcl::FPFHEstimation (setKSearch) with the normals
// stored with the index.  The reference does not call it; the arithmetic is stated in include/ltm.h, "fpfh", the bin rules in ltm_fpfh_bins.h.
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
//
// A fixed sequence of launches for the whole batch, every record (one listed index) found through the batch's owner table (ltm_block_table.h) over the
// FINITE points of the records in their index's Morton order:
//   k_fpfh_fill     every descriptor row NaN (what a non-finite position and a point without a normal keep); the SPFH words are zeroed by the caller
//   k_fpfh_spfh     one thread per finite point in Morton order, the kNN seed the point's own stored code (the form of ltm_k_normals.hip): the list holds
//                   (d2, target index, sorted position) in 4 / 8 / 16 registers, or for 17 .. 64 slots in LDS [slot][lane] with one wavefront per
//                   workgroup (48 KB).  After the walk the neighbours' points and normals are gathered by sorted position, the pair features computed in
//                   double and counted: 6-bit fields added by a shift into one 64-bit word per feature (bins 0 .. 9; bin 10 is the pair count less their
//                   sum), so there is no dynamically indexed private array.  Four words per point, at the point's ORIGINAL position.
//   k_fpfh_weight   33 statically indexed double accumulators per point, every neighbour's words unpacked once; the three groups scaled to 100 and rounded to
//                   float.  Two forms with the same bytes: _stored reads the (d2, target index) lists the SPFH pass kept, slot-major, where they fit the
//                   call's scratch budget (kFpfhListBudget) -- no walk; _reg / _lds keep the thread mapping of the SPFH pass and collect the same
//                   neighbourhoods AGAIN, as (d2, target index) only (no n x k buffer).  The wavefront's rows are staged in LDS and written by the whole
//                   wavefront, consecutive lanes to consecutive floats: where the Morton order keeps neighbours of the original order together the rows
//                   leave as contiguous runs of 132 bytes instead of 64 scattered words.
// No floating-point atomics: every value is a function of its index and k alone.
#include "ltm_kernels_common.h"
#include "ltm_search_walk.h"      // pair_less (ltm_knn_list.h), walk, seed_leaves, finite3
#include "ltm_fpfh_bins.h"
namespace ltm {

namespace {

struct D3 { double x, y, z; };
__device__ __forceinline__ double dot3(const D3& a, const D3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross3(const D3& a, const D3& b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// the SPFH of one point while it is counted: bins 0 .. 9 of each feature as 6-bit fields, the pairs counted
struct SpfhWords {
    unsigned long long w[3] = {0ull, 0ull, 0ull};
    uint32_t pairs = 0;
    __device__ __forceinline__ void add(int ba, int bp, int bt)
    {
        w[0] += ba < 10 ? 1ull << (6 * ba) : 0ull;
        w[1] += bp < 10 ? 1ull << (6 * bp) : 0ull;
        w[2] += bt < 10 ? 1ull << (6 * bt) : 0ull;
        ++pairs;
    }
};

// computePairFeatures of (p, q) as include/ltm.h states it; false: the pair is skipped
__device__ __forceinline__ bool fpfh_pair(const float4& p, const D3& np, const float4& q, const float4& nq4, SpfhWords& W)
{
    if (!finite3(nq4.x, nq4.y, nq4.z)) return false;
    const D3 nq{(double)nq4.x, (double)nq4.y, (double)nq4.z};
    D3 d{(double)q.x - (double)p.x, (double)q.y - (double)p.y, (double)q.z - (double)p.z};
    const double f4 = sqrt(dot3(d, d));
    if (f4 == 0.0) return false;
    const double a1 = dot3(np, d) / f4, a2 = dot3(nq, d) / f4;
    const bool swap = fabs(a1) < fabs(a2);
    const D3 u = swap ? nq : np, o = swap ? np : nq;
    if (swap) { d.x = -d.x; d.y = -d.y; d.z = -d.z; }
    const double phi = swap ? -a2 : a1;
    D3 v = cross3(d, u);
    const double vn = sqrt(dot3(v, v));
    if (vn == 0.0) return false;
    v.x = v.x / vn; v.y = v.y / vn; v.z = v.z / vn;
    const D3 w = cross3(u, v);
    const double alpha = dot3(v, o);
    W.add(fpfh_bin_unit(alpha), fpfh_bin_unit(phi), fpfh_bin_theta(dot3(w, o), dot3(u, o)));
    return true;
}

__device__ __forceinline__ void spfh_store(unsigned long long* __restrict__ spfh, uint64_t at, const SpfhWords& W)
{
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(spfh + 4 * at);
    dst[0] = make_ulonglong2(W.w[0], W.w[1]);
    dst[1] = make_ulonglong2(W.w[2], (unsigned long long)W.pairs);
}

// the 33 sums of one point
struct FpfhSums {
    double s[kFpfhSize];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int b = 0; b < kFpfhSize; ++b) s[b] = 0.0;
    }
    // S_b = S_b + (1 / d2) count_q[b] for the neighbour whose words are at spfh + 4 at
    __device__ __forceinline__ void add(const unsigned long long* __restrict__ spfh, uint64_t at, float d2)
    {
        const ulonglong2* src = reinterpret_cast<const ulonglong2*>(spfh + 4 * at);
        const ulonglong2 lo = src[0], hi = src[1];
        const unsigned long long word[3] = {lo.x, lo.y, hi.x};
        const uint32_t pairs = (uint32_t)hi.y;
        const double w = 1.0 / (double)d2;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            uint32_t rest = pairs;
#pragma unroll
            for (int b = 0; b < kFpfhBins - 1; ++b) {
                const uint32_t c = (uint32_t)(word[g] >> (6 * b)) & 63u;
                rest -= c;
                s[g * kFpfhBins + b] = s[g * kFpfhBins + b] + w * (double)c;
            }
            s[g * kFpfhBins + kFpfhBins - 1] = s[g * kFpfhBins + kFpfhBins - 1] + w * (double)rest;
        }
    }
    // every group scaled to sum to 100 (a group whose sum is 0 stays 0), rounded to float, into the lane's row
    __device__ __forceinline__ void finish(float* __restrict__ row) const
    {
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            double T = s[g * kFpfhBins];
#pragma unroll
            for (int b = 1; b < kFpfhBins; ++b) T = T + s[g * kFpfhBins + b];
#pragma unroll
            for (int b = 0; b < kFpfhBins; ++b) row[g * kFpfhBins + b] = T == 0.0 ? 0.0f : (float)(100.0 * s[g * kFpfhBins + b] / T);
        }
    }
};

// The rows of a workgroup staged in `rows` (BLOCK x 33 floats, the row of thread t from 33 t) leave for desc: every wavefront writes its own 64 rows,
// consecutive lanes to consecutive floats.  row_at[t]: the row's position among the call's rows, ~0 for none.  Reached by every thread of the workgroup
template <int BLOCK>
__device__ __forceinline__ void store_rows(const float* rows, const uint64_t* row_at, float* __restrict__ desc)
{
    __syncthreads();
    const uint32_t wave0 = threadIdx.x & ~63u, lane = threadIdx.x & 63u;
    for (uint32_t i = lane; i < 64u * kFpfhSize; i += 64u) {
        const uint32_t r = i / kFpfhSize, b = i - r * kFpfhSize;
        const uint64_t at = row_at[wave0 + r];
        if (at != ~0ull) desc[at * kFpfhSize + b] = rows[wave0 * kFpfhSize + i];
    }
}

} // namespace

__global__ void __launch_bounds__(kFpfhBlock)
k_fpfh_fill(uint64_t n_floats, float* __restrict__ desc)
{
    const uint64_t i = (uint64_t)blockIdx.x * kFpfhBlock + threadIdx.x;
    if (i < n_floats) desc[i] = __builtin_nanf("");
}

// ------------------------------------------------------------------------------------------------------------------------ pass 1: SPFH
// KT in {4, 8, 16}: the list in registers, the insertion network of KnnListReg (ltm_knn_list.h) written out as in ltm_k_normals.hip
template <int KT>
__global__ void __launch_bounds__(kFpfhBlock)
k_fpfh_spfh_reg(const FpfhSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, int k, unsigned long long* __restrict__ spfh,
                float* __restrict__ list_d2, int* __restrict__ list_idx, uint64_t total_f, unsigned long long* __restrict__ stats)
{
    uint32_t j0;
    const FpfhSeg& S = block_record<kFpfhBlock>(segs, block_seg, j0);
    j0 += threadIdx.x;
    const SearchTree t = S.t;
    const bool active = j0 < t.Mf;
    uint32_t evals = 0, skipped = 0;
    if (active) {
        const float4 n4 = S.nrm[j0];
        if (finite3(n4.x, n4.y, n4.z)) {      // a point without a normal keeps its zeros
            const int kk = (int)min((uint32_t)k, t.Mf);
            const float4 qp = t.pts[j0];
            const int self = (int)t.idx[j0];
            float bd[KT];
            int bi[KT];
            uint32_t bj[KT];
#pragma unroll
            for (int j = 0; j < KT; ++j) { const bool sent = j < KT - kk; bd[j] = sent ? -1.0f : __builtin_inff(); bi[j] = sent ? -1 : INT_MAX; bj[j] = 0u; }
            auto push = [&](float d, int i, uint32_t pos) {
                if (!pair_less(d, i, bd[KT - 1], bi[KT - 1])) return;
#pragma unroll
                for (int j = KT - 1; j > 0; --j) {
                    const bool before_prev = pair_less(d, i, bd[j - 1], bi[j - 1]);
                    const bool before_this = pair_less(d, i, bd[j], bi[j]);
                    const float nd = before_prev ? bd[j - 1] : (before_this ? d : bd[j]);
                    const int ni = before_prev ? bi[j - 1] : (before_this ? i : bi[j]);
                    const uint32_t nj = before_prev ? bj[j - 1] : (before_this ? pos : bj[j]);
                    bd[j] = nd; bi[j] = ni; bj[j] = nj;
                }
                if (pair_less(d, i, bd[0], bi[0])) { bd[0] = d; bi[0] = i; bj[0] = pos; }
            };
            auto visit = [&](uint32_t l) {
                const uint32_t a = l * kSearchLeaf, b = min(a + (uint32_t)kSearchLeaf, t.Mf);
                evals += b - a;
                for (uint32_t j = a; j < b; ++j) {
                    const float4 p = t.pts[j];
                    push(sqdist_l2simple(qp.x, qp.y, qp.z, p.x, p.y, p.z), (int)t.idx[j], j);
                }
            };
            uint32_t sa, sb;
            seed_leaves(t, t.keys[j0], (uint32_t)kk, sa, sb);
            for (uint32_t l = sa; l <= sb; ++l) visit(l);
            walk(t, qp.x, qp.y, qp.z, sa, sb, [&](double lb) { return lb > (double)bd[KT - 1]; }, visit);
            if (list_d2) {      // the list for the weights, slot-major: a wavefront writes 64 consecutive entries per slot (first, so that the distances need not stay live)
                const uint64_t g = S.fbase + j0;
#pragma unroll
                for (int j = 0; j < KT; ++j)
                    if (j >= KT - kk) { list_d2[(uint64_t)(j - (KT - kk)) * total_f + g] = bd[j]; list_idx[(uint64_t)(j - (KT - kk)) * total_f + g] = bi[j]; }
            }
            const D3 np{(double)n4.x, (double)n4.y, (double)n4.z};
            SpfhWords W;
#pragma unroll
            for (int j = 0; j < KT; ++j)
                if (j >= KT - kk && bi[j] != self && !fpfh_pair(qp, np, t.pts[bj[j]], S.nrm[bj[j]], W)) ++skipped;
            spfh_store(spfh, S.tbase + (uint32_t)self, W);
        }
    }
    count_up(stats, 0, active ? 1u : 0u);
    count_up(stats, 1, evals);
    count_up(stats, 2, skipped);
}

// 17 .. 64 slots: the lists in LDS, [slot][lane], one wavefront per workgroup (64 x 64 x 12 B = 48 KB)
__global__ void __launch_bounds__(kFpfhBlockLds)
k_fpfh_spfh_lds(const FpfhSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, int k, unsigned long long* __restrict__ spfh,
                float* __restrict__ list_d2, int* __restrict__ list_idx, uint64_t total_f, unsigned long long* __restrict__ stats)
{
    __shared__ float sd[kFpfhMaxK][kFpfhBlockLds];
    __shared__ int si[kFpfhMaxK][kFpfhBlockLds];
    __shared__ uint32_t sj[kFpfhMaxK][kFpfhBlockLds];
    uint32_t j0;
    const FpfhSeg& S = block_record<kFpfhBlockLds>(segs, block_seg, j0);
    j0 += threadIdx.x;
    const SearchTree t = S.t;
    const int lane = (int)threadIdx.x;
    const bool active = j0 < t.Mf;
    uint32_t evals = 0, skipped = 0;
    if (active) {
        const float4 n4 = S.nrm[j0];
        if (finite3(n4.x, n4.y, n4.z)) {
            const int kk = (int)min((uint32_t)min(k, kFpfhMaxK), t.Mf);
            const float4 qp = t.pts[j0];
            const int self = (int)t.idx[j0];
            int cnt = 0;
            float kth = __builtin_inff();
            auto push = [&](float d, int i, uint32_t pos) {
                int j;
                if (cnt < kk) j = cnt++;
                else if (pair_less(d, i, sd[kk - 1][lane], si[kk - 1][lane])) j = kk - 1;
                else return;
                while (j > 0 && pair_less(d, i, sd[j - 1][lane], si[j - 1][lane])) {
                    sd[j][lane] = sd[j - 1][lane]; si[j][lane] = si[j - 1][lane]; sj[j][lane] = sj[j - 1][lane];
                    --j;
                }
                sd[j][lane] = d; si[j][lane] = i; sj[j][lane] = pos;
                if (cnt == kk) kth = sd[kk - 1][lane];
            };
            auto visit = [&](uint32_t l) {
                const uint32_t a = l * kSearchLeaf, b = min(a + (uint32_t)kSearchLeaf, t.Mf);
                evals += b - a;
                for (uint32_t j = a; j < b; ++j) {
                    const float4 p = t.pts[j];
                    push(sqdist_l2simple(qp.x, qp.y, qp.z, p.x, p.y, p.z), (int)t.idx[j], j);
                }
            };
            uint32_t sa, sb;
            seed_leaves(t, t.keys[j0], (uint32_t)kk, sa, sb);
            for (uint32_t l = sa; l <= sb; ++l) visit(l);
            walk(t, qp.x, qp.y, qp.z, sa, sb, [&](double lb) { return lb > (double)kth; }, visit);
            const D3 np{(double)n4.x, (double)n4.y, (double)n4.z};
            SpfhWords W;
            for (int j = 0; j < cnt; ++j) {      // cnt == kk: the index holds at least kk points
                const uint32_t pos = sj[j][lane];
                if (si[j][lane] != self && !fpfh_pair(qp, np, t.pts[pos], S.nrm[pos], W)) ++skipped;
            }
            spfh_store(spfh, S.tbase + (uint32_t)self, W);
            if (list_d2) {
                const uint64_t g = S.fbase + j0;
                for (int j = 0; j < cnt; ++j) { list_d2[(uint64_t)j * total_f + g] = sd[j][lane]; list_idx[(uint64_t)j * total_f + g] = si[j][lane]; }
            }
        }
    }
    count_up(stats, 0, active ? 1u : 0u);
    count_up(stats, 1, evals);
    count_up(stats, 2, skipped);
    count_up(stats, 3, active ? 1u : 0u);
}

// ---------------------------------------------------------------------------------------------------------------------- pass 2: weights
template <int KT>
__global__ void __launch_bounds__(kFpfhBlock)
k_fpfh_weight_reg(const FpfhSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, int k, const unsigned long long* __restrict__ spfh,
                  float* __restrict__ desc, unsigned long long* __restrict__ stats)
{
    __shared__ float rows[kFpfhBlock * kFpfhSize];      // 33 KB; a lane's row at stride 33: no bank conflict
    __shared__ uint64_t row_at[kFpfhBlock];
    uint32_t j0;
    const FpfhSeg& S = block_record<kFpfhBlock>(segs, block_seg, j0);
    j0 += threadIdx.x;
    const SearchTree t = S.t;
    uint32_t evals = 0;
    uint64_t at = ~0ull;
    if (j0 < t.Mf) {
        const float4 n4 = S.nrm[j0];
        if (finite3(n4.x, n4.y, n4.z)) {      // a point without a normal keeps its NaN row
            const int kk = (int)min((uint32_t)k, t.Mf);
            const float4 qp = t.pts[j0];
            float bd[KT];
            int bi[KT];
#pragma unroll
            for (int j = 0; j < KT; ++j) { const bool sent = j < KT - kk; bd[j] = sent ? -1.0f : __builtin_inff(); bi[j] = sent ? -1 : INT_MAX; }
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
                evals += b - a;
                for (uint32_t j = a; j < b; ++j) {
                    const float4 p = t.pts[j];
                    push(sqdist_l2simple(qp.x, qp.y, qp.z, p.x, p.y, p.z), (int)t.idx[j]);
                }
            };
            uint32_t sa, sb;
            seed_leaves(t, t.keys[j0], (uint32_t)kk, sa, sb);
            for (uint32_t l = sa; l <= sb; ++l) visit(l);
            walk(t, qp.x, qp.y, qp.z, sa, sb, [&](double lb) { return lb > (double)bd[KT - 1]; }, visit);
            FpfhSums F;
            F.clear();
#pragma unroll
            for (int j = 0; j < KT; ++j)
                if (j >= KT - kk && bd[j] != 0.0f) F.add(spfh, S.tbase + (uint32_t)bi[j], bd[j]);
            F.finish(rows + threadIdx.x * kFpfhSize);
            at = S.tbase + t.idx[j0];
        }
    }
    row_at[threadIdx.x] = at;
    store_rows<kFpfhBlock>(rows, row_at, desc);
    count_up(stats, 1, evals);
}

// 17 .. 64 slots: (d2, index) lists in LDS, [slot][lane], one wavefront per workgroup (32 KB); the rows are staged over the lists once they are read
__global__ void __launch_bounds__(kFpfhBlockLds)
k_fpfh_weight_lds(const FpfhSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, int k, const unsigned long long* __restrict__ spfh,
                  float* __restrict__ desc, unsigned long long* __restrict__ stats)
{
    __shared__ uint32_t raw[2 * kFpfhMaxK * kFpfhBlockLds];
    __shared__ uint64_t row_at[kFpfhBlockLds];
    static_assert(kFpfhBlockLds * kFpfhSize <= 2 * kFpfhMaxK * kFpfhBlockLds, "the rows fit over the lists");
    float (*sd)[kFpfhBlockLds] = reinterpret_cast<float (*)[kFpfhBlockLds]>(raw);
    int (*si)[kFpfhBlockLds] = reinterpret_cast<int (*)[kFpfhBlockLds]>(raw + kFpfhMaxK * kFpfhBlockLds);
    float* rows = reinterpret_cast<float*>(raw);
    uint32_t j0;
    const FpfhSeg& S = block_record<kFpfhBlockLds>(segs, block_seg, j0);
    j0 += threadIdx.x;
    const SearchTree t = S.t;
    const int lane = (int)threadIdx.x;
    uint32_t evals = 0;
    uint64_t at = ~0ull;
    FpfhSums F;
    F.clear();
    if (j0 < t.Mf) {
        const float4 n4 = S.nrm[j0];
        if (finite3(n4.x, n4.y, n4.z)) {
            const int kk = (int)min((uint32_t)min(k, kFpfhMaxK), t.Mf);
            const float4 qp = t.pts[j0];
            int cnt = 0;
            float kth = __builtin_inff();
            auto push = [&](float d, int i) {
                int j;
                if (cnt < kk) j = cnt++;
                else if (pair_less(d, i, sd[kk - 1][lane], si[kk - 1][lane])) j = kk - 1;
                else return;
                while (j > 0 && pair_less(d, i, sd[j - 1][lane], si[j - 1][lane])) {
                    sd[j][lane] = sd[j - 1][lane]; si[j][lane] = si[j - 1][lane];
                    --j;
                }
                sd[j][lane] = d; si[j][lane] = i;
                if (cnt == kk) kth = sd[kk - 1][lane];
            };
            auto visit = [&](uint32_t l) {
                const uint32_t a = l * kSearchLeaf, b = min(a + (uint32_t)kSearchLeaf, t.Mf);
                evals += b - a;
                for (uint32_t j = a; j < b; ++j) {
                    const float4 p = t.pts[j];
                    push(sqdist_l2simple(qp.x, qp.y, qp.z, p.x, p.y, p.z), (int)t.idx[j]);
                }
            };
            uint32_t sa, sb;
            seed_leaves(t, t.keys[j0], (uint32_t)kk, sa, sb);
            for (uint32_t l = sa; l <= sb; ++l) visit(l);
            walk(t, qp.x, qp.y, qp.z, sa, sb, [&](double lb) { return lb > (double)kth; }, visit);
            for (int j = 0; j < cnt; ++j) {
                const float d2 = sd[j][lane];
                if (d2 != 0.0f) F.add(spfh, S.tbase + (uint32_t)si[j][lane], d2);
            }
            at = S.tbase + t.idx[j0];
        }
    }
    __syncthreads();      // every lane has read its list: the rows go over it
    if (at != ~0ull) F.finish(rows + lane * kFpfhSize);
    row_at[lane] = at;
    store_rows<kFpfhBlockLds>(rows, row_at, desc);
    count_up(stats, 1, evals);
}

// The weights from the lists the SPFH pass stored: no walk, no list in registers or LDS.  BLOCK is the workgroup of the call's owner table
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
k_fpfh_weight_stored(const FpfhSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, int k, const unsigned long long* __restrict__ spfh,
                     const float* __restrict__ list_d2, const int* __restrict__ list_idx, uint64_t total_f, float* __restrict__ desc)
{
    __shared__ float rows[BLOCK * kFpfhSize];
    __shared__ uint64_t row_at[BLOCK];
    uint32_t j0;
    const FpfhSeg& S = block_record<BLOCK>(segs, block_seg, j0);
    j0 += threadIdx.x;
    const SearchTree t = S.t;
    uint64_t at = ~0ull;
    if (j0 < t.Mf) {
        const float4 n4 = S.nrm[j0];
        if (finite3(n4.x, n4.y, n4.z)) {      // the SPFH pass stored a list for exactly these points
            const int kk = (int)min((uint32_t)min(k, kFpfhMaxK), t.Mf);
            const uint64_t g = S.fbase + j0;
            FpfhSums F;
            F.clear();
            for (int j = 0; j < kk; ++j) {
                const float d2 = list_d2[(uint64_t)j * total_f + g];
                if (d2 != 0.0f) F.add(spfh, S.tbase + (uint32_t)list_idx[(uint64_t)j * total_f + g], d2);
            }
            F.finish(rows + threadIdx.x * kFpfhSize);
            at = S.tbase + t.idx[j0];
        }
    }
    row_at[threadIdx.x] = at;
    store_rows<BLOCK>(rows, row_at, desc);
}

int fpfh_block(int k) { return k > kKnnListRegSlots ? kFpfhBlockLds : kFpfhBlock; }

hipError_t fpfh_estimate(const FpfhSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, uint64_t n_points, int k, unsigned long long* spfh, float* desc,
                         float* list_d2, int* list_idx, uint64_t total_f, unsigned long long* stats4, hipStream_t s)
{
    if (k < 2 || k > kFpfhMaxK) return hipErrorInvalidValue;
    const uint64_t n_floats = n_points * kFpfhSize;
    if (n_floats) k_fpfh_fill<<<dim3(grid_for(n_floats, kFpfhBlock)), dim3(kFpfhBlock), 0, s>>>(n_floats, desc);
    if (n_blocks) {
        knn_list_dispatch<false>(k, [&](auto kt) {
            constexpr int KT = decltype(kt)::value;
            const bool stored = list_d2 && list_idx;
            if constexpr (KT == 0) {
                k_fpfh_spfh_lds<<<dim3(n_blocks), dim3(kFpfhBlockLds), 0, s>>>(segs, block_seg, k, spfh, stored ? list_d2 : nullptr, list_idx, total_f, stats4);
                if (stored) k_fpfh_weight_stored<kFpfhBlockLds><<<dim3(n_blocks), dim3(kFpfhBlockLds), 0, s>>>(segs, block_seg, k, spfh, list_d2, list_idx, total_f, desc);
                else k_fpfh_weight_lds<<<dim3(n_blocks), dim3(kFpfhBlockLds), 0, s>>>(segs, block_seg, k, spfh, desc, stats4);
            } else {
                k_fpfh_spfh_reg<KT><<<dim3(n_blocks), dim3(kFpfhBlock), 0, s>>>(segs, block_seg, k, spfh, stored ? list_d2 : nullptr, list_idx, total_f, stats4);
                if (stored) k_fpfh_weight_stored<kFpfhBlock><<<dim3(n_blocks), dim3(kFpfhBlock), 0, s>>>(segs, block_seg, k, spfh, list_d2, list_idx, total_f, desc);
                else k_fpfh_weight_reg<KT><<<dim3(n_blocks), dim3(kFpfhBlock), 0, s>>>(segs, block_seg, k, spfh, desc, stats4);
            }
        });
    }
    return hipGetLastError();
}

} // namespace ltm
