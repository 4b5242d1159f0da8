// ltm_k_sac.hip -- from descriptors to an initial alignment: feature-space correspondences between records of 33-float descriptor rows, and the sample
// consensus over them, the counterparts of pcl::SampleConsensusPrerejective's FLANN search and of its computeTransformation.  The reference calls neither;
// the arithmetic is stated in include/ltm.h, "fpfh matches" and "initial alignment".
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
//
// Matches, one launch for the whole batch, every pair found through the batch's owner table (ltm_block_table.h):
//   k_fpfh_match<KT>   source rows x target rows x 33.  A thread keeps ONE source row in 33 registers and its list in KnnListReg<KT> (ltm_knn_list.h); a
//                      workgroup of kMatchBlock source rows of one pair walks the pair's target rows in tiles of kMatchTileRows staged in LDS with a row
//                      stride of 33 words.  In the distance loop every lane reads the SAME target word: the read is a broadcast, free of bank conflicts
//                      whatever the stride; the odd stride is for the flag pass, where lane r reads row r.  A target row with a NaN component is skipped
//                      by a uniform branch on a per-row flag staged with the tile.
// The distance is a float sum in bin order without fused multiply-add: that order is the statement, so no MFMA, whose accumulation
// order is its own (DESIGN.md 4.4 on Scan Context).
// Alignment, a fixed sequence of launches for the whole batch:
//   k_sac_rows         original position -> sorted position of every index of the call (the hypotheses draw ROWS, the trees hold sorted finite points)
//   k_sac_hypotheses   one thread per (pair, hypothesis): the draws, the coincidence tests, the prerejection and the transform from the two frames; the valid
//                      byte and 12 doubles
//   k_sac_vote         hypotheses x voting points.  A workgroup keeps kSacBlockPoints voting points of ONE pair in registers, read in place from the source
//                      index, and loops over the pair's hypotheses.  The hypothesis is wave-uniform: its row comes through scalar loads, an invalid one is
//                      skipped by a uniform branch.  Each inlier test is the stackless walk of ltm_search_walk.h asking whether a target point EXISTS within
//                      the bound: boxes beyond it are skipped and the first hit ends the walk.  The wave's count is the popcount of the ballot; one global
//                      integer atomic per wave and hypothesis with a non-zero count.
//   k_sac_best         one wavefront per pair: arg-max by (count descending, h ascending), the record
// No floating-point atomics: every double is a function of its pair alone.
#include "ltm_kernels_common.h"
#include "ltm_search_walk.h"
namespace ltm {

namespace {

__device__ __forceinline__ bool is_nan_f(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

} // namespace

template <int KT>
__global__ void __launch_bounds__(kMatchBlock)
k_fpfh_match(const MatchPair* __restrict__ pairs, const uint32_t* __restrict__ block_pair, int kc, int32_t* __restrict__ out_idx, float* __restrict__ out_dist)
{
    __shared__ float tile[kMatchTileRows * kMatchRow];
    __shared__ uint32_t skip[kMatchTileRows];
    uint32_t first;
    const MatchPair& P = block_record<kMatchBlock>(pairs, block_pair, first);
    const uint32_t tid = threadIdx.x, ns = P.n_source, nt = P.n_target;
    const uint32_t row = first + tid;
    const bool live = row < ns;
    float s[kMatchRow];
    bool eligible = live;
#pragma unroll
    for (int b = 0; b < kMatchRow; ++b) {
        s[b] = live ? P.src[(size_t)row * kMatchRow + b] : 0.0f;
        eligible = eligible && !is_nan_f(s[b]);
    }
    KnnListReg<KT> list;
    list.init(kc);
    for (uint32_t t0 = 0; t0 < nt; t0 += kMatchTileRows) {
        const uint32_t rows = min((uint32_t)kMatchTileRows, nt - t0);      // uniform
        __syncthreads();      // the tile before this one has been read
        const float* __restrict__ g = P.tgt + (size_t)t0 * kMatchRow;
        for (uint32_t w = tid; w < rows * kMatchRow; w += kMatchBlock) tile[w] = g[w];
        __syncthreads();
        if (tid < rows) {
            bool nan = false;
#pragma unroll
            for (int b = 0; b < kMatchRow; ++b) nan = nan || is_nan_f(tile[tid * kMatchRow + b]);
            skip[tid] = nan ? 1u : 0u;
        }
        __syncthreads();
        for (uint32_t r = 0; r < rows; ++r) {
            if (__builtin_amdgcn_readfirstlane(skip[r])) continue;      // uniform: a branch, not a mask
            const float* __restrict__ t = tile + r * kMatchRow;
            float acc = 0.0f;
#pragma unroll
            for (int b = 0; b < kMatchRow; ++b) { const float e = s[b] - t[b]; acc = acc + e * e; }
            if (eligible) list.push(acc, (int)(t0 + r), 0u);      // a NaN sum (infinite components) is before nothing and is not listed
        }
    }
    if (!live) return;
    int32_t* oi = out_idx + (P.obase + row) * (size_t)kc;
    float* od = out_dist + (P.obase + row) * (size_t)kc;
    list.for_each([&](int rank, float d, int i, uint32_t) {
        const bool filled = i != INT_MAX;
        oi[rank] = filled ? i : -1;
        od[rank] = filled ? d : __builtin_inff();
    });
}

hipError_t fpfh_match(const MatchPair* pairs, const uint32_t* block_pair, uint32_t n_blocks, int kc, int32_t* idx, float* dist, hipStream_t s)
{
    if (kc < 1 || kc > kMatchMaxK) return hipErrorInvalidValue;
    if (!n_blocks) return hipSuccess;
    knn_list_dispatch<false>(kc, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if constexpr (KT != 0) k_fpfh_match<KT><<<dim3(n_blocks), dim3(kMatchBlock), 0, s>>>(pairs, block_pair, kc, idx, dist);
    });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------- initial alignment
namespace {

// the 32-bit hash behind the draws (include/ltm.h, "initial alignment"): the mix of "planes" over seed + 0x9E3779B9 (6 h + j + 1)
__device__ __forceinline__ uint32_t sac_mix(uint32_t seed, uint32_t h, uint32_t j)
{
    uint32_t x = seed + 0x9E3779B9u * (6u * h + j + 1u);
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ bool finite_d(double v) { return (((uint64_t)__double_as_longlong(v) >> 52) & 0x7ffull) != 0x7ffull; }
__device__ __forceinline__ double sqlen3(const double* a, const double* b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}
// the frame (e1, e2, e3 as rows of f) and centroid of a triangle; false where a squared length is 0 or not finite
__device__ bool sac_frame(const double a[3][3], double f[3][3], double c[3])
{
    double u[3], w[3];
    for (int d = 0; d < 3; ++d) { u[d] = a[1][d] - a[0][d]; w[d] = a[2][d] - a[0][d]; }
    const double uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (!(uu > 0.0) || !(nn > 0.0) || !finite_d(uu) || !finite_d(nn)) return false;
    const double lu = sqrt(uu), ln = sqrt(nn);
    for (int d = 0; d < 3; ++d) { f[0][d] = u[d] / lu; f[2][d] = n[d] / ln; }
    f[1][0] = f[2][1] * f[0][2] - f[2][2] * f[0][1];
    f[1][1] = f[2][2] * f[0][0] - f[2][0] * f[0][2];
    f[1][2] = f[2][0] * f[0][1] - f[2][1] * f[0][0];
    for (int d = 0; d < 3; ++d) c[d] = ((a[0][d] + a[1][d]) + a[2][d]) / 3.0;
    return true;
}

// is there a target point whose float distance to q is within r2?  The walk skips a box whose bound is above r2 and everything once a point was found:
// the hit is kept in the bound itself, the way the kNN walkers keep their k-th distance
__device__ __forceinline__ bool sac_point_within(const SearchTree& t, float qx, float qy, float qz, double r2)
{
    double bound = r2;      // the walk's skip rule starts at the inlier bound; a hit drops it below every box, which ends the walk
    walk(t, qx, qy, qz, 1u, 0u, [&](double lb) { return lb > bound; },
         [&](uint32_t l) {
             for_leaf_points(t, l, qx, qy, qz, [&](uint32_t, const float4&, float d) {
                 if ((double)d <= r2) bound = -1.0;
                 return bound >= 0.0;
             });
         });
    return bound < 0.0;
}

} // namespace

__global__ void __launch_bounds__(kSacBlock)
k_sac_rows(const SacRows* __restrict__ rows, const uint32_t* __restrict__ block_rows, uint32_t* __restrict__ row)
{
    uint32_t first;
    const SacRows& R = block_record<kSacBlock>(rows, block_rows, first);
    const uint32_t j = first + threadIdx.x;
    if (j < R.Mf) row[R.base + R.idx[j]] = j;
}

__global__ void __launch_bounds__(kSacBlock)
k_sac_hypotheses(const SacPair* __restrict__ pairs, SacLaunch L, uint32_t blocks_per_pair, SacHyp* __restrict__ hyp, uint8_t* __restrict__ valid,
                 SacOut* __restrict__ out)
{
    const uint32_t r = blockIdx.x / blocks_per_pair;
    const uint32_t h = (blockIdx.x - r * blocks_per_pair) * kSacBlock + threadIdx.x;
    const bool live = h < L.max_iterations;
    const SacPair& P = pairs[r];
    const uint32_t n = P.n_rows;
    SacHyp H;
#pragma unroll
    for (int d = 0; d < 12; ++d) H.T[d] = 0.0;
    bool ok = false, prerejected = false;
    if (live && n >= 3u) {
        uint32_t s[3], ps[3] = {0u, 0u, 0u}, pt[3] = {0u, 0u, 0u};
        int32_t m[3] = {0, 0, 0};
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) s[j] = (uint32_t)(((uint64_t)sac_mix(L.seed, h, j) * (uint64_t)n) >> 32);
        ok = s[0] != s[1] && s[0] != s[2] && s[1] != s[2];
        if (ok) {
#pragma unroll
            for (uint32_t j = 0; j < 3; ++j) {
                ps[j] = P.srow[s[j]];
                const int32_t* list = P.match + (size_t)s[j] * (size_t)L.kc;
                uint32_t kk = 0;
                for (int q = 0; q < L.kc; ++q) kk += list[q] >= 0 ? 1u : 0u;      // the filled slots come first
                ok = ok && ps[j] != 0xffffffffu && kk != 0u;
                if (kk) m[j] = list[(uint32_t)(((uint64_t)sac_mix(L.seed, h, 3u + j) * (uint64_t)kk) >> 32)];
            }
        }
        ok = ok && m[0] != m[1] && m[0] != m[2] && m[1] != m[2];
        if (ok) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { pt[j] = P.trow[m[j]]; ok = ok && pt[j] != 0xffffffffu; }
        }
        if (ok) {
            double a[3][3], b[3][3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float4 p = P.st.pts[ps[j]], q = P.tt.pts[pt[j]];
                a[j][0] = (double)p.x; a[j][1] = (double)p.y; a[j][2] = (double)p.z;
                b[j][0] = (double)q.x; b[j][1] = (double)q.y; b[j][2] = (double)q.z;
            }
#pragma unroll
            for (int e = 0; e < 3; ++e) {      // edges (0,1), (1,2), (2,0)
                const int e1 = (e + 1) % 3;
                const double ls = sqlen3(a[e], a[e1]), lt = sqlen3(b[e], b[e1]);
                const double lo = ls < lt ? ls : lt, hi = ls < lt ? lt : ls;
                if (!(lo >= L.thr2 * hi)) prerejected = true;
            }
            ok = !prerejected;
            if (ok) {
                double f[3][3], g[3][3], cs[3], ct[3];
                ok = sac_frame(a, f, cs) && sac_frame(b, g, ct);
                if (ok) {
#pragma unroll
                    for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
                        for (int cc = 0; cc < 3; ++cc) H.T[4 * rr + cc] = (g[0][rr] * f[0][cc] + g[1][rr] * f[1][cc]) + g[2][rr] * f[2][cc];
                        H.T[4 * rr + 3] = ct[rr] - ((H.T[4 * rr] * cs[0] + H.T[4 * rr + 1] * cs[1]) + H.T[4 * rr + 2] * cs[2]);
                    }
                }
            }
        }
    }
    if (live) {
        const size_t at = (size_t)r * L.max_iterations + h;
        hyp[at] = H;
        valid[at] = ok ? 1 : 0;
    }
    const uint32_t nv = ballot_count(ok), np = ballot_count(prerejected);
    if ((threadIdx.x & 63u) == 0u) {
        if (nv) atomicAdd(&out[r].n_valid, nv);
        if (np) atomicAdd(&out[r].n_prerejected, np);
    }
}

__global__ void __launch_bounds__(kSacBlock)
k_sac_vote(const SacPair* __restrict__ pairs, const uint32_t* __restrict__ block_pair, const SacHyp* __restrict__ hyp, const uint8_t* __restrict__ valid,
           SacLaunch L, uint32_t* __restrict__ counts, const SacOut* __restrict__ out, unsigned long long* __restrict__ stats)
{
    uint32_t first, r;
    const SacPair& P = block_record<kSacBlockPoints>(pairs, block_pair, first, &r);
    const uint32_t tid = threadIdx.x, H = L.max_iterations;
    float px[kSacPointsPerThread], py[kSacPointsPerThread], pz[kSacPointsPerThread];
    bool has[kSacPointsPerThread];
    uint32_t n_pts = 0;
#pragma unroll
    for (int k = 0; k < kSacPointsPerThread; ++k) {
        const uint32_t j = first + (uint32_t)k * kSacBlock + tid;
        has[k] = j < P.n_eval;
        px[k] = py[k] = pz[k] = 0.0f;
        if (has[k]) {
            const float4 p = P.st.pts[(size_t)j * L.stride];      // (n_eval - 1) stride < Mf
            px[k] = p.x; py[k] = p.y; pz[k] = p.z;
        }
        n_pts += ballot_count(has[k]);
    }
    if (!P.tt.Mf) return;      // uniform: no target point, no inlier
    const SacHyp* __restrict__ Hr = hyp + (size_t)r * H;
    const uint8_t* __restrict__ Vr = valid + (size_t)r * H;
    unsigned long long hits = 0;
    for (uint32_t h = 0; h < H; ++h) {
        if (!Vr[h]) continue;      // uniform
        const double T00 = Hr[h].T[0], T01 = Hr[h].T[1], T02 = Hr[h].T[2], T03 = Hr[h].T[3], T10 = Hr[h].T[4], T11 = Hr[h].T[5], T12 = Hr[h].T[6],
                     T13 = Hr[h].T[7], T20 = Hr[h].T[8], T21 = Hr[h].T[9], T22 = Hr[h].T[10], T23 = Hr[h].T[11];
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < kSacPointsPerThread; ++k) {
            bool in = false;
            if (has[k]) {
                const double x = (double)px[k], y = (double)py[k], z = (double)pz[k];
                const float qx = (float)(((T00 * x + T01 * y) + T02 * z) + T03);
                const float qy = (float)(((T10 * x + T11 * y) + T12 * z) + T13);
                const float qz = (float)(((T20 * x + T21 * y) + T22 * z) + T23);
                if (finite3(qx, qy, qz)) in = sac_point_within(P.tt, qx, qy, qz, L.r2);
            }
            c += ballot_count(in);
        }
        if (c && (tid & 63u) == 0u) { atomicAdd(&counts[(size_t)r * H + h], c); hits += c; }
    }
    if ((tid & 63u) == 0u) {
        if (n_pts) atomicAdd(&stats[0], (unsigned long long)n_pts * (unsigned long long)out[r].n_valid);
        if (hits) atomicAdd(&stats[2], hits);
    }
}

__global__ void __launch_bounds__(64)
k_sac_best(const SacPair* __restrict__ pairs, const SacHyp* __restrict__ hyp, const uint8_t* __restrict__ valid, const uint32_t* __restrict__ counts, SacLaunch L,
           SacOut* __restrict__ out, unsigned long long* __restrict__ stats)
{
    const uint32_t r = blockIdx.x, lane = threadIdx.x, H = L.max_iterations;
    uint32_t hi = 0u, lo = 0u;      // (count + 1, ~h) of the best valid hypothesis so far; hi = 0: none
    for (uint32_t h = lane; h < H; h += 64u) {
        if (!valid[(size_t)r * H + h]) continue;
        const uint32_t c1 = counts[(size_t)r * H + h] + 1u, nh = ~h;
        if (c1 > hi || (c1 == hi && nh > lo)) { hi = c1; lo = nh; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t ohi = __shfl_xor(hi, off, 64), olo = __shfl_xor(lo, off, 64);
        if (ohi > hi || (ohi == hi && olo > lo)) { hi = ohi; lo = olo; }
    }
    if (lane != 0u) return;
    SacOut& O = out[r];
    O.n_eval = pairs[r].n_eval;
    atomicAdd(&stats[1], (unsigned long long)O.n_prerejected);
    atomicAdd(&stats[3], 1ull);
    if (!hi) {
        const double qnan = __builtin_nan("");
        O.found = 0; O.best = -1; O.consensus = 0u;
        for (int d = 0; d < 16; ++d) O.T[d] = qnan;
        return;
    }
    const uint32_t h = ~lo;
    const SacHyp B = hyp[(size_t)r * H + h];
    O.best = (int32_t)h; O.consensus = hi - 1u;
    O.found = ((double)O.consensus >= L.inlier_fraction * (double)O.n_eval && O.consensus >= 3u) ? 1 : 0;
    for (int d = 0; d < 12; ++d) O.T[d] = B.T[d];
    O.T[12] = O.T[13] = O.T[14] = 0.0; O.T[15] = 1.0;
}

hipError_t sac_align(const SacRows* rows, const uint32_t* block_rows, uint32_t n_row_blocks, uint32_t* row, const SacPair* pairs, const uint32_t* block_pair,
                     uint32_t n_blocks, uint32_t n_pairs, const SacLaunch& L, SacHyp* hyp, uint8_t* valid, uint32_t* counts, SacOut* out,
                     unsigned long long* stats4, hipStream_t s)
{
    if (!n_pairs) return hipSuccess;
    if (L.max_iterations < 1u || L.max_iterations > (uint32_t)kSacMaxIterations || L.stride < 1u || L.kc < 1 || L.kc > kMatchMaxK) return hipErrorInvalidValue;
    const uint32_t bpp = (L.max_iterations + kSacBlock - 1) / kSacBlock;
    if ((uint64_t)n_pairs * bpp >= BlockTable::kMaxBlocks) return hipErrorInvalidValue;
    if (n_row_blocks) k_sac_rows<<<dim3(n_row_blocks), dim3(kSacBlock), 0, s>>>(rows, block_rows, row);
    k_sac_hypotheses<<<dim3(n_pairs * bpp), dim3(kSacBlock), 0, s>>>(pairs, L, bpp, hyp, valid, out);
    if (n_blocks) k_sac_vote<<<dim3(n_blocks), dim3(kSacBlock), 0, s>>>(pairs, block_pair, hyp, valid, L, counts, out, stats4);
    k_sac_best<<<dim3(n_pairs), dim3(64), 0, s>>>(pairs, hyp, valid, counts, L, out, stats4);
    return hipGetLastError();
}

} // namespace ltm
