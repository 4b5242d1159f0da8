// ltm_k_scancontext.hip -- Scan Context place recognition (ltslam/src/Scancontext.cpp:69-324): descriptor scatter, ring / sector keys and column
// norms, ring-key candidate search, and the column-shift cosine distance of descriptor pairs.
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
//
// Arithmetic: everything the reference does in double is done in double here, without contraction (-ffp-contract=off), in the order of the
// reference's loops; include/ltm.h ("scan context") states the semantics.  The pair distance is plain fp64 vector arithmetic, not
// v_mfma_f64_16x16x4: DESIGN.md section 4.4 gives the reasons.
#include "ltm_kernels_common.h"
#include <climits>
namespace ltm {

namespace {

constexpr int kScPtsPerThread = 8;          // points per thread of the scatter: one block pre-reduces 2048 points of one keyframe
constexpr int kScLdsBins = 4096;            // descriptors up to this many bins are pre-reduced in LDS (4 bytes per bin, 4.8 KB for 20 x 60), larger ones go straight to HBM
constexpr int kScPairBlock = 64;            // one wave per descriptor pair
constexpr size_t kScPairLdsMax = 60 << 10;  // both descriptors of a pair are staged in LDS when they fit

// max(min(n, int(ceil(v))), 1) as x86 evaluates it: a NaN or out-of-range double converts to INT_MIN (cvttsd2si), which the clamp turns into cell 1
__device__ __forceinline__ int sc_cell(double v, int n)
{
    const double c = ceil(v);
    const int i = (c >= -2147483648.0 && c < 2147483648.0) ? (int)c : INT_MIN;
    return max(min(n, i), 1);
}

// Scancontext.cpp:23-36 xy2theta + :171-179: bin of (x, y), or -1 for a point outside max_radius.  x == -0.0f takes the x >= 0 branches like the reference.
__device__ __forceinline__ int sc_bin(float x, float y, const ScGeom& g)
{
    constexpr double kDeg = 180.0 / 3.14159265358979323846;
    const float r = sqrtf(x * x + y * y);
    if ((double)r > g.max_radius) return -1;
    double t;
    if (x >= 0.0f && y >= 0.0f) t = kDeg * atan((double)(y / x));
    else if (x < 0.0f && y >= 0.0f) t = 180.0 - kDeg * atan((double)(y / (-x)));
    else if (x < 0.0f && y < 0.0f) t = 180.0 + kDeg * atan((double)(y / x));
    else t = 360.0 - kDeg * atan((double)((-y) / x));
    const float theta = (float)t;
    const int ring = sc_cell(((double)r / g.max_radius) * (double)g.R, g.R);
    const int sector = sc_cell(((double)theta / 360.0) * (double)g.S, g.S);
    return (ring - 1) * g.S + (sector - 1);
}

__device__ __forceinline__ void sc_max_u32(uint32_t* p, uint32_t v)      // relaxed pre-test: a bin only ever grows
{
    const uint32_t cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v > cur) atomicMax(p, v);
}

// makeScancontext :164-184 for every keyframe of a batch: grid = (chunks of the longest keyframe, keyframes) like the scan-image kernels.  bins: zeroed,
// R * S keys per keyframe.  kLds: R * S * 4 bytes of dynamic LDS.
template <bool kLds>
__global__ void __launch_bounds__(kBlock)
k_sc_scatter(const float4* __restrict__ scans, const uint64_t* __restrict__ offsets, size_t kb, ScGeom g, uint32_t* __restrict__ bins)
{
    extern __shared__ uint32_t sc_bins_sm[];      // kLds: R * S keys
    uint32_t* sm = sc_bins_sm;
    const int nbins = g.R * g.S;
    const uint64_t a = offsets[kb + blockIdx.y], n = offsets[kb + blockIdx.y + 1] - a;
    const uint64_t first = (uint64_t)blockIdx.x * (kBlock * kScPtsPerThread);
    if (first >= n) return;      // the whole block leaves
    uint32_t* __restrict__ out = bins + (size_t)blockIdx.y * (size_t)nbins;
    if (kLds) {
        for (int i = threadIdx.x; i < nbins; i += kBlock) sm[i] = 0u;
        __syncthreads();
    }
    for (int j = 0; j < kScPtsPerThread; ++j) {
        const uint64_t local = first + (uint64_t)j * kBlock + threadIdx.x;
        if (local >= n) break;
        const float4 p = scans[a + local];
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
        const int bin = sc_bin(p.x, p.y, g);
        if (bin < 0) continue;
        const uint32_t key = ordered_key((float)((double)p.z + g.lidar_height));      // integer atomic max; the zero-filled bins are below the key of every height: "no point"
        if (kLds) atomicMax(&sm[bin], key);
        else sc_max_u32(out + bin, key);
    }
    if (kLds) {
        __syncthreads();
        for (int i = threadIdx.x; i < nbins; i += kBlock) {
            const uint32_t k = sm[i];
            if (k) sc_max_u32(out + i, k);
        }
    }
}

// One block per descriptor: bins -> heights (:186-190; a bin that no value above -1000 reached is 0), then ring keys (row means, float), sector keys
// (column means) and column norms.  bins == nullptr: the heights are given (ltm_sc_from_descriptors).
__global__ void __launch_bounds__(kBlock)
k_sc_finish(const uint32_t* __restrict__ bins, int R, int S, double* __restrict__ desc, float* __restrict__ ring_keys, double* __restrict__ sector_keys,
            double* __restrict__ norms)
{
    const size_t d = blockIdx.x, nb = (size_t)R * (size_t)S;
    double* D = desc + d * nb;
    if (bins) {
        for (size_t i = threadIdx.x; i < nb; i += kBlock) {
            const uint32_t k = bins[d * nb + i];
            const float v = k ? ordered_unkey(k) : -1000.0f;
            D[i] = (v > -1000.0f) ? (double)v : 0.0;
        }
        __syncthreads();
    }
    for (int c = threadIdx.x; c < S; c += kBlock) {
        double sum = 0.0, sq = 0.0;
        for (int r = 0; r < R; ++r) {
            const double v = D[(size_t)r * S + c];
            sum = sum + v;
            sq = sq + v * v;
        }
        sector_keys[d * S + c] = sum / (double)R;
        norms[d * S + c] = sqrt(sq);
    }
    for (int r = threadIdx.x; r < R; r += kBlock) {
        double sum = 0.0;
        for (int c = 0; c < S; ++c) sum = sum + D[(size_t)r * S + c];
        ring_keys[d * R + r] = (float)(sum / (double)S);
    }
}

// nanoflann's L2_Adaptor::evalMetric in float (nanoflann.hpp:383-409): groups of four, then the tail
__global__ void __launch_bounds__(kBlock)
k_sc_ring_distances(const float* __restrict__ qk, size_t nq, const float* __restrict__ dbk, size_t nd, int R, float* __restrict__ rd)
{
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nq * nd) return;
    const float* __restrict__ a = qk + (t / nd) * R;
    const float* __restrict__ b = dbk + (t % nd) * R;
    float result = 0.0f;
    int d = 0;
    for (; d + 3 < R; d += 4) {
        const float d0 = a[d] - b[d], d1 = a[d + 1] - b[d + 1], d2 = a[d + 2] - b[d + 2], d3 = a[d + 3] - b[d + 3];
        result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    for (; d < R; ++d) {
        const float d0 = a[d] - b[d];
        result += d0 * d0;
    }
    rd[t] = result;
}

// The candidates' order: (key distance is NaN, key distance, index) ascending -- a NaN sorts after everything, +inf included, and NaNs among
// themselves by index.  True if candidate (d, j) comes before (pd, pj).
__device__ __forceinline__ bool sc_key_before(float d, int j, float pd, int pj)
{
    const bool n = d != d, pn = pd != pd;
    if (n != pn) return pn;
    return (!n && d < pd) || ((n || d == pd) && j < pj);
}

// The K nearest ring keys of every query in sc_key_before order (ascending (distance, index), NaN distances last): one wave per query, K selection rounds over its row of rd.
// pairs[(q * K + k) * 2] = {q, index}.  K <= nd.
__global__ void __launch_bounds__(64)
k_sc_candidates(const float* __restrict__ rd, size_t nd, int K, int32_t* __restrict__ pairs)
{
    const size_t q = blockIdx.x;
    const float* __restrict__ row = rd + q * nd;
    float pd = -1.0f;
    int pj = -1;
    for (int k = 0; k < K; ++k) {
        float bd = __builtin_nanf("");      // (NaN, INT_MAX): after every entry
        int bj = INT_MAX;
        for (size_t j = threadIdx.x; j < nd; j += 64) {
            const float d = row[j];
            if (sc_key_before(pd, pj, d, (int)j) && sc_key_before(d, (int)j, bd, bj)) { bd = d; bj = (int)j; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(bd, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (sc_key_before(od, oj, bd, bj)) { bd = od; bj = oj; }
        }
        pd = bd; pj = bj;
        if (threadIdx.x == 0) {
            pairs[(q * (size_t)K + k) * 2] = (int32_t)q;
            pairs[(q * (size_t)K + k) * 2 + 1] = bj;
        }
    }
}

// distanceBtnScanContext(a[i], b[j]) (:116-148) of one pair per wave.  Lane s owns shift s (and s + 64, ...): the sector-key alignment
// (fastAlignUsingVkey :93-113), then distDirectSC (:69-90) of every shift within `radius` of the aligned one.  Shifting b's columns right by s puts
// b's column (c - s) mod S under a's column c, so nothing is moved: the lane walks b with an offset.  The descriptors are row-major
// [ring][sector]: at a given (ring, column) a's element is one LDS broadcast and the lanes' elements of b are consecutive words.
// pairs == nullptr: pair p is (p / nd, p % nd).
template <bool kLds>
__global__ void __launch_bounds__(kScPairBlock)
k_sc_pair(const double* __restrict__ descA, const double* __restrict__ skA, const double* __restrict__ nrmA, const double* __restrict__ descB,
          const double* __restrict__ skB, const double* __restrict__ nrmB, int R, int S, const int32_t* __restrict__ pairs, size_t nd, int radius,
          double* __restrict__ dist, int32_t* __restrict__ shift)
{
    extern __shared__ double sc_sm[];
    const size_t p = blockIdx.x, nb = (size_t)R * (size_t)S;
    const size_t i = pairs ? (size_t)pairs[2 * p] : p / nd, j = pairs ? (size_t)pairs[2 * p + 1] : p % nd;
    double* tmp = sc_sm;                 // one value per shift
    double* ska = tmp + S;
    double* skb = ska + S;
    double* na = skb + S;
    double* nbm = na + S;
    double* la = nbm + S;                // kLds: the two descriptors
    double* lb = la + nb;
    for (int c = threadIdx.x; c < S; c += kScPairBlock) {
        ska[c] = skA[i * S + c]; skb[c] = skB[j * S + c];
        na[c] = nrmA[i * S + c]; nbm[c] = nrmB[j * S + c];
    }
    const double* __restrict__ A = descA + i * nb;
    const double* __restrict__ B = descB + j * nb;
    if (kLds)
        for (size_t e = threadIdx.x; e < nb; e += kScPairBlock) { la[e] = A[e]; lb[e] = B[e]; }
    __syncthreads();
    // 1. alignment by the sector keys: the first shift with the smallest ||vkey_a - shift(vkey_b, s)||
    for (int s = threadIdx.x; s < S; s += kScPairBlock) {
        double acc = 0.0;
        int jj = (s == 0) ? 0 : S - s;      // (0 - s) mod S
        for (int c = 0; c < S; ++c) {
            const double dl = ska[c] - skb[jj];
            acc = acc + dl * dl;
            if (++jj == S) jj = 0;
        }
        tmp[s] = sqrt(acc);
    }
    __syncthreads();
    int a0 = 0;
    {
        double mn = 10000000.0;
        for (int s = 0; s < S; ++s) {
            const double v = tmp[s];
            if (v < mn) { mn = v; a0 = s; }
        }
    }
    __syncthreads();
    // 2. column-wise cosine distance at every shift of the search space
    for (int s = threadIdx.x; s < S; s += kScPairBlock) {
        int cd = s - a0;
        if (cd < 0) cd += S;
        cd = min(cd, S - cd);
        double res = __builtin_nan("");      // not in the search space: never below the running minimum
        if (cd <= radius) {
            double sum = 0.0;
            int count = 0;
            int jj = (s == 0) ? 0 : S - s;
            for (int c = 0; c < S; ++c) {
                const double n1 = na[c], n2 = nbm[jj];
                if (!(n1 == 0.0 || n2 == 0.0)) {
                    double dot = 0.0;
                    if (kLds) {
                        for (int r = 0; r < R; ++r) dot = dot + la[r * S + c] * lb[r * S + jj];
                    } else {
                        for (int r = 0; r < R; ++r) dot = dot + A[(size_t)r * S + c] * B[(size_t)r * S + jj];
                    }
                    sum = sum + dot / (n1 * n2);
                    ++count;
                }
                if (++jj == S) jj = 0;
            }
            res = 1.0 - sum / (double)count;      // count == 0: NaN, as the reference gives
        }
        tmp[s] = res;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double mn = 10000000.0;
        int arg = 0;
        for (int s = 0; s < S; ++s) {
            const double v = tmp[s];
            if (v < mn) { mn = v; arg = s; }
        }
        dist[p] = mn;
        shift[p] = arg;
    }
}

// detectLoopClosureIDBetweenSession :296-311 for one query per wave: the candidate with the smallest distance, the first one in sc_key_before order (ring-key
// distance, index; NaN last) among equals.  A candidate whose distance is NaN or not below 10000000 never wins (nn_idx 0, shift 0 if none does).
__global__ void __launch_bounds__(64)
k_sc_detect_reduce(const double* __restrict__ dist, const int32_t* __restrict__ shift, const int32_t* __restrict__ pairs, const float* __restrict__ rd,
                   size_t nd, size_t K, int32_t* __restrict__ nn_idx, double* __restrict__ min_dist, int32_t* __restrict__ nn_align)
{
    const size_t q = blockIdx.x;
    double bd = 10000000.0;
    float br = 0.0f;
    int bj = -1, bs = 0;
    for (size_t k = threadIdx.x; k < K; k += 64) {
        const size_t p = q * K + k;
        const double d = dist[p];
        if (!(d < 10000000.0)) continue;
        const int j = pairs ? pairs[2 * p + 1] : (int)k;
        const float r = rd[q * nd + (size_t)j];
        if (bj < 0 || d < bd || (d == bd && sc_key_before(r, j, br, bj))) { bd = d; br = r; bj = j; bs = shift[p]; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(bd, off, 64);
        const float orr = __shfl_xor(br, off, 64);
        const int oj = __shfl_xor(bj, off, 64), os = __shfl_xor(bs, off, 64);
        if (oj >= 0 && (bj < 0 || od < bd || (od == bd && sc_key_before(orr, oj, br, bj)))) { bd = od; br = orr; bj = oj; bs = os; }
    }
    if (threadIdx.x == 0) {
        nn_idx[q] = bj < 0 ? 0 : bj;
        min_dist[q] = bd;
        nn_align[q] = bs;
    }
}

size_t sc_pair_lds_bytes(int R, int S, bool* fits)
{
    const size_t small = (size_t)5 * S * sizeof(double), full = small + (size_t)2 * R * S * sizeof(double);
    *fits = full <= kScPairLdsMax;
    return *fits ? full : small;
}

bool sc_scatter_in_lds(int R, int S) { return R * S <= kScLdsBins; }

} // namespace

void sc_paths(int R, int S, bool* scatter_in_lds, bool* pair_in_lds)
{
    *scatter_in_lds = sc_scatter_in_lds(R, S);
    sc_pair_lds_bytes(R, S, pair_in_lds);
}

hipError_t sc_scatter(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t nb, uint64_t max_kf_pts, ScGeom g, uint32_t* bins, hipStream_t s)
{
    if (!nb || !max_kf_pts) return hipSuccess;
    const unsigned gx = grid_for(max_kf_pts, kBlock * kScPtsPerThread);
    for (size_t k0 = 0; k0 < nb; k0 += 65535) {       // gridDim.y limit
        const size_t nk = std::min<size_t>(65535, nb - k0);
        uint32_t* out = bins + k0 * (size_t)g.R * (size_t)g.S;
        if (sc_scatter_in_lds(g.R, g.S)) k_sc_scatter<true><<<dim3(gx, (unsigned)nk), dim3(kBlock), (size_t)g.R * g.S * sizeof(uint32_t), s>>>(scans, offsets_dev, kb + k0, g, out);
        else k_sc_scatter<false><<<dim3(gx, (unsigned)nk), dim3(kBlock), 0, s>>>(scans, offsets_dev, kb + k0, g, out);
    }
    return hipGetLastError();
}

hipError_t sc_finish(const uint32_t* bins, size_t n, int R, int S, double* desc, float* ring_keys, double* sector_keys, double* norms, hipStream_t s)
{
    if (!n) return hipSuccess;
    k_sc_finish<<<dim3((unsigned)n), dim3(kBlock), 0, s>>>(bins, R, S, desc, ring_keys, sector_keys, norms);
    return hipGetLastError();
}

hipError_t sc_ring_distances(const float* qk, size_t nq, const float* dbk, size_t nd, int R, float* rd, hipStream_t s)
{
    if (!nq || !nd) return hipSuccess;
    k_sc_ring_distances<<<dim3(grid_for(nq * nd)), dim3(kBlock), 0, s>>>(qk, nq, dbk, nd, R, rd);
    return hipGetLastError();
}

hipError_t sc_candidates(const float* rd, size_t nq, size_t nd, int K, int32_t* pairs, hipStream_t s)
{
    if (!nq || K < 1) return hipSuccess;
    k_sc_candidates<<<dim3((unsigned)nq), dim3(64), 0, s>>>(rd, nd, K, pairs);
    return hipGetLastError();
}

hipError_t sc_pair_distance(const double* descA, const double* skA, const double* nrmA, const double* descB, const double* skB, const double* nrmB, int R, int S,
                            const int32_t* pairs, size_t nd, size_t n_pairs, int radius, double* dist, int32_t* shift, hipStream_t s)
{
    if (!n_pairs) return hipSuccess;
    bool fits = false;
    const size_t lds = sc_pair_lds_bytes(R, S, &fits);
    if (fits) k_sc_pair<true><<<dim3((unsigned)n_pairs), dim3(kScPairBlock), lds, s>>>(descA, skA, nrmA, descB, skB, nrmB, R, S, pairs, nd, radius, dist, shift);
    else k_sc_pair<false><<<dim3((unsigned)n_pairs), dim3(kScPairBlock), lds, s>>>(descA, skA, nrmA, descB, skB, nrmB, R, S, pairs, nd, radius, dist, shift);
    return hipGetLastError();
}

hipError_t sc_detect_reduce(const double* dist, const int32_t* shift, const int32_t* pairs, const float* rd, size_t nq, size_t nd, size_t K,
                            int32_t* nn_idx, double* min_dist, int32_t* nn_align, hipStream_t s)
{
    if (!nq) return hipSuccess;
    k_sc_detect_reduce<<<dim3((unsigned)nq), dim3(64), 0, s>>>(dist, shift, pairs, rd, nd, K, nn_idx, min_dist, nn_align);
    return hipGetLastError();
}

} // namespace ltm
