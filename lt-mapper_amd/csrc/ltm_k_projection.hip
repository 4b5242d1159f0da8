// ltm_k_projection.hip -- range-image projection, the remove / revert visibility vote, the exact arg-min image and its occlusion cull (utility.cpp:38-142, Removerter.cpp:109-156, 381-593)
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
#include "ltm_kernels_common.h"
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace ltm {

// ------------------------------------------------------------------------------------ fills
__global__ void k_fill_u32(uint32_t* p, uint32_t v, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}
__global__ void k_fill_u64(uint64_t* p, uint64_t v, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}
hipError_t fill_u32(uint32_t* p, uint32_t v, size_t n, hipStream_t s)
{
    if (!n) return hipSuccess;
    k_fill_u32<<<dim3((unsigned)std::min<size_t>(grid_for(n), 8192)), dim3(kBlock), 0, s>>>(p, v, n);
    return hipGetLastError();
}
hipError_t fill_u64(uint64_t* p, uint64_t v, size_t n, hipStream_t s)
{
    if (!n) return hipSuccess;
    k_fill_u64<<<dim3((unsigned)std::min<size_t>(grid_for(n), 8192)), dim3(kBlock), 0, s>>>(p, v, n);
    return hipGetLastError();
}

// Removerter.cpp:109-156 scan2RangeImg, all keyframes of a batch and up to kMaxScanShapes image shapes in one launch: the remove / revert passes of selfRemovert
// project every scan into six shapes (2.5, 2.375, 2.0, 1.9, 1.5, 1.425 pixels per degree).  The point is read once, the exact atan2f / sqrtf chain and the two
// divisions by the field of view (shape-independent) run once, and each shape costs a multiply, a round, a clamp and its atomic -- bit for bit pixel_row_col's
// arithmetic.  grid = (chunks of the longest keyframe, keyframes): the keyframe comes from blockIdx.y instead of a binary search over the offsets.
struct ScanShapes { int n; int rows[kMaxScanShapes], cols[kMaxScanShapes]; uint32_t* img[kMaxScanShapes]; };
// pixel_row_col's arithmetic in its shape-independent and per-shape parts: the row and column fractions of a direction, and the clamped pixel of a fraction
__device__ __forceinline__ float scan_row_frac(const RimgGeom& g, float el)
{
    const float el_deg = g.fast ? rad2deg_fast(el) : rad2deg_exact(el);
    return 1.0f - div_by_const(el_deg + g.half_v, g.vfov, g.inv_v, g.fast);
}
__device__ __forceinline__ float scan_col_frac(const RimgGeom& g, float az)
{
    const float az_deg = g.fast ? rad2deg_fast(az) : rad2deg_exact(az);
    return div_by_const(az_deg + g.half_h, g.hfov, g.inv_h, g.fast);
}
__device__ __forceinline__ int scan_clamped_px(float fn, float frac)      // fn = (float)rows or (float)cols
{
    float f = roundf(fn * frac);
    f = (f < 0.0f) ? 0.0f : f;  f = (fn - 1.0f < f) ? fn - 1.0f : f;
    return (int)f;
}
__global__ void __launch_bounds__(kBlock)
k_scan_rimg_multi(const float4* __restrict__ scans, const uint64_t* __restrict__ offsets, size_t kb, Geom gg, ScanShapes sh)
{
    const size_t lo = kb + blockIdx.y;
    const uint64_t a = offsets[lo], local = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= offsets[lo + 1] - a) return;
    const RimgGeom g = make_geom(gg);      // rows / cols of gg are not used: only the field of view and the fast-form switch
    const float4 p = scans[a + local];
    const Sph s = cart2sph(p.x, p.y, p.z);
    const float u = scan_row_frac(g, s.el);
    const float w = scan_col_frac(g, s.az);
    const uint32_t rbits = f2u(s.r);
#pragma unroll
    for (int j = 0; j < kMaxScanShapes; ++j) {
        if (j >= sh.n) break;
        const int row = scan_clamped_px((float)sh.rows[j], u), col = scan_clamped_px((float)sh.cols[j], w);
        const size_t npx = (size_t)sh.rows[j] * (size_t)sh.cols[j];
        img_min_u32(sh.img[j] + (size_t)blockIdx.y * npx + (size_t)(row * sh.cols[j] + col), rbits);
    }
}

// smax[kf] = float bits of the largest NON-EMPTY (< 10000) pixel of the finished scan image of keyframe kf: a map point farther than
// smax - thr cannot be flagged in mode 0.  grid = (chunks, keyframes); positive floats order like their bit patterns.
__global__ void __launch_bounds__(kBlock)
k_image_max(const uint32_t* __restrict__ img, uint32_t npx, uint32_t* __restrict__ smax)
{
    __shared__ uint32_t sm[kBlock / 64];
    const uint32_t* __restrict__ imgk = img + (size_t)blockIdx.y * npx;
    uint32_t m = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
        const uint32_t v = imgk[i];
        m = max(m, (v < 0x461c4000u /* 10000.0f = empty */) ? v : 0u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) m = max(m, sm[w]);
        m = max(m, sm[0]);
        if (m) atomicMax(smax + blockIdx.y, m);
    }
}

// qbound[px] for the range-culled vote (mode 0, diff = scan - map > thr): a map point of this pixel can only be flagged if its
// exact range r_e < s - thr (+ float rounding of the subtraction, <= 2e-5 for |diff| < 200).  The kernel tests the squared range
// r2 of its approximate projection, r_e^2 >= r2 (1 - 3e-6) (validated bound), so it may drop the point iff
// r2 >= ((s - thr + 1e-3) (1 + 1e-5))^2, rounded up.  Empty pixels (10000) never flag below 9800 m (and farther points take the
// exact path): 0.  Evaluated in double, rounded up to float.
__device__ __forceinline__ float scan_qbound_of(uint32_t sb, float thr)
{
    float q = 0.0f;
    if (sb < kNoPointBits) {
        const double lim = ((double)u2f(sb) - (double)thr + 1.0e-3) * (1.0 + 1.0e-5);
        if (lim > 0.0) {
            const double q2 = lim * lim;
            q = (float)q2;
            if ((double)q < q2) q = u2f(f2u(q) + 1u);      // round up (q > 0)
        }
    }
    return q;
}
__global__ void __launch_bounds__(kBlock)
k_scan_qbound(const uint32_t* __restrict__ scan_img, size_t n, float thr, float* __restrict__ qbound)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    qbound[i] = scan_qbound_of(scan_img[i], thr);
}
hipError_t scan_qbound(const uint32_t* scan_img, size_t n, float thr, float* qbound, hipStream_t s)
{
    if (!n) return hipSuccess;
    k_scan_qbound<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(scan_img, n, thr, qbound);
    return hipGetLastError();
}

hipError_t scan_range_images_multi(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t nb, uint64_t n_pts, uint64_t max_kf_pts, Geom g,
                                   int n_shapes, const int* rows, const int* cols, uint32_t* const* imgs, uint32_t* const* smax_bits, hipStream_t s)
{
    if (n_shapes < 1 || n_shapes > kMaxScanShapes) return hipErrorInvalidValue;
    ScanShapes sh{};
    sh.n = n_shapes;
    for (int j = 0; j < n_shapes; ++j) { sh.rows[j] = rows[j]; sh.cols[j] = cols[j]; sh.img[j] = imgs[j]; }
    if (n_pts && max_kf_pts)
        for (size_t k0 = 0; k0 < nb; k0 += 65535) {       // gridDim.y limit
            const size_t nk = std::min<size_t>(65535, nb - k0);
            ScanShapes part = sh;
            for (int j = 0; j < n_shapes; ++j) part.img[j] = sh.img[j] + k0 * (size_t)rows[j] * (size_t)cols[j];
            k_scan_rimg_multi<<<dim3(grid_for(max_kf_pts), (unsigned)nk), dim3(kBlock), 0, s>>>(scans, offsets_dev, kb + k0, g, part);
        }
    if (nb)
        for (int j = 0; j < n_shapes; ++j) {
            if (!smax_bits || !smax_bits[j]) continue;
            const uint32_t npx = (uint32_t)(rows[j] * cols[j]);
            k_image_max<<<dim3(std::min<unsigned>(grid_for(npx, kBlock * 8), 64), (unsigned)nb), dim3(kBlock), 0, s>>>(imgs[j], npx, smax_bits[j]);
        }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------ scan images built in LDS
// The same images without a fill, without global atomics and without the two read-back passes (k_image_max, k_scan_qbound): one workgroup owns one band of
// one keyframe (ltm_kernels.h: ScanBands), keeps the band's rows of every shape in LDS, streams ALL points of the keyframe over it and writes every pixel of
// the band out exactly once, with the per-shape maximum and (when a threshold is given) the bound image in the same loop.
//   * Per point and band only a first reject runs: z against tan(elevation) * sqrt(x^2 + y^2) for the two elevations that bound the band's rows over all
//     shapes, widened by kScanBandMarginDeg (0.01 degrees, four orders of magnitude above the float error of either side).  It only ever lets too many
//     points through: what passes is projected with today's arithmetic (cart2sph, the row / column fractions, multiply / round / clamp per shape) and
//     enters a shape only when its exact row lies in the band, so the images do not depend on the reject, only the time.  The bands cut all shapes at
//     the same elevations, so a point passes in one band, seldom two.  (The exact elevation half in every band, the first form, was VALU-bound at four
//     times the time: NOTEBOOK 4.1.)
//   * The points that pass are queued per wave in LDS and projected 64 at a time: the exact arithmetic runs with full waves whatever the order of the
//     scan (ring-major scans pass whole waves, voxel-ordered ones a few lanes of each).
//   * Workgroups b, b + 8, b + 16, ... run on the same XCD (see tile_kf_of_block): the bands of a keyframe follow each other there, so its points come from
//     HBM once and from that XCD's L2 for the other bands.
// The minimum of positive float bit patterns does not depend on the order, so the images are those of k_scan_rimg_multi bit for bit.
struct ScanLdsArgs {
    int n, n_bands;
    int rows[kMaxScanShapes], cols[kMaxScanShapes];
    uint32_t* img[kMaxScanShapes]; uint32_t* smax[kMaxScanShapes]; float* qbound[kMaxScanShapes];
    float thr;
};
__global__ void __launch_bounds__(kScanLdsThreads)
k_scan_rimg_lds(const float4* __restrict__ scans, const uint64_t* __restrict__ offsets, size_t kb, uint32_t nk, Geom gg, ScanLdsArgs sh)
{
    constexpr int kWaves = kScanLdsThreads / 64;
    __shared__ uint4 s_img4[kScanLdsBudget / 16];
    __shared__ uint32_t s_queue[kWaves][128];
    __shared__ uint32_t s_max[kMaxScanShapes][kWaves];
    static_assert(sizeof(s_img4) + sizeof(s_queue) + sizeof(s_max) == (size_t)160 * 1024, "the workgroup declares the CU's whole LDS");
    uint32_t* const s_img = reinterpret_cast<uint32_t*>(s_img4);

    const uint32_t b = blockIdx.x, q8 = b >> 3;
    const uint32_t band = q8 % (uint32_t)sh.n_bands, kfl = (q8 / (uint32_t)sh.n_bands) * 8u + (b & 7u);
    if (kfl >= nk) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const RimgGeom g = make_geom(gg);      // rows / cols of gg are not used: only the field of view and the fast-form switch

    // the band: per shape its rows [row0, row1), the LDS word its first pixel sits at, the global pixel that is
    int row0[kMaxScanShapes], row1[kMaxScanShapes];
    uint32_t lbase[kMaxScanShapes];
    uint32_t band_words = 0;
#pragma unroll
    for (int j = 0; j < kMaxScanShapes; ++j) {
        row0[j] = row1[j] = 0; lbase[j] = 0;
        if (j >= sh.n) continue;
        row0[j] = scan_band_row0(sh.rows[j], sh.n_bands, (int)band);
        row1[j] = scan_band_row0(sh.rows[j], sh.n_bands, (int)band + 1);
        lbase[j] = band_words;
        band_words += (uint32_t)scan_band_shape_words(row1[j] - row0[j], sh.cols[j]);
    }
    for (uint32_t i = tid; i < band_words / 4u; i += kScanLdsThreads) s_img4[i] = make_uint4(kNoPointBits, kNoPointBits, kNoPointBits, kNoPointBits);
    // (shape j's pixels start `pad` words into its range, pad = the global pixel offset mod 4: an aligned group of four in LDS is an aligned group in HBM)
    uint32_t pad[kMaxScanShapes];
#pragma unroll
    for (int j = 0; j < kMaxScanShapes; ++j) {
        pad[j] = 0;
        if (j >= sh.n) continue;
        const size_t gofs = (size_t)kfl * ((size_t)sh.rows[j] * (size_t)sh.cols[j]) + (size_t)row0[j] * (size_t)sh.cols[j];
        pad[j] = (uint32_t)(gofs & 3u);
    }
    __syncthreads();

    const size_t lo = kb + kfl;
    const uint64_t a = offsets[lo];
    const uint32_t n = (uint32_t)(offsets[lo + 1] - a);
    const float4* __restrict__ pts = scans + a;
    uint32_t qn = 0;      // entries in this wave's queue (wave-uniform, < 64 between points)

    // the first reject: tangents of the elevations that bound the band (see above); a side that reaches the image's first / last row, where everything
    // beyond is clamped into the band, or comes within a degree of the pole, is not tested
    float t_lo = 0.0f, t_hi = 0.0f;
    bool has_lo = false, has_hi = false;
    {
        double el_lo = 1.0e9, el_hi = -1.0e9;      // degrees
        bool open_lo = false, open_hi = false;
#pragma unroll
        for (int j = 0; j < kMaxScanShapes; ++j) {
            if (j >= sh.n || row1[j] <= row0[j]) continue;
            // row = round(rows * u), u = 1 - (el_deg + vfov / 2) / vfov: row >= row0 <=> rows * u >= row0 - 0.5, row < row1 <=> rows * u < row1 - 0.5
            if (row0[j] == 0) open_hi = true;
            else el_hi = fmax(el_hi, (1.0 - ((double)row0[j] - 0.5) / (double)sh.rows[j]) * (double)gg.vfov - 0.5 * (double)gg.vfov);
            if (row1[j] == sh.rows[j]) open_lo = true;
            else el_lo = fmin(el_lo, (1.0 - ((double)row1[j] - 0.5) / (double)sh.rows[j]) * (double)gg.vfov - 0.5 * (double)gg.vfov);
        }
        el_lo -= kScanBandMarginDeg; el_hi += kScanBandMarginDeg;
        has_lo = !open_lo && el_lo > -89.0 && el_lo < 89.0;
        has_hi = !open_hi && el_hi > -89.0 && el_hi < 89.0;
        if (el_lo >= 89.0 && !open_lo) { has_lo = true; el_lo = 89.0; }          // (a band wholly above 89 degrees: still a lower bound)
        if (el_hi <= -89.0 && !open_hi) { has_hi = true; el_hi = -89.0; }
        if (has_lo) t_lo = (float)tan(el_lo * (3.14159265358979323846 / 180.0));
        if (has_hi) t_hi = (float)tan(el_hi * (3.14159265358979323846 / 180.0));
    }

    auto drain = [&](uint32_t from, uint32_t cnt) {      // project queue entries [from, from + cnt), cnt <= 64
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the entries were written by other lanes of this wave
        if (lane < cnt) {
            const float4 p = pts[s_queue[wave][from + lane]];
            const Sph sp = cart2sph(p.x, p.y, p.z);
            const float u = scan_row_frac(g, sp.el), w = scan_col_frac(g, sp.az);
            const uint32_t rbits = f2u(sp.r);
#pragma unroll
            for (int j = 0; j < kMaxScanShapes; ++j) {
                if (j >= sh.n) break;
                const int row = scan_clamped_px((float)sh.rows[j], u);
                if (row >= row0[j] && row < row1[j]) {
                    const int col = scan_clamped_px((float)sh.cols[j], w);
                    atomicMin(&s_img[lbase[j] + pad[j] + (uint32_t)((row - row0[j]) * sh.cols[j] + col)], rbits);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // read before the next points overwrite them
    };

    constexpr uint32_t kAhead = 4;      // loads in flight per lane
    for (uint32_t i0 = 0; i0 < n; i0 += kScanLdsThreads * kAhead) {      // (block-uniform trip count)
        float4 p[kAhead];
#pragma unroll
        for (uint32_t k = 0; k < kAhead; ++k) {
            const uint32_t i = i0 + k * kScanLdsThreads + tid;
            p[k] = pts[i < n ? i : 0u];      // (n > 0 inside the loop)
        }
#pragma unroll
        for (uint32_t k = 0; k < kAhead; ++k) {
            const uint32_t i = i0 + k * kScanLdsThreads + tid;
            const float xx = p[k].x * p[k].x, yy = p[k].y * p[k].y;
            const float xy = xx + yy;
            const float rho = __builtin_amdgcn_sqrtf(xy);
            // written as rejects, so that a NaN anywhere passes; so does a point on the axis (xy tiny: elevation +-90 degrees or, at the origin, 0)
            const bool out = (xy > 1.0e-30f) && ((has_lo && p[k].z < t_lo * rho) || (has_hi && p[k].z > t_hi * rho));
            const bool hit = !out && i < n;
            const uint64_t m = __ballot(hit);
            if (m) {
                if (hit) s_queue[wave][qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = i;
                qn += (uint32_t)__popcll(m);
                if (qn >= 64u) { qn -= 64u; drain(qn, 64u); }
            }
        }
    }
    if (qn) drain(0u, qn);
    __syncthreads();

    // write-out: every pixel of the band once, in aligned groups of four; the first and last group of a range may be shared with the neighbouring band or
    // keyframe and go out pixel by pixel
#pragma unroll
    for (int j = 0; j < kMaxScanShapes; ++j) {
        if (j >= sh.n) break;
        const uint32_t nw = (uint32_t)((row1[j] - row0[j]) * sh.cols[j]);
        uint32_t mx = 0;
        if (nw) {
            const size_t gofs = (size_t)kfl * ((size_t)sh.rows[j] * (size_t)sh.cols[j]) + (size_t)row0[j] * (size_t)sh.cols[j] - pad[j];      // multiple of 4
            uint32_t* __restrict__ gimg = sh.img[j] + gofs;
            float* __restrict__ gq = sh.qbound[j] ? sh.qbound[j] + gofs : nullptr;
            const uint32_t end = pad[j] + nw, ngroups = (end + 3u) >> 2;
            for (uint32_t k = tid; k < ngroups; k += kScanLdsThreads) {
                const uint4 v = s_img4[(lbase[j] >> 2) + k];
                const uint32_t w0 = k * 4u;
                if (w0 >= pad[j] && w0 + 4u <= end) {
                    reinterpret_cast<uint4*>(gimg)[k] = v;
                    mx = max(mx, v.x < kNoPointBits ? v.x : 0u); mx = max(mx, v.y < kNoPointBits ? v.y : 0u);
                    mx = max(mx, v.z < kNoPointBits ? v.z : 0u); mx = max(mx, v.w < kNoPointBits ? v.w : 0u);
                    if (gq) reinterpret_cast<float4*>(gq)[k] = make_float4(scan_qbound_of(v.x, sh.thr), scan_qbound_of(v.y, sh.thr), scan_qbound_of(v.z, sh.thr), scan_qbound_of(v.w, sh.thr));
                } else {
                    const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (uint32_t t = 0; t < 4u; ++t) {
                        if (w0 + t < pad[j] || w0 + t >= end) continue;
                        gimg[w0 + t] = e[t];
                        mx = max(mx, e[t] < kNoPointBits ? e[t] : 0u);
                        if (gq) gq[w0 + t] = scan_qbound_of(e[t], sh.thr);
                    }
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
        if (lane == 0) s_max[j][wave] = mx;
    }
    __syncthreads();
    if (tid < (uint32_t)sh.n) {
        uint32_t mx = 0;
        for (int w = 0; w < kWaves; ++w) mx = max(mx, s_max[tid][w]);
        // (dynamic index into the argument arrays would put them into scratch: select)
        uint32_t* smax = nullptr;
#pragma unroll
        for (int j = 0; j < kMaxScanShapes; ++j) smax = ((int)tid == j) ? sh.smax[j] : smax;
        if (mx && smax) atomicMax(smax + kfl, mx);
    }
}

size_t scan_band_bytes(const ScanBands& p, int b)
{
    size_t words = 0;
    for (int j = 0; j < p.n_shapes; ++j) words += scan_band_shape_words(scan_band_row0(p.rows[j], p.n_bands, b + 1) - scan_band_row0(p.rows[j], p.n_bands, b), p.cols[j]);
    return words * 4;
}
bool make_scan_bands(int n_shapes, const int* rows, const int* cols, size_t budget, ScanBands* out)
{
    if (n_shapes < 1 || n_shapes > kMaxScanShapes || !rows || !cols || !out) return false;
    ScanBands p{};
    p.n_shapes = n_shapes;
    int max_rows = 0;
    size_t all = 0;
    for (int j = 0; j < n_shapes; ++j) {
        if (rows[j] < 1 || cols[j] < 1 || (size_t)rows[j] * (size_t)cols[j] > 0x7fffffffull) return false;
        p.rows[j] = rows[j]; p.cols[j] = cols[j];
        max_rows = std::max(max_rows, rows[j]);
        all += scan_band_shape_words(rows[j], cols[j]) * 4;
    }
    // more bands than the tallest shape has rows cut nothing smaller: band 0 then still holds one row of every shape
    const int last = std::min(max_rows, kMaxScanBands);
    for (int nb = (int)std::min<size_t>((all + budget - 1) / std::max<size_t>(budget, 1), (size_t)last); nb <= last; ++nb) {
        if (nb < 1) continue;
        p.n_bands = nb;
        size_t worst = 0;
        for (int b = 0; b < nb && worst <= budget; ++b) worst = std::max(worst, scan_band_bytes(p, b));
        if (worst <= budget) { p.max_band_bytes = worst; *out = p; return true; }
    }
    return false;
}

hipError_t scan_range_images_lds(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t nb, Geom g, const ScanBands& plan,
                                 uint32_t* const* imgs, uint32_t* const* smax_bits, float* const* qbounds, float thr, hipStream_t s)
{
    if (plan.n_shapes < 1 || plan.n_shapes > kMaxScanShapes || plan.n_bands < 1 || plan.max_band_bytes > kScanLdsBudget) return hipErrorInvalidValue;
    for (int b = 0; b < plan.n_bands; ++b)
        if (scan_band_bytes(plan, b) > kScanLdsBudget) return hipErrorInvalidValue;      // the kernel lays its LDS out by the same formula
    ScanLdsArgs sh{};
    sh.n = plan.n_shapes; sh.n_bands = plan.n_bands; sh.thr = thr;
    for (int j = 0; j < plan.n_shapes; ++j) {
        if ((reinterpret_cast<uintptr_t>(imgs[j]) & 15u) || (qbounds && (reinterpret_cast<uintptr_t>(qbounds[j]) & 15u))) return hipErrorInvalidValue;
        sh.rows[j] = plan.rows[j]; sh.cols[j] = plan.cols[j];
    }
    const size_t per_launch = std::max<size_t>(8, (((size_t)1 << 30) / (size_t)plan.n_bands) & ~(size_t)7);      // keyframes of one grid, a multiple of 8
    for (size_t k0 = 0; k0 < nb; k0 += per_launch) {
        const size_t nk = std::min(per_launch, nb - k0);
        for (int j = 0; j < plan.n_shapes; ++j) {
            const size_t npx = (size_t)plan.rows[j] * (size_t)plan.cols[j];      // (k0 is a multiple of 8: the alignment holds)
            sh.img[j] = imgs[j] + k0 * npx;
            sh.smax[j] = (smax_bits && smax_bits[j]) ? smax_bits[j] + k0 : nullptr;
            sh.qbound[j] = (qbounds && qbounds[j]) ? qbounds[j] + k0 * npx : nullptr;
        }
        k_scan_rimg_lds<<<dim3((unsigned)(((nk + 7) / 8) * 8 * (size_t)plan.n_bands)), dim3(kScanLdsThreads), 0, s>>>(scans, offsets_dev, kb + k0, (uint32_t)nk, g, sh);
    }
    return hipGetLastError();
}

// axis-aligned bounds of every 4096-point map tile (map frame): 6 floats per tile {min xyz, max xyz}
__global__ void __launch_bounds__(kBlock)
k_tile_bounds(const float4* __restrict__ map, uint32_t M, float* __restrict__ bounds)
{
    __shared__ float smn[3][kBlock / 64], smx[3][kBlock / 64];
    const uint32_t per_block = (uint32_t)kBlock * 16u;
    const uint32_t base = blockIdx.x * per_block;
    const uint32_t nloc = min(per_block, M - base);
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (uint32_t li = threadIdx.x; li < nloc; li += kBlock) {
        const float4 p = map[base + li];
        mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { mn[d] = fminf(mn[d], __shfl_xor(mn[d], off, 64)); mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], off, 64)); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int d = 0; d < 3; ++d) { smn[d][wave] = mn[d]; smx[d][wave] = mx[d]; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int d = threadIdx.x;
        float a = smn[d][0], b = smx[d][0];
        for (int w = 1; w < kBlock / 64; ++w) { a = fminf(a, smn[d][w]); b = fmaxf(b, smx[d][w]); }
        bounds[6 * (size_t)blockIdx.x + d] = a; bounds[6 * (size_t)blockIdx.x + 3 + d] = b;
    }
}
// bounds of the four 1024-point quarters of every 4096-point tile (24 floats per tile): the occlusion cull's second look (k_pair_shell_select).
// One wavefront per quarter; a quarter beyond the end of the map gets an inverted box (never live).
__global__ void __launch_bounds__(kBlock)
k_subtile_bounds(const float4* __restrict__ map, uint32_t M, float* __restrict__ bounds)
{
    const uint32_t sub = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t base = sub * 1024u;
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (uint32_t li = lane; li < 1024u; li += 64u) {
        if (base + li >= M) break;
        const float4 p = map[base + li];
        mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { mn[d] = fminf(mn[d], __shfl_xor(mn[d], off, 64)); mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], off, 64)); }
    if (lane < 3u) { bounds[6 * (size_t)sub + lane] = mn[lane]; bounds[6 * (size_t)sub + 3 + lane] = mx[lane]; }
}
hipError_t subtile_bounds(const float4* map, size_t M, float* bounds, hipStream_t s)
{
    if (!M) return hipSuccess;
    k_subtile_bounds<<<dim3((unsigned)((M + 4095) / 4096)), dim3(kBlock), 0, s>>>(map, (uint32_t)M, bounds);
    return hipGetLastError();
}
hipError_t tile_bounds(const float4* map, size_t M, float* bounds, hipStream_t s)
{
    if (!M) return hipSuccess;
    const size_t per_block = (size_t)kBlock * 16;
    k_tile_bounds<<<dim3((unsigned)((M + per_block - 1) / per_block)), dim3(kBlock), 0, s>>>(map, (uint32_t)M, bounds);
    return hipGetLastError();
}

// utility.cpp:64-72 + :92-142.  grid = (map tiles, keyframes of the batch)
template <bool B2L_IDENTITY>
__global__ void __launch_bounds__(kBlock)
k_map_rimg(const float4* __restrict__ map, size_t M, const double* __restrict__ inv_poses, size_t kb,
           HostMat34 b2l_h, ProjLaunch pl, uint64_t* __restrict__ img)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const size_t kf = kb + blockIdx.y;
    const Mat34 Tinv = load_mat(inv_poses + 12 * kf);
    const RimgGeom& g = pl.g;
    const float4 p4 = map[i];
    float3 p = xform(Tinv, make_float3(p4.x, p4.y, p4.z));
    if (B2L_IDENTITY) p = xform_identity(p); else p = xform(to_dev(b2l_h), p);
    const Sph s = cart2sph(p.x, p.y, p.z);
    const int px = pixel_index(g, s.az, s.el);
    const uint64_t v = ((uint64_t)f2u(s.r) << 32) | (uint64_t)(uint32_t)i;
    img_min_u64(img + (size_t)blockIdx.y * (size_t)pl.npx + px, v);
}

static constexpr int kPtsPerThread = 16;      // a map tile = kBlock * kPtsPerThread = 4096 consecutive points

hipError_t map_range_images(const float4* map, size_t M, const double* inv_poses_dev, const float* approx_poses_dev, size_t kb, size_t nb,
                            HostMat34 b2l, int b2l_identity, Geom g, uint64_t* map_img, hipStream_t s, const KernelOpts& ko);

// ---------------------------------------------------------------------------------------------------------------
// Range-culled vote kernel (mode 0: diff = scan - map).  A map point P can influence the labels only if it could be
// flagged in its own pixel, i.e. fl(scan[px(P)] - r_P) > thr: if it cannot, then (a) it is not flagged itself, and
// (b) removing it from the arg-min competition changes nothing -- whoever wins instead is at least as far, so that
// pixel stays unflagged; and any flagged winner is nearer than P, so P never displaces it.  The scan images are
// complete before this kernel runs, so the test needs no inter-workgroup ordering.
// Phase 1 (every point): exact fp64 transform, then a bounded-error projection (atan2 within 3e-6 rad, native
// sqrt) gives the pixel up to +-Geom::cull_eps_px; the point survives if for ANY candidate pixel the scan range exceeds a
// lower bound of its range by more than thr minus a margin (or if it is in a domain the fast forms do not cover).
// Survivors (typically 10-20 %) are queued in LDS.  Phase 2: survivors get the exact arithmetic and go through the
// workgroup's pixel table ("building blocks" below: ballot4, drain_segment, exact_tiles, uncertain_tail, table_*).  Labels are identical to the un-culled path (parity tests); the map image is
// not (culled points are absent), which is why ltm_debug_range_image / reprojection / mode 1 use k_map_rimg_lds.

// rb/cb: the pixel if it is certain; multi: within cull_eps_px of a rounding boundary (candidates r0..r1 x c0..c1, filled by
// cull_expand); r2: squared range of the approximate local point -- the exact range r_e satisfies r_e^2 in r2 * [1 - 3e-6, 1 + 3e-6]
// (validated on the device by ltm_debug_cull_check); unusual: outside the fast forms' domain
struct CullCand { int rb, cb, r0, r1, c0, c1; float rowh, colh, r2; bool multi, unusual; };

// p' = A (p - c): the inverse pose (composed with base->lidar) rewritten around the sensor position c so that the
// subtraction happens between nearby numbers; c is carried as a float-float pair (c_hi, c_lo) and the tiny constant
// -A c_lo is precomputed per keyframe (ap[12..14]) and enters through the first FMA of each row.  Relative error of p'
// <= 5e-7 (binary32 roundings only), i.e. <= 5e-7 rad of direction error at any range.  16 floats per keyframe.
__device__ __forceinline__ float3 xform_approx(const float* __restrict__ ap, float4 p4, bool& ok)
{
    const float dx = p4.x - ap[9], dy = p4.y - ap[10], dz = p4.z - ap[11];
    ok = ap[15] != 0.0f;
    float3 o;
    o.x = __builtin_fmaf(ap[2], dz, __builtin_fmaf(ap[1], dy, __builtin_fmaf(ap[0], dx, ap[12])));
    o.y = __builtin_fmaf(ap[5], dz, __builtin_fmaf(ap[4], dy, __builtin_fmaf(ap[3], dx, ap[13])));
    o.z = __builtin_fmaf(ap[8], dz, __builtin_fmaf(ap[7], dy, __builtin_fmaf(ap[6], dx, ap[14])));
    return o;
}

// steep_clamps: the field of view is narrow enough (vfov/2 < 44 deg) that every elevation beyond +-45 deg clamps into the first /
// last row whatever its value, so the elevation polynomial only ever sees |z| / rxy <= 1 (one v_rsq instead of v_sqrt + v_rcp and
// no octant select); with a wider vertical field of view the steep points take the exact path instead.
// EL3: the field of view is narrow enough for the fitted degree-3 elevation polynomial (Geom::el_fit, two FMAs fewer and ~2x more
// accurate than the generic one on [0, 1]); then elevations beyond the clamp need no special case at all.
// (Tried: packed v_pk_* evaluation of the two polynomials -- no gain on gfx950, where v_pk_fma_f32 issues at half the rate of
// v_fma_f32, tools/ubench/valu_rate.hip.)
template <bool EL3 = false>
__device__ __forceinline__ CullCand cull_candidates(const ProjLaunch& pl, float3 p)
{
    const RimgGeom& g = pl.g;
    CullCand cc;
    const float xy2 = __builtin_fmaf(p.x, p.x, p.y * p.y);
    cc.r2 = __builtin_fmaf(p.z, p.z, xy2);
    const float inv_rxy = __builtin_amdgcn_rsqf(xy2);
    const float t_el = fabsf(p.z) * inv_rxy;                                  // tan |elevation|
    // azimuth, reduced to the first octant: min(|x|, |y|) / rxy is its sine (no reciprocal of max(|x|, |y|) needed)
    const float ax = fabsf(p.x), ay = fabsf(p.y);
    const float az_oct = asin_octant_approx(fminf(ax, ay) * inv_rxy);
    float el_abs;
    if (EL3) {
        const float t = fminf(t_el, g.el_tclamp), u = t * t;
        el_abs = t * __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(g.el_c3, u, g.el_c2), u, g.el_c1), u, g.el_c0);
    } else {
        el_abs = atan_unit_approx(fminf(t_el, 1.0f));
    }
    const float el = __builtin_copysignf(el_abs, p.z);
    float az = (ay > ax) ? (1.57079632679f - az_oct) : az_oct;
    az = (p.x < 0.0f) ? (3.14159265359f - az) : az;
    az = __builtin_copysignf(az, p.y);          // az >= 0: one v_bfi instead of compare + select
    // rowf = R*(1 - (el_deg + V/2)/V) = R/2 - el*(R*180/(pi*V)) ; colf = C*((az_deg + H/2)/H) = C/2 + az*(C*180/(pi*H)).
    // rowh = rowf + 0.5 - eps: floor(rowf + 0.5) is the rounded pixel, and with the band half-width eps taken off up front
    //   fract(rowh) < 1 - 2 eps  <=>  fract(rowf + 0.5) in [eps, 1 - eps)  <=>  the pixel is certain, and then floor(rowh) is that pixel
    // (one fract and one compare per axis instead of a two-sided test; the sign of el sits on the uniform factor).
    cc.rowh = __builtin_fmaf(el, -pl.row_scale, pl.row_bias);
    cc.colh = __builtin_fmaf(az, pl.col_scale, pl.col_bias);
    const bool certain = fmaxf(__builtin_amdgcn_fractf(cc.rowh), __builtin_amdgcn_fractf(cc.colh)) < pl.certain_lim;
    // Outside the fast forms' domain (every such case ends in the exact path):
    //  - the +-180 deg seam -- the SIGN of y picks column 0 or C-1 there, and the approximate y is only good to ~1e-7 of the range,
    //    so x < 0 with |y| <= 1e-6 |x| is undecidable here (y == +-0 included); the same test catches vanishing x and y (the squares
    //    would underflow and 0 * rsq(0) makes a NaN azimuth);
    //  - r >= 8000 m (inf included): the reference's "empty pixel = 10000 m" sentinel arithmetic (diff = 10000 - r,
    //    Removerter.cpp:398-404) flags a map point 9800..9999.9 m from the sensor on an EMPTY scan pixel, which the fast test (empty
    //    pixels never flag) would drop;
    //  - steep elevations when the field of view does not clamp them.
    // A NaN coordinate needs no guard: its range is NaN, `r < rimg` is false in the reference (utility.cpp:134), so the point never
    // wins a pixel -- and here r2 = NaN fails both compares below and the caller's r2 < qbound, so it is dropped, which is the same.
    cc.unusual = (fabsf(p.y) <= __builtin_fmaf(-1.0e-6f, p.x, 1.0e-18f)) | (cc.r2 > 6.4e7f);
    if (!EL3) cc.unusual |= !pl.steep_clamps & (t_el > 1.0f);
    cc.multi = !certain;
    // clamp(floor(v), 0, n-1) == trunc(med3(v, 0, n-1)): the bounds are integers and the clamped value is non-negative
    cc.rb = (int)__builtin_amdgcn_fmed3f(cc.rowh, 0.0f, g.row_max);
    cc.cb = (int)__builtin_amdgcn_fmed3f(cc.colh, 0.0f, g.col_max);
    cc.r0 = cc.r1 = cc.rb; cc.c0 = cc.c1 = cc.cb;
    return cc;
}

// lower bound of the exact range from the squared approximate range (native sqrt, 1 ulp): upper bound = r_lo * (1 + 3e-6)
__device__ __forceinline__ float cull_r_lo(float r2) { return __builtin_amdgcn_sqrtf(r2) * (1.0f - 1.5e-6f); }

// candidate pixel rectangle of a point that sits within cull_eps_px of a rounding boundary (rare)
__device__ __forceinline__ void cull_expand(const ProjLaunch& pl, CullCand& cc)
{
    const RimgGeom& g = pl.g;
    // rowh / colh carry the -eps shift of cull_candidates: a fraction >= 1 - 2 eps means the unshifted value is within eps of the
    // integer above floor(rowh) -- either pixel floor(rowh) or floor(rowh) + 1
    const float rfl = floorf(cc.rowh), cfl = floorf(cc.colh);
    const float rfr = cc.rowh - rfl, cfr = cc.colh - cfl;
    const int rc = (int)rfl, ccn = (int)cfl;
    const int rmax = g.rows - 1, cmax = g.cols - 1;
    const float lim = pl.certain_lim;
    cc.r0 = min(max(rc, 0), rmax);
    cc.r1 = min(max(rc + (rfr >= lim ? 1 : 0), 0), rmax);
    cc.c0 = min(max(ccn, 0), cmax);
    cc.c1 = min(max(ccn + (cfr >= lim ? 1 : 0), 0), cmax);
}

// With a non-identity base->lidar extrinsic the exact path rounds to float between the two transforms (utility.cpp:70-71), i.e.
// at magnitude range + lever arm; relative to a range much smaller than the lever arm that rounding exceeds the validated bounds
// of the approximate projection, so points nearer than lever/8 take the exact path (none with an identity extrinsic):
// ProjLaunch::rmin2 = (0.125 |t| + 1e-6)^2 of the extrinsic's translation t (make_proj_launch).

__device__ unsigned long long g_cull_stats[4];   // {survivors, points} of k_vote_map_cull, then of k_map_rimg_blockmin: diagnostic, read by cull_stats()

static constexpr int kCullQueue = 2048;   // survivor queue capacity: four wave-private segments in k_vote_map_cull (drained before they can overflow); one queue per tile in k_map_rimg_blockmin (~370 of 4096 expected, overflow sends the whole tile down the exact path)

// ---------------------------------------------------------------------------------------------------------------
// Building blocks of the tile pipelines (k_map_rimg_lds, k_vote_map_cull, k_map_rimg_blockmin, k_map_rimg_blockmin_run).  The kernels differ in what they select
// and in their control flow; what reaches an image always comes from exact_insert / exact_range_insert and leaves through table_min / table_flush.
// Direct-mapped pixel table of a workgroup in LDS: ROWS x COLS slots, slot = low bits of row / column, tags[slot] = the pixel that owns the slot (first
// come), vals[slot] = the minimum of the 64-bit (range bits << 32 | point index) words of that pixel so far; the exact-image pre-filter keeps a third
// array beside them, amin[slot] = float bits of the smallest range upper bound published for the pixel (publish_bound).  table_init: pass null for an
// array that the caller does not (re)initialise.
static constexpr uint32_t kEmptyTag = 0xffffffffu;
template <int SLOTS>
__device__ __forceinline__ void table_init(uint32_t* __restrict__ tags, uint64_t* __restrict__ vals, uint32_t* __restrict__ amin)
{
    for (int s = threadIdx.x; s < SLOTS; s += kBlock) {
        if (tags) tags[s] = kEmptyTag;
        if (amin) amin[s] = 0x7f800000u;      // +inf
        if (vals) vals[s] = ~0ull;
    }
}
// Returns the slot if `px` owns it, or -1 (then the caller goes to the global image).  A slot never changes owner.
// (Tried: a second chance in the (ROWS/2) x (2 COLS) cut of the coordinates.  It turns ~7 % of misses into ~2 % on octree-ordered
// map tiles, but the extra probe costs as much as the saved global atomics: no change in either kernel.)
template <int ROWS, int COLS>
__device__ __forceinline__ int table_claim(uint32_t* __restrict__ tags, int row, int col, uint32_t px)
{
    const int slot = ((row & (ROWS - 1)) * COLS) | (col & (COLS - 1));
    uint32_t t = tags[slot];
    if (t == kEmptyTag) {
        const uint32_t old = atomicCAS(&tags[slot], kEmptyTag, px);
        t = (old == kEmptyTag) ? px : old;
    }
    return (t == px) ? slot : -1;
}
// v into the minimum of pixel px: through the table if the pixel owns its slot, else straight to the global image.  uint64 min is associative,
// commutative and idempotent, so the final image does not depend on which way a word takes, on the order, or on a word arriving twice.
template <int ROWS, int COLS>
__device__ __forceinline__ void table_min(uint64_t* __restrict__ vals, uint32_t* __restrict__ tags, uint64_t* __restrict__ imgk, int row, int col, uint32_t px,
                                          uint64_t v)
{
    const int slot = table_claim<ROWS, COLS>(tags, row, col, px);
    // vals only decreases: skip hopeless same-address atomics.  (Workgroup scope is all an LDS word needs, and it keeps the compiler from folding this
    // atomic and the image's into one flat instruction on a selected address.)
    if (slot >= 0) { if (v < vals[slot]) __hip_atomic_fetch_min(&vals[slot], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    else img_min_u64(imgk + px, v);
}
// One global atomic per touched pixel leaves the CU.  In the exact-image pre-filter a slot is claimed in phase 1a and may never get a word (its points
// were all dropped): a slot that still holds all ones is skipped.  A minimum with all ones changes nothing in the image, so the test is only a saving
// there and is harmless in the two kernels whose claimed slots always hold a word.
template <int SLOTS>
__device__ __forceinline__ void table_flush(const uint32_t* __restrict__ tags, const uint64_t* __restrict__ vals, uint64_t* __restrict__ imgk)
{
    for (int s = threadIdx.x; s < SLOTS; s += kBlock) {
        const uint32_t t = tags[s];
        if (t != kEmptyTag && vals[s] != ~0ull) img_min_u64(imgk + t, vals[s]);
    }
}
// exact projection of one map point into image `imgk`, reduced through the workgroup's LDS table
template <bool B2L_IDENTITY, int ROWS, int COLS>
__device__ __forceinline__ void exact_insert(const float4* __restrict__ map, uint32_t i, const Mat34& Tinv, const HostMat34& b2l_h, const RimgGeom& g,
                                             uint64_t* __restrict__ vals, uint32_t* __restrict__ tags, uint64_t* __restrict__ imgk)
{
    const float4 p4 = map[i];
    float3 p = xform(Tinv, make_float3(p4.x, p4.y, p4.z));
    if (B2L_IDENTITY) p = xform_identity(p); else p = xform(to_dev(b2l_h), p);
    const Sph s = cart2sph(p.x, p.y, p.z);
    int row, col;
    pixel_row_col(g, s.az, s.el, row, col);
    table_min<ROWS, COLS>(vals, tags, imgk, row, col, (uint32_t)(row * g.cols + col), ((uint64_t)f2u(s.r) << 32) | (uint64_t)i);
}
// Exact range of a map point whose pixel is already certain (single candidate of the bounded-error projection, which
// ltm_debug_cull_check validates to contain the exact pixel): the reference arithmetic up to sqrtf only --
// r = sqrtf((x*x + y*y) + z*z) on the float-rounded fp64 transform -- without the atan2f / rad2deg / pixel chain.
template <bool B2L_IDENTITY>
__device__ __forceinline__ uint32_t exact_range_bits(const float4 p4, const Mat34& Tinv, const HostMat34& b2l_h)
{
    float3 p = xform(Tinv, make_float3(p4.x, p4.y, p4.z));
    if (B2L_IDENTITY) p = xform_identity(p); else p = xform(to_dev(b2l_h), p);
    const float xy = p.x * p.x + p.y * p.y;
    return f2u(__builtin_sqrtf(xy + p.z * p.z));
}
// ... and into the minimum of that pixel
template <bool B2L_IDENTITY, int ROWS, int COLS>
__device__ __forceinline__ void exact_range_insert(const float4* __restrict__ map, uint32_t i, int row, int col, uint32_t px, const Mat34& Tinv,
                                                   const HostMat34& b2l_h, uint64_t* __restrict__ vals, uint32_t* __restrict__ tags, uint64_t* __restrict__ imgk)
{
    table_min<ROWS, COLS>(vals, tags, imgk, row, col, px, ((uint64_t)exact_range_bits<B2L_IDENTITY>(map[i], Tinv, b2l_h) << 32) | (uint64_t)i);
}
// Queue positions of a group of four points per lane, of which m[u] says which ones are queued: four ballots and their popcounts on the scalar unit,
// nothing shared with another wave.  The wave's entries of the group are dense and ordered by (u, lane); the caller supplies the base (a count it
// keeps in a scalar register, or one LDS atomic per wave and group), decides what happens when base + total does not fit, and stores its word at
// base + ballot4_pos(q, u) for every m[u].  (Letting the compiler aggregate four separate atomicAdd(&count, 1) costs ~40 instructions each.)
struct Ballot4 { uint64_t b[4]; uint32_t total; };
__device__ __forceinline__ Ballot4 ballot4(const bool (&m)[4])
{
    Ballot4 q;
#pragma unroll
    for (int u = 0; u < 4; ++u) q.b[u] = __builtin_amdgcn_ballot_w64(m[u]);
    q.total = (uint32_t)__popcll(q.b[0]) + (uint32_t)__popcll(q.b[1]) + (uint32_t)__popcll(q.b[2]) + (uint32_t)__popcll(q.b[3]);
    return q;
}
__device__ __forceinline__ uint32_t ballot4_pos(const Ballot4& q, int u)
{
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) before += (w < u) ? (uint32_t)__popcll(q.b[w]) : 0u;
    return before + __builtin_amdgcn_mbcnt_hi((uint32_t)(q.b[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)q.b[u], 0u));
}
// Phase 2 of k_vote_map_cull, by wave: the exact range of the nq survivors queued in the wave's own segment `seg`, 64 per iteration, all lanes active.
// The word is ltm_kernels_common.h's ( tile in run 4 bits | group 4 | lane 6 | pixel 18; the wave is implied).  Pixel all ones = not
// certain: the point takes a ticket for the run's shared uqueue (UQ entries of (tile in run) << 12 | tile-local index, served behind the run by
// uncertain_tail); a ticket past the capacity is served on the spot.  No barrier: min is idempotent, a superset of survivors is correct, and the table
// is touched through LDS atomics and reads that tolerate staleness only.  (k_map_rimg_blockmin_run has its own copy, `drain`: NOTEBOOK 4.1.)
template <bool B2L_IDENTITY, int ROWS, int COLS, int UQ>
__device__ __forceinline__ void drain_segment(const uint32_t* __restrict__ seg, uint32_t nq, const float4* __restrict__ map, uint32_t run_base,
                                              const double* __restrict__ inv_pose, const HostMat34& b2l_h, const ProjLaunch& pl, uint64_t* __restrict__ vals,
                                              uint32_t* __restrict__ tags, uint64_t* __restrict__ imgk, uint16_t* __restrict__ uqueue, uint32_t* __restrict__ ucount)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the segment's words were written by other lanes of this wave
    const Mat34 Tinv = load_mat(inv_pose);
    for (uint32_t q = threadIdx.x & 63u; q < nq; q += 64u) {
        const uint32_t e = seg[q];
        const uint32_t off = ((e >> 24) << 8) | (threadIdx.x & 192u) | ((e >> kVoteQueuePxBits) & 63u);
        const uint32_t px = e & kVoteQueuePxUncertain;
        if (px == kVoteQueuePxUncertain) {
            const uint32_t ticket = atomicAdd(ucount, 1u);
            if (ticket < (uint32_t)UQ) uqueue[ticket] = (uint16_t)off;
            else exact_insert<B2L_IDENTITY, ROWS, COLS>(map, run_base + off, Tinv, b2l_h, pl.g, vals, tags, imgk);
            continue;
        }
        uint32_t row, col;
        vote_queue_row_col(px, (uint32_t)pl.g.cols, pl.px_magic, pl.px_shift, row, col);
        exact_range_insert<B2L_IDENTITY, ROWS, COLS>(map, run_base + off, (int)row, (int)col, px, Tinv, b2l_h, vals, tags, imgk);
    }
    // The drain's image atomics retire here.  The vector memory counter also counts them, and they may retire out of order with loads: with
    // some still in flight every wait for a point of phase 1 would have to be a wait for ALL loads in flight, the prefetched ones included.
    __builtin_amdgcn_s_waitcnt(0x0f70);      // vmcnt(0) only
}
// The uncertain-pixel survivors of a whole run, by all 256 threads, behind the barrier that makes ucount and uqueue final
template <bool B2L_IDENTITY, int ROWS, int COLS, int UQ>
__device__ __forceinline__ void uncertain_tail(const uint16_t* __restrict__ uqueue, uint32_t ucount, const float4* __restrict__ map, uint32_t run_base,
                                               const double* __restrict__ inv_pose, const HostMat34& b2l_h, const RimgGeom& g, uint64_t* __restrict__ vals,
                                               uint32_t* __restrict__ tags, uint64_t* __restrict__ imgk)
{
    const uint32_t nu = min(ucount, (uint32_t)UQ);
    if (!nu) return;
    const Mat34 Tinv = load_mat(inv_pose);
    for (uint32_t q = threadIdx.x; q < nu; q += kBlock)
        exact_insert<B2L_IDENTITY, ROWS, COLS>(map, run_base + uqueue[q], Tinv, b2l_h, g, vals, tags, imgk);
}
// The tiles of k_vote_map_cull's run that are not on the fast path (bit t of `tiles` = tile first_tile + t: the partial last tile of the map, a shape the
// queue word does not hold, a keyframe without a usable approximate pose): every point takes the exact projection, each thread its own, no barrier.
// Returns the statistics line: a full tile down the exact path counts every point as a survivor (per wave).
template <bool B2L_IDENTITY, int ROWS, int COLS>
__device__ __forceinline__ uint32_t exact_tiles(uint32_t tiles, uint32_t first_tile, const float4* __restrict__ map, uint32_t M, const double* __restrict__ inv_pose,
                                                const HostMat34& b2l_h, const RimgGeom& g, uint64_t* __restrict__ vals, uint32_t* __restrict__ tags,
                                                uint64_t* __restrict__ imgk)
{
    const uint32_t per_block = (uint32_t)(kBlock * kPtsPerThread);
    const Mat34 Tinv = load_mat(inv_pose);
    uint32_t nsurv = 0;
    for (; tiles; tiles &= tiles - 1u) {
        const uint32_t block_base = (first_tile + (uint32_t)__builtin_ctz(tiles)) * per_block;
        const uint32_t nloc = min(per_block, M - block_base);
        for (uint32_t li = threadIdx.x; li < nloc; li += kBlock)
            exact_insert<B2L_IDENTITY, ROWS, COLS>(map, block_base + li, Tinv, b2l_h, g, vals, tags, imgk);
        if (nloc == per_block) nsurv += per_block / (kBlock / 64);
    }
    return nsurv;
}
// Phase 1a of the exact-image pre-filter, one point.  pixel_certain: the bounded-error projection has one candidate pixel and the point is inside the
// fast forms' domain.  publish_bound: such a point, if its pixel px owns its table slot, publishes an UPPER bound of its exact range into amin[slot],
// puts the slot into its record (rec |= slot << SLOT_SHIFT; each kernel packs the pixel below that in its own way) and returns the LOWER bound of
// its range.  Every other point returns -1, which no table entry can beat -- it survives unconditionally -- and keeps a slot field of 0, any valid
// index, so that phase 1b can read amin without a branch.
__device__ __forceinline__ bool pixel_certain(const ProjLaunch& pl, const CullCand& cc) { return !cc.unusual & !cc.multi & !(cc.r2 < pl.rmin2); }
template <int ROWS, int COLS, int SLOT_SHIFT>
__device__ __forceinline__ float publish_bound(const CullCand& cc, bool certain, uint32_t px, uint32_t* __restrict__ tags, uint32_t* __restrict__ amin, uint32_t& rec)
{
    const float r_lo = cull_r_lo(cc.r2);
    if (!certain) return -1.0f;
    const int slot = table_claim<ROWS, COLS>(tags, cc.rb, cc.cb, px);
    if (slot < 0) return -1.0f;                                    // slot owned by another pixel
    rec |= (uint32_t)slot << SLOT_SHIFT;
    // upper bound of the exact range: r_e <= r_lo (1 + 3e-6) (k_cull_check) and a rounding.  amin only ever decreases, so a plain read that is
    // already smaller makes the (same-address, hence serialised) atomic unnecessary for most points of a pixel
    const uint32_t hi = f2u(r_lo * (1.0f + 3.5e-6f));
    if (hi < amin[slot]) atomicMin(&amin[slot], hi);
    return r_lo;
}
// The <B2L_IDENTITY, EL3> instantiation of a kernel template for a launch (identity extrinsic; fitted elevation polynomial, see cull_candidates)
#define LTM_LAUNCH_ID_EL3(KERNEL, IDENT, EL3, GRID, STREAM, ...)                                                                                                       \
    do { if (IDENT) { if (EL3) KERNEL<true, true><<<GRID, dim3(kBlock), 0, STREAM>>>(__VA_ARGS__); else KERNEL<true, false><<<GRID, dim3(kBlock), 0, STREAM>>>(__VA_ARGS__); } \
         else { if (EL3) KERNEL<false, true><<<GRID, dim3(kBlock), 0, STREAM>>>(__VA_ARGS__); else KERNEL<false, false><<<GRID, dim3(kBlock), 0, STREAM>>>(__VA_ARGS__); }   \
    } while (0)

// Same contract as k_map_rimg, with a per-workgroup LDS pre-reduction.  Map points are stored in octree (Morton)
// order, so the 4096 consecutive points of a workgroup cover a compact patch of the range image and many of
// them share a pixel: they are first min-reduced in a 16 x 128-slot table (building blocks above), so the final image is
// identical to the serial reference result.
// (the XCD-aware workgroup -> (map tile, keyframe) mapping, tile_kf_of_block, is in ltm_kernels_common.h)
static constexpr int kLdsSlots = 2048;
template <bool B2L_IDENTITY>
__global__ void __launch_bounds__(kBlock)
k_map_rimg_lds(const float4* __restrict__ map, uint32_t M, const double* __restrict__ inv_poses, uint32_t kb, uint32_t nb,
               HostMat34 b2l_h, ProjLaunch pl, uint64_t* __restrict__ img)
{
    __shared__ uint64_t vals[kLdsSlots];
    __shared__ uint32_t tags[kLdsSlots];
    const uint32_t per_block = (uint32_t)(kBlock * kPtsPerThread);
    const TileKf tk = tile_kf_of_block(blockIdx.x, pl, nb);
    if (!tk.valid) return;
    table_init<kLdsSlots>(tags, vals, nullptr);
    __syncthreads();
    const uint32_t block_base = tk.tile * per_block;
    const uint32_t nloc = min(per_block, M - block_base);
    const Mat34 Tinv = load_mat(inv_poses + 12 * (size_t)(kb + tk.kfb));
    uint64_t* __restrict__ imgk = img + (size_t)tk.kfb * pl.npx;
#pragma unroll 2
    for (uint32_t li = threadIdx.x; li < nloc; li += kBlock)
        exact_insert<B2L_IDENTITY, 16, 128>(map, block_base + li, Tinv, b2l_h, pl.g, vals, tags, imgk);
    __syncthreads();
    table_flush<kLdsSlots>(tags, vals, imgk);
}

// Whole-tile range cull: no point of a tile can be nearer to the sensor than the distance from the sensor position to the tile's
// bounding box; if that already exceeds the keyframe's longest scan return (minus thr, with margins for a slightly
// non-orthonormal pose and float rounding) nothing there can be flagged and the workgroup is done.
// ap = the keyframe's approximate pose (16 floats), tb = {min xyz, max xyz} of the tile, smax = longest non-empty scan return.
__device__ __forceinline__ bool tile_out_of_reach(const float* __restrict__ ap, const float* __restrict__ tb, float smax, float thr)
{
    float d2 = 0.0f, far2 = 0.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float c = ap[9 + d];                            // sensor position to ~1e-5 m: the margins below are 1e-2
        const float lo = tb[d] - c, hi = c - tb[3 + d];
        const float e = fmaxf(fmaxf(lo, hi), 0.0f);          // distance to the box along this axis
        const float f = fmaxf(fabsf(lo), fabsf(hi));          // distance to its farthest face
        d2 = __builtin_fmaf(e, e, d2);
        far2 = __builtin_fmaf(f, f, far2);
    }
    // exact local range of any point of the tile: |A (p - c)| >= smin * |p - c| >= smin * dist(c, box); ap[15] = lower bound of smin
    const float smin = ap[15];
    const float reach = fmaxf(smax - thr, 0.0f) + 1.0e-2f + smax * 1.0e-3f;
    // far2 guard: beyond ~8.9 km the reference's "empty pixel = 10000" sentinel arithmetic could flag a point; never cull there
    return smin > 0.5f && far2 < 8.0e7f && d2 * smin * smin * 0.996f > reach * reach;
}

// number of (tile, keyframe) workgroups of a k_vote_map_cull launch that survive the whole-tile cull (measurement only: the
// algorithmic bytes of a launch count the map tiles that are actually read)
__global__ void __launch_bounds__(kBlock)
k_count_live_tiles(const float* __restrict__ approx_poses, uint32_t kb, uint32_t nb, const float* __restrict__ tile_bounds, uint32_t n_tiles,
                   const uint32_t* __restrict__ smax_bits, float thr, unsigned long long* __restrict__ live)
{
    const uint32_t tile = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t kfb = blockIdx.y;
    bool alive = false;
    if (tile < n_tiles) alive = !tile_out_of_reach(approx_poses + 16 * (size_t)(kb + kfb), tile_bounds + 6 * (size_t)tile, u2f(smax_bits[kfb]), thr);
    __shared__ uint32_t wsum[kBlock / 64];
    const uint64_t b = __builtin_amdgcn_ballot_w64(alive);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {         // one atomic per workgroup
        uint32_t t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += wsum[w];
        if (t) atomicAdd(live, (unsigned long long)t);
    }
}
hipError_t count_live_tiles(const float* approx_poses_dev, size_t kb, size_t nb, const float* tile_bounds_dev, size_t n_tiles,
                            const uint32_t* smax_bits_dev, float thr, unsigned long long* live_dev, hipStream_t s)
{
    if (!nb || !n_tiles) return hipSuccess;
    k_count_live_tiles<<<dim3(grid_for(n_tiles), (unsigned)nb), dim3(kBlock), 0, s>>>(approx_poses_dev, (uint32_t)kb, (uint32_t)nb, tile_bounds_dev,
                                                                                    (uint32_t)n_tiles, smax_bits_dev, thr, live_dev);
    return hipGetLastError();
}

static constexpr int kCullSlots = 512;   // survivors are ~10 % of a workgroup's points: a small LDS table keeps 8 workgroups per CU

template <bool B2L_IDENTITY, bool EL3>     // EL3: fitted elevation polynomial (Geom::el_fit), see cull_candidates
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
k_vote_map_cull(const float4* __restrict__ map, uint32_t M, const double* __restrict__ inv_poses, const float* __restrict__ approx_poses,
                uint32_t kb, uint32_t nb, HostMat34 b2l_h, ProjLaunch pl, RunLaunch rl, const float* __restrict__ qbound_img,
                const float* __restrict__ tile_bounds, const uint32_t* __restrict__ smax_bits, float thr, uint64_t* __restrict__ img)
{
    __shared__ uint64_t vals[kCullSlots];
    __shared__ uint32_t tags[kCullSlots];
    // Survivors of phase 1, one word each (ltm_kernels_common.h: tile in run 4 bits | group 4 | lane 6 | pixel 18, pixel all ones = not certain, needs the full
    // exact projection).  Four wave-private segments: wave w fills and drains queue[w * kSeg .. (w + 1) * kSeg) and counts its entries in a scalar register.
    __shared__ uint32_t queue[kCullQueue];
    // the uncertain ones of the whole run, re-queued densely by the drains: (tile in run) << 12 | tile-local index = the offset from the run's first point.
    // Shared by the four waves; a ticket past the capacity is served on the spot.
    __shared__ uint16_t uqueue[kCullQueue];
    __shared__ uint32_t ucount;
    static_assert(kMaxTileRun * kBlock * kPtsPerThread <= 65536, "uqueue entries are 16 bits");
    static_assert(kMaxTileRun <= 16 && kPtsPerThread == 16 && kBlock == 256, "queue word: 4 bits of tile, 4 of group, 6 of lane; the wave is implied");
    constexpr int kInFlight = 4;
    constexpr uint32_t kSeg = (uint32_t)kCullQueue / (kBlock / 64);      // 512 entries per wave
    constexpr uint32_t kDrainAt = kSeg - 64u * kInFlight;                  // a group of kInFlight points per lane adds at most 64 * kInFlight
    const uint32_t per_block = (uint32_t)(kBlock * kPtsPerThread);
    // One workgroup = a run of rl.T consecutive tiles against one keyframe.  Whatever depends on the keyframe only -- pose, image bases, the pixel
    // table and its flush -- happens once per run.  The waves share the pixel table only: each walks its own quarter of every tile (lanes 64 w .. 64 w + 63
    // of each group of 256 points) through all tiles of the run as one pipelined stream, and gives its survivors their exact range whenever its segment fills.
    const RunKf rk = run_kf_of_block(blockIdx.x, rl, nb);
    if (!rk.valid) return;
    const RimgGeom& g = pl.g;
    const uint32_t npx = pl.npx;
    const uint32_t kf = kb + rk.kfb;
    const uint32_t first_tile = rk.run * rl.T;
    const uint32_t run_base = first_tile * per_block;
    uint64_t* __restrict__ imgk = img + (size_t)rk.kfb * npx;
    const float* __restrict__ qk = qbound_img + (size_t)rk.kfb * npx;
    const float* __restrict__ ap = approx_poses + 16 * (size_t)kf;
    // The reach test of all tiles of the run at once: lane t of every wave tests tile t, and the ballot -- the same in every wave -- is the set of
    // tiles to visit.
    uint32_t todo;
    {
        const uint32_t t = threadIdx.x & 63u;
        bool visit = (t < rl.T) & (first_tile + t < pl.n_tiles);
        if (visit && tile_bounds) visit = !tile_out_of_reach(ap, tile_bounds + 6 * (size_t)(first_tile + t), u2f(smax_bits[rk.kfb]), thr);
        todo = (uint32_t)__builtin_amdgcn_ballot_w64(visit);
    }
    if (!todo) return;
    table_init<kCullSlots>(tags, vals, nullptr);
    if (threadIdx.x == 0) ucount = 0;
    __syncthreads();      // the only barrier in front of the exact-projection tail: from here to there no wave waits for another
    // Fast path: every full tile, if the image's pixels fit the queue word and the keyframe's approximate pose is usable (ap[15] != 0.0f, as an integer test:
    // the scalar unit has no float compare).  The one partial tile at the end of the map takes the exact path as a whole, which keeps bounds tests and clamped
    // indices out of the stream.
    uint32_t full = todo;
    {
        const uint32_t t_last = pl.n_tiles - 1u - first_tile;
        if (t_last < kMaxTileRun && (M & (per_block - 1u)) != 0u) full &= ~(1u << t_last);
    }
    const uint32_t fast = (pl.vote_queueable & ((f2u(ap[15]) << 1) != 0u)) ? full : 0u;
    const uint32_t slow = todo & ~fast;
    // statistics, sampled 1/64 (same-address atomics from every workgroup would serialise the grid): the points of the run's full tiles here, the queued
    // survivors per wave behind the stream
    const bool sampled = (blockIdx.x & 63u) == 0u;
    if (sampled && threadIdx.x == 0) atomicAdd(&g_cull_stats[1], (unsigned long long)((uint32_t)__popc(full) * per_block));
    const double* __restrict__ inv_pose = inv_poses + 12 * (size_t)kf;      // (loaded where the exact arithmetic starts: 24 scalar registers that phase 1 has no room for)
    const float4* __restrict__ mapr = map + run_base;
    uint32_t* __restrict__ seg = queue + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * kSeg;
    const uint32_t lane = threadIdx.x & 63u;
    // ---- the stream.  G counts groups of 4 x 256 points from the run's first point: tile in run = G >> 2, the lane's points of group G are
    // mapr[G * 1024 + u * 256 + threadIdx.x], u = 0..3, and (G << 2 | u) is the tile and group field of the queue word.  Everything the loop carries is uniform.
    bool more = fast != 0u;
    uint32_t G = 0, rest = 0, nq = 0, nsurv = 0;
    float4 nxt[kInFlight];
    if (more) {
        G = (uint32_t)__builtin_ctz(fast) << 2;
        rest = fast & (fast - 1u);
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) nxt[u] = mapr[(G << 10) + (uint32_t)u * kBlock + threadIdx.x];
    }
    for (;;) {
        // ---- phase 2, by wave: taken when another group could overflow the segment, and once behind the last group; the prefetched points are requested again
        if (__builtin_expect((nq > kDrainAt) | !more, 0)) {
            drain_segment<B2L_IDENTITY, 8, 64, kCullQueue>(seg, nq, map, run_base, inv_pose, b2l_h, pl, vals, tags, imgk, uqueue, &ucount);
            nsurv += nq;
            nq = 0;
            if (more) {
#pragma unroll
                for (int u = 0; u < kInFlight; ++u) nxt[u] = mapr[(G << 10) + (uint32_t)u * kBlock + threadIdx.x];
            }
        }
        if (!more) break;
        // ---- phase 1: who can matter?  (bounded-error arithmetic only).  Four points per lane are in flight at once so the dependent scan-image load
        // of one overlaps the arithmetic of the others, and the next group's points -- of the next tile to visit, behind a tile's last group -- are
        // requested before this group's arithmetic.
        float4 pt[kInFlight];
        CullCand cc[kInFlight];
        float q0[kInFlight];
        uint32_t pxi[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) pt[u] = nxt[u];
        float3 p[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            bool ok;      // (uniform, part of the fast-path condition)
            p[u] = xform_approx(ap, pt[u], ok);
        }
        // (the request goes out behind the last use of this group's coordinates: their registers take the next group's, and no copy is needed.  Behind
        // the last group of the run the same group is requested once more and dropped: cheaper than a request under a condition, which costs the copies.)
        const uint32_t Gcur = G;
        if ((G & 3u) != 3u) ++G;
        else if (rest) { G = (uint32_t)__builtin_ctz(rest) << 2; rest &= rest - 1u; }
        else more = false;
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) nxt[u] = mapr[(G << 10) + (uint32_t)u * kBlock + threadIdx.x];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            cc[u] = cull_candidates<EL3>(pl, p[u]);
            // not certain of the pixel (within cull_eps_px of a rounding boundary, ~1 % of the points): straight to the exact path
            cc[u].unusual |= cc[u].multi | (B2L_IDENTITY ? false : (cc[u].r2 < pl.rmin2));
            pxi[u] = __umul24((uint32_t)cc[u].rb, (uint32_t)g.cols) + (uint32_t)cc[u].cb;
            q0[u] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(qk) + (pxi[u] << 2));   // uniform base + 32-bit offset
        }
        bool mt[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            // qbound[px] = an upper bound of the SQUARED range below which a point of that pixel could be flagged (k_scan_qbound):
            // one compare decides; empty pixels hold 0
            mt[u] = cc[u].unusual | (cc[u].r2 < q0[u]);
        }
        const Ballot4 qg = ballot4(mt);
        if (qg.total) {
            const uint32_t word = (Gcur << 26) | (lane << kVoteQueuePxBits);
#pragma unroll
            for (int u = 0; u < kInFlight; ++u)
                if (mt[u]) seg[nq + ballot4_pos(qg, u)] = (word | ((uint32_t)u << 24)) | (cc[u].unusual ? kVoteQueuePxUncertain : pxi[u]);
            nq += qg.total;      // <= kDrainAt + 64 * kInFlight = kSeg
        }
    }
    if (__builtin_expect(slow != 0u, 0)) nsurv += exact_tiles<B2L_IDENTITY, 8, 64>(slow, first_tile, map, M, inv_pose, b2l_h, g, vals, tags, imgk);
    if (sampled && lane == 0u && nsurv) atomicAdd(&g_cull_stats[0], (unsigned long long)nsurv);
    __syncthreads();     // ucount and uqueue are final: every wave is behind its last drain
    uncertain_tail<B2L_IDENTITY, 8, 64, kCullQueue>(uqueue, ucount, map, run_base, inv_pose, b2l_h, g, vals, tags, imgk);
    __syncthreads();
    table_flush<kCullSlots>(tags, vals, imgk);
}

hipError_t cull_stats(unsigned long long* out2, int reset, hipStream_t s, int which_kernel)
{
    hipError_t e = hipMemcpyFromSymbolAsync(out2, HIP_SYMBOL(g_cull_stats), 16, 16 * (size_t)(which_kernel ? 1 : 0), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(s);
    if (e != hipSuccess || !reset) return e;
    const unsigned long long z[4] = {0, 0, 0, 0};
    e = hipMemcpyToSymbolAsync(HIP_SYMBOL(g_cull_stats), z, 32, 0, hipMemcpyHostToDevice, s);
    return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

hipError_t vote_map_range_images(const float4* map, size_t M, const double* inv_poses_dev, const float* approx_poses_dev, size_t kb, size_t nb,
                                 HostMat34 b2l, int b2l_identity, Geom g, const float* qbound_img, const float* tile_bounds_dev,
                                 const uint32_t* smax_bits_dev, float thr, int mode, uint64_t* map_img, hipStream_t s, const KernelOpts& ko)
{
    if (!M || !nb) return hipSuccess;
    if (mode != 0 || !ko.vote_cull || !approx_poses_dev || !qbound_img) return map_range_images(map, M, inv_poses_dev, approx_poses_dev, kb, nb, b2l, b2l_identity, g, map_img, s, ko);
    const ProjLaunch pl = make_proj_launch(g, b2l, b2l_identity, M);
    const RunLaunch rl = make_run_launch(pl.n_tiles, (uint32_t)std::max(ko.vote_tile_run, 1));
    dim3 grid(run_kf_grid(rl, nb));
    const float* tb = (ko.tile_cull && smax_bits_dev) ? tile_bounds_dev : nullptr;
    LTM_LAUNCH_ID_EL3(k_vote_map_cull, b2l_identity, g.el_fit != 0, grid, s, map, (uint32_t)M, inv_poses_dev, approx_poses_dev, (uint32_t)kb, (uint32_t)nb, b2l, pl, rl,
                      qbound_img, tb, smax_bits_dev, thr, map_img);
    return hipGetLastError();
}

// debug: number of points whose exact pixel is NOT inside the candidate set of the bounded-error projection.
// T (3x4 double) / ap (16 floats) are the exact and the approximate form of the same keyframe transform, or null.
__global__ void __launch_bounds__(kBlock)
k_cull_check(const float* __restrict__ xyz, size_t n, HostMat34 T, HostMat34 b2l, int b2l_identity, const float* __restrict__ ap, ProjLaunch pl,
             unsigned long long* __restrict__ bad)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RimgGeom& g = pl.g;
    const float4 p4 = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.0f);
    float3 pe = make_float3(p4.x, p4.y, p4.z), pa = pe;
    bool ok = true;
    if (ap) {   // exact side exactly as the vote kernels do it: inverse pose, float store, then base->lidar (utility.cpp:64-72)
        pe = xform(to_dev(T), pe);
        pe = b2l_identity ? xform_identity(pe) : xform(to_dev(b2l), pe);
        pa = xform_approx(ap, p4, ok);
    }
    CullCand cc = g.el_fit ? cull_candidates<true>(pl, pa) : cull_candidates<false>(pl, pa);      // the launch constants of the hot kernels, from the same make_proj_launch
    if (cc.unusual || !ok) return;
    if (ap && !b2l_identity && cc.r2 < pl.rmin2) return;      // these take the exact path in the kernels
    if (cc.multi) cull_expand(pl, cc);
    const Sph s = cart2sph(pe.x, pe.y, pe.z);
    int row, col;
    pixel_row_col(g, s.az, s.el, row, col);
    // the vote kernel relies on r_e^2 >= r2 (1 - 3e-6); the exact-image kernel on r_lo <= r_e <= r_lo (1 + 3e-6) with its r_lo
    const double re2 = (double)s.r * (double)s.r;
    const float r_lo = cull_r_lo(cc.r2);
    const bool good = (row == cc.r0 || row == cc.r1) && (col == cc.c0 || col == cc.c1) && (r_lo <= s.r) && (s.r <= r_lo * (1.0f + 3.0e-6f)) &&
                      (re2 >= (double)cc.r2 * (1.0 - 3.0e-6)) && (re2 <= (double)cc.r2 * (1.0 + 3.0e-6));
    if (!good) atomicAdd(bad, 1ull);
}
hipError_t cull_check(const float* xyz_dev, size_t n, const HostMat34* T, const HostMat34* b2l, int b2l_identity, const float* approx_pose_dev,
                      Geom g, unsigned long long* bad_dev, hipStream_t s)
{
    if (!n) return hipSuccess;
    HostMat34 z{};
    const int ident = b2l ? b2l_identity : 1;
    k_cull_check<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(xyz_dev, n, T ? *T : z, b2l ? *b2l : z, ident,
                                                            T ? approx_pose_dev : nullptr, make_proj_launch(g, b2l ? *b2l : z, ident, 0), bad_dev);
    return hipGetLastError();
}

// Probe points for the create-on-first-use validation of the bounded-error projection (ltm_api_vote.cpp: cull_geometry_ok): local-frame points that sit
// ON and a hair beside the pixel-rounding boundaries of this image shape -- rows, columns and their crossings -- at ranges from 0.3 m to 200 m, plus
// points in general position; optionally moved into the map frame by `pose` (3x4) so that the approximate inverse transform is exercised too.
__global__ void __launch_bounds__(kBlock)
k_cull_probe_points(Geom g, size_t n, HostMat34 pose, int with_pose, float* __restrict__ xyz)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t h = (uint32_t)i * 0x9e3779b1u + 0x7f4a7c15u;
    auto next = [&]() { h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16; return h; };
    const double jit[8] = {0.0, 1.0e-5, -1.0e-5, 1.0e-4, -1.0e-4, 4.0e-4, -4.0e-4, 2.0e-3};      // pixels off the boundary
    const double ranges[8] = {0.3, 1.0, 3.0, 10.0, 30.0, 60.0, 119.0, 200.0};
    const uint32_t kind = next() & 3u;                     // 0: row boundary, 1: column boundary, 2: both, 3: general position
    double rowf = (double)(next() % (uint32_t)(g.rows * 16 + 1)) / 16.0 - 0.5;
    double colf = (double)(next() % (uint32_t)(g.cols * 16 + 1)) / 16.0 - 0.5;
    if (kind == 0 || kind == 2) rowf = (double)(next() % (uint32_t)(g.rows + 1)) - 0.5 + jit[next() & 7u];
    if (kind == 1 || kind == 2) colf = (double)(next() % (uint32_t)(g.cols + 1)) - 0.5 + jit[next() & 7u];
    // rowf = R (1 - (el + V/2) / V), colf = C (az + H/2) / H  (utility.cpp:122-123)
    const double el = ((double)g.vfov * 0.5 - (double)g.vfov * rowf / (double)g.rows) * (3.14159265358979323846 / 180.0);
    const double az = ((double)g.hfov * colf / (double)g.cols - (double)g.hfov * 0.5) * (3.14159265358979323846 / 180.0);
    const double r = ranges[next() & 7u] * (1.0 + 1.0e-3 * (double)(next() & 1023u));
    double x = r * cos(el) * cos(az), y = r * cos(el) * sin(az), z = r * sin(el);
    if (with_pose) {
        const double X = pose.m[0] * x + pose.m[1] * y + pose.m[2] * z + pose.m[3], Y = pose.m[4] * x + pose.m[5] * y + pose.m[6] * z + pose.m[7],
                     Z = pose.m[8] * x + pose.m[9] * y + pose.m[10] * z + pose.m[11];
        x = X; y = Y; z = Z;
    }
    xyz[3 * i] = (float)x; xyz[3 * i + 1] = (float)y; xyz[3 * i + 2] = (float)z;
}
hipError_t cull_probe_points(Geom g, size_t n, const HostMat34* pose, float* xyz_dev, hipStream_t s)
{
    if (!n) return hipSuccess;
    HostMat34 z{};
    k_cull_probe_points<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(g, n, pose ? *pose : z, pose ? 1 : 0, xyz_dev);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Exact arg-min range image with a workgroup-local pre-filter (reprojection, ND votes, and any caller that needs the
// true image).  Only a point that could be the nearest of its pixel AMONG THE 4096 POINTS OF ITS OWN TILE can be the
// global arg-min, so:
//   phase 1a  bounded-error projection of every point; points whose pixel is certain (one candidate) publish an UPPER
//             bound of their range into a per-pixel LDS min table;
//   phase 1b  a point survives unless its pixel is certain, owns a table slot, and its range LOWER bound exceeds the
//             table's minimum upper bound (then some other point of the tile is strictly nearer in the same exact pixel);
//   phase 2   survivors (a few per pixel) get the exact arithmetic and the usual 64-bit LDS/global min.
// Built from the blocks above: pixel_certain / publish_bound (1a), ballot4 (1b), exact_range_insert / exact_insert (2), table_init / table_flush.
// The result is bit-identical to k_map_rimg_lds / the serial reference: discarded points are provably not arg-mins.
static constexpr int kBmSlotsMax = 1024;   // LDS table of the pre-filter: SLOT_ROWS x 64 pixels.  8 rows (8 workgroups per CU instead of 6) were tried: 15.3 ms against 10.3 ms per full-map launch -- the misses of the smaller table cost far more than the occupancy brings
static constexpr int kBmQueue = 2048;     // survivor queue capacity (~11 % of 4096 expected); overflow: the whole tile goes exact
// per-point record / queue entry: tile-local index (12 bits) | row (9) | column (11).  Row field 511 = pixel not certain
// (needs the full exact projection).  Images with >= 511 rows or >= 2048 columns mark every point that way.
static constexpr uint32_t kBmRowUncertain = 511u;
static constexpr int kBmUQueue = 1024;    // dense re-queue of the uncertain survivors (~1 % of the tile); beyond it they are handled in place

// pairs != null: workgroup b processes the (tile, keyframe) pair pairs[b] = tile * nb + keyframe (occlusion-culled launch, see exact_images_occlusion_*)
// (Round 5 tried three restructurings of phase 1 -- a wave-level combine of the lanes of one pixel, a single 64-bit {owner, minimum} table word, and
// a one-pass candidate stream -- all bit-exact, none faster: profiles/r5_ab_blockmin_restructurings.txt)
template <bool B2L_IDENTITY, bool EL3, int SLOT_ROWS = 16>
__global__ void __launch_bounds__(kBlock)
k_map_rimg_blockmin(const float4* __restrict__ map, uint32_t M, const double* __restrict__ inv_poses, const float* __restrict__ approx_poses,
                    uint32_t kb, uint32_t nb, HostMat34 b2l_h, ProjLaunch pl, uint64_t* __restrict__ img, const uint32_t* __restrict__ pairs, uint32_t n_pairs,
                    const uint8_t* __restrict__ submask)
{
    constexpr int kBmSlots = SLOT_ROWS * 64;
    static_assert(kBmSlots <= kBmSlotsMax, "");
    __shared__ uint64_t vals[kBmSlots];
    __shared__ uint32_t tags[kBmSlots];
    // the pre-filter's minimum table is only alive in phase 1 and the 64-bit (range | index) table only in phase 2: same LDS
    // (22.6 KB instead of 26.6 KB per workgroup: 7 workgroups per CU instead of 6)
    uint32_t* const amin = reinterpret_cast<uint32_t*>(vals);
    __shared__ uint32_t queue[kBmQueue];
    __shared__ uint16_t uqueue[kBmUQueue];
    __shared__ uint32_t qcount, ucount;
    const uint32_t per_block = (uint32_t)(kBlock * kPtsPerThread);
    TileKf tk;
    uint32_t quarters = 0xfu;
    if (pairs) {
        // the list is sorted by (tile, keyframe); workgroup b runs on XCD b % 8 (see tile_kf_of_block), so XCD x walks the x-th eighth of
        // the list front to back: consecutive workgroups of one XCD share a tile and it is served from that XCD's L2, as in the plain launch
        const uint32_t seg = (n_pairs + 7u) >> 3, at = (blockIdx.x & 7u) * seg + (blockIdx.x >> 3);
        if ((blockIdx.x >> 3) >= seg || at >= n_pairs) return;
        const uint32_t pr = pairs[at];
        tk.tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pr / nb)); tk.kfb = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pr % nb)); tk.valid = true;
        if (submask) quarters = (uint32_t)__builtin_amdgcn_readfirstlane((int)submask[pr]);      // quarters of the tile the occlusion cull left alive
    } else {
        tk = tile_kf_of_block(blockIdx.x, pl, nb);
    }
    if (!tk.valid) return;
    table_init<kBmSlots>(tags, nullptr, amin);
    if (threadIdx.x == 0) { qcount = 0; ucount = 0; }
    __syncthreads();
    const RimgGeom& g = pl.g;
    const uint32_t npx = pl.npx;
    const uint32_t block_base = tk.tile * per_block;
    const float4* __restrict__ mapb = map + block_base;
    const uint32_t nloc = min(per_block, M - block_base);
    const uint32_t kf = kb + tk.kfb;
    uint64_t* __restrict__ imgk = img + (size_t)tk.kfb * npx;
    const float* __restrict__ ap = approx_poses + 16 * (size_t)kf;
    static_assert(kBmRowUncertain == 511u, "ProjLaunch::packable is rows < 511");
    // per-lane record of the 16 points: amin slot (bits 20+) | row | col, and the range lower bound -- of the points that own an
    // amin slot; -1 for the others, which no table entry can beat (their slot field is 0: any valid index)
    float rlo[kPtsPerThread];
    uint32_t rec[kPtsPerThread];
    // Only full tiles run the pre-filter: the one partial tile at the end of the map takes the exact path as a whole (phase 2),
    // which keeps bounds tests and clamped indices out of these loops.
    // Neither does an image whose rows / columns do not fit the record (9 + 11 bits) nor a keyframe whose approximate pose is not usable (ap[15] == 0):
    // every point of such a tile used to be recorded as "uncertain" and survive, which overflowed the queue and sent the tile down the exact path anyway.
    const bool full_tile = (nloc == per_block) & pl.packable & (ap[15] != 0.0f);
    if (full_tile) {
        // ---- phase 1a (four points per lane in flight, as in k_vote_map_cull)
#pragma unroll
        for (int j0 = 0; j0 < kPtsPerThread; j0 += 4) {
            // points (j0 .. j0+3) * 256 + lane are the 1024 consecutive points of quarter j0 / 4: a hidden quarter costs nothing (uniform branch)
            if (!((quarters >> (j0 >> 2)) & 1u)) {
#pragma unroll
                for (int u = 0; u < 4; ++u) { rlo[j0 + u] = -1.0f; rec[j0 + u] = 0u; }
                continue;
            }
            float4 pt[4];
            CullCand cc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) pt[u] = mapb[(uint32_t)(j0 + u) * kBlock + threadIdx.x];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bool ok;      // (uniform, part of full_tile)
                const float3 p = xform_approx(ap, pt[u], ok);
                cc[u] = cull_candidates<EL3>(pl, p);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                const bool certain = pixel_certain(pl, cc[u]);
                rec[j] = ((certain ? (uint32_t)cc[u].rb : kBmRowUncertain) << 11) | (uint32_t)(cc[u].cb & 2047);
                rlo[j] = publish_bound<SLOT_ROWS, 64, 20>(cc[u], certain, (uint32_t)(cc[u].rb * g.cols + cc[u].cb), tags, amin, rec[j]);
            }
        }
        __syncthreads();
        // ---- phase 1b: a point survives unless it owns a slot and some point of the tile is provably nearer in the same pixel
        const uint32_t lane_word = threadIdx.x << 20;
#pragma unroll
        for (int j0 = 0; j0 < kPtsPerThread; j0 += 4) {
            // the four table reads go out together and nothing branches on them (the slot index is valid whatever the flags say)
            float am[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) am[u] = u2f(amin[rec[j0 + u] >> 20]);
            bool sv[4];
            const bool quarter_live = ((quarters >> (j0 >> 2)) & 1u) != 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) sv[u] = quarter_live & !(rlo[j0 + u] > am[u]);
            const Ballot4 qg = ballot4(sv);
            if (!qg.total) continue;
            uint32_t base = 0;
            if ((threadIdx.x & 63u) == 0u) base = atomicAdd(&qcount, qg.total);      // one LDS atomic per wave and group of four
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (base + qg.total > (uint32_t)kBmQueue) continue;          // overflow, decided on the scalar unit: the whole tile goes exact in phase 2
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (sv[u]) queue[base + ballot4_pos(qg, u)] = ((rec[j0 + u] & 0xfffffu) | lane_word) | ((uint32_t)((j0 + u) * kBlock) << 20);
        }
    }
    __syncthreads();
    table_init<kBmSlots>(nullptr, vals, nullptr);        // amin is dead from here on
    __syncthreads();
    // ---- phase 2: survivors.  Certain pixel: only the exact range; the others are re-queued densely and get the full exact projection
    const uint32_t nq = full_tile ? qcount : (uint32_t)kBmQueue + 1u;
    if (nloc == per_block && threadIdx.x == 0 && (blockIdx.x & 63u) == 0u) {   // sampled diagnostic
        atomicAdd(&g_cull_stats[2], (unsigned long long)nq);
        atomicAdd(&g_cull_stats[3], (unsigned long long)nloc);
    }
    const Mat34 Tinv = load_mat(inv_poses + 12 * (size_t)kf);
    if (__builtin_expect(nq > (uint32_t)kBmQueue, 0)) {      // queue overflow: a superset is always correct (min is idempotent)
        for (uint32_t li = threadIdx.x; li < nloc; li += kBlock)
            exact_insert<B2L_IDENTITY, SLOT_ROWS, 64>(map, block_base + li, Tinv, b2l_h, g, vals, tags, imgk);
    } else {
        for (uint32_t q = threadIdx.x; q < nq; q += kBlock) {
            const uint32_t e = queue[q];
            const uint32_t li = e >> 20;
            const int row = (int)((e >> 11) & 511u), col = (int)(e & 2047u);
            const uint32_t i = block_base + li;
            if (row == (int)kBmRowUncertain) {
                const uint32_t up = atomicAdd(&ucount, 1u);
                if (up < (uint32_t)kBmUQueue) uqueue[up] = (uint16_t)li;
                else exact_insert<B2L_IDENTITY, SLOT_ROWS, 64>(map, i, Tinv, b2l_h, g, vals, tags, imgk);
                continue;
            }
            exact_range_insert<B2L_IDENTITY, SLOT_ROWS, 64>(map, i, row, col, (uint32_t)(row * g.cols + col), Tinv, b2l_h, vals, tags, imgk);
        }
        __syncthreads();
        const uint32_t nu = min(ucount, (uint32_t)kBmUQueue);
        for (uint32_t q = threadIdx.x; q < nu; q += kBlock)
            exact_insert<B2L_IDENTITY, SLOT_ROWS, 64>(map, block_base + uqueue[q], Tinv, b2l_h, g, vals, tags, imgk);
    }
    __syncthreads();
    table_flush<kBmSlots>(tags, vals, imgk);
}

// The plain launch of the same pre-filter: one workgroup = a run of rl.T consecutive tiles against one keyframe (RunLaunch, as k_vote_map_cull), so the mapping,
// the image and pose pointers, the initialisation of the three tables, the fp64 pose, the flush and the statistics sample are paid once per run.  tags / vals
// live for the run (a slot never changes owner), and so does amin: a bound published by an earlier tile comes from a real map point of the same exact
// pixel, so a strictly farther point of a later tile is no arg-min either.  amin therefore has LDS of its own (4 KB more); the queues pay for it.
// Each wave queues the survivors of its own lanes in its own segment and counts them in a scalar register ; it drains the segment (the vote
// kernel's queue word) when a group of 4 x 64 points does not fit what is left of it, and once behind the run's last tile.  A segment
// always takes a group behind a drain (<= 256 words), so no tile ever falls back to the exact path for lack of room.
// The points of the next group of 4 x 256 -- of the next tile behind a tile's last group -- are requested before the arithmetic of the current one.
// Fast path iff ProjLaunch::vote_queueable, else every tile takes the whole-tile exact path like the partial last tile and a keyframe without
// a usable approximate pose (map_range_images sends the shapes that fit the one-tile kernel's record but not the queue word to the one-tile kernel instead).
// 8 KB vals + 4 tags + 4 amin + 5.9 queue + 0.5 uqueue = 22.4 KB: 7 workgroups per CU as the one-tile kernel, and 72 VGPRs for 7 waves per SIMD.
// What was measured: NOTEBOOK 4.1, profiles/blockmin_tile_run_ab_kernels.txt.
static constexpr uint32_t kBmRunSeg = 376;      // queue words per wave
static constexpr int kBmRunUQueue = 256;        // uncertain-pixel survivors of a run that wait for its end; a ticket past it is served on the spot
static constexpr uint32_t kBmRunDefaultT = 2;    // tiles per run when LTM_MAP_TILE_RUN is not given.  Full-map launches of the lot workload: 8.51 ms at 2, 8.34 at 4 (10.29 the one-tile kernel); the plain launches of a street step: 34.3 ms at 2, 34.8 at 1, 39.4 at 4 (37.2 the one-tile kernel) -- 2 is the one value that wins on both
static constexpr uint64_t kBmRunMinBlocks = 16384;   // ... and the workgroups a launch keeps at least (map_range_images); one choice, about nine times what the device holds at once, not swept
static constexpr uint32_t kBmRunNoBarrier = 1u, kBmRunResetPerTile = 2u;      // KernelOpts::map_tile_barrier / map_tile_persist, see flags below

// flags: kBmRunNoBarrier (the default) -- no barrier between a tile's phase 1a and 1b: a wave tests against what the others have published so far (a superset
//        survives); kBmRunResetPerTile (A/B form) -- the tables do not outlive a tile: drain, flush and re-initialise behind every tile (two more barriers per tile)
template <bool B2L_IDENTITY, bool EL3>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(7, 7)))      // 7 workgroups per CU by LDS: 72 VGPRs
k_map_rimg_blockmin_run(const float4* __restrict__ map, uint32_t M, const double* __restrict__ inv_poses, const float* __restrict__ approx_poses,
                        uint32_t kb, uint32_t nb, HostMat34 b2l_h, ProjLaunch pl, RunLaunch rl, uint32_t flags, uint64_t* __restrict__ img)
{
    constexpr int kRows = 16, kSlots = kRows * 64;
    static_assert(kSlots <= kBmSlotsMax, "");
    __shared__ uint64_t vals[kSlots];
    __shared__ uint32_t tags[kSlots];
    __shared__ uint32_t amin[kSlots];
    __shared__ uint32_t queue[kBmRunSeg * (kBlock / 64)];
    __shared__ uint16_t uqueue[kBmRunUQueue];       // (tile in run) << 12 | tile-local index
    __shared__ uint32_t ucount;
    static_assert(kMaxTileRun <= 16 && kPtsPerThread == 16 && kBlock == 256, "queue word: 4 bits of tile, 4 of group, 6 of lane; the wave is implied");
    static_assert(kBmRunSeg >= 4u * 64u && kSlots <= (1 << (32 - kVoteQueuePxBits)), "a group fits an empty segment; slot and pixel share a record");
    const uint32_t per_block = (uint32_t)(kBlock * kPtsPerThread);
    const RunKf rk = run_kf_of_block(blockIdx.x, rl, nb);
    if (!rk.valid) return;
    const RimgGeom& g = pl.g;
    const uint32_t kf = kb + rk.kfb;
    const uint32_t first_tile = rk.run * rl.T;
    const uint32_t run_base = first_tile * per_block;
    const uint32_t n_run = min(rl.T, pl.n_tiles - first_tile);      // >= 1: rk.run < rl.n_runs
    uint64_t* __restrict__ imgk = img + (size_t)rk.kfb * pl.npx;
    const float* __restrict__ ap = approx_poses + 16 * (size_t)kf;
    const double* __restrict__ inv_pose = inv_poses + 12 * (size_t)kf;      // (loaded where the exact arithmetic starts)
    for (int s = threadIdx.x; s < kSlots; s += kBlock) { tags[s] = kEmptyTag; amin[s] = 0x7f800000u; vals[s] = ~0ull; }
    if (threadIdx.x == 0) ucount = 0;
    __syncthreads();
    // Fast path as in k_vote_map_cull: tiles [0, n_fast) of the run are fast (all full tiles, or none), [n_fast, n_run) take the exact path as a whole.
    const uint32_t n_full = (first_tile + n_run == pl.n_tiles && (M & (per_block - 1u)) != 0u) ? n_run - 1u : n_run;
    const uint32_t n_fast = (pl.vote_queueable & ((f2u(ap[15]) << 1) != 0u)) ? n_full : 0u;
    const float4* __restrict__ mapr = map + run_base;
    uint32_t* __restrict__ seg = queue + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * kBmRunSeg;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_off = threadIdx.x & 192u;
    uint32_t nq = 0, nsurv = 0;      // uniform: entries in this wave's segment, survivors it has drained
    // phase 2, by wave.  This kernel keeps its own copies of drain_segment and, below, of table_init / table_flush, ballot4 and exact_tiles: NOTEBOOK 4.1
    auto drain = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const Mat34 Tinv = load_mat(inv_pose);
        for (uint32_t q = lane; q < nq; q += 64u) {
            const uint32_t e = seg[q];
            const uint32_t off = ((e >> 24) << 8) | wave_off | ((e >> kVoteQueuePxBits) & 63u);
            const uint32_t px = e & kVoteQueuePxUncertain;
            if (px == kVoteQueuePxUncertain) {
                const uint32_t ticket = atomicAdd(&ucount, 1u);
                if (ticket < (uint32_t)kBmRunUQueue) uqueue[ticket] = (uint16_t)off;
                else exact_insert<B2L_IDENTITY, kRows, 64>(map, run_base + off, Tinv, b2l_h, g, vals, tags, imgk);
                continue;
            }
            const uint32_t i = run_base + off;
            uint32_t row, col;
            vote_queue_row_col(px, (uint32_t)g.cols, pl.px_magic, pl.px_shift, row, col);
            const uint64_t v = ((uint64_t)exact_range_bits<B2L_IDENTITY>(map[i], Tinv, b2l_h) << 32) | (uint64_t)i;
            const int slot = table_claim<kRows, 64>(tags, (int)row, (int)col, px);
            if (slot >= 0) { if (v < vals[slot]) atomicMin(reinterpret_cast<unsigned long long*>(&vals[slot]), (unsigned long long)v); }   // (table_min)
            else img_min_u64(imgk + px, v);
        }
        nsurv += nq;
        nq = 0;
        __builtin_amdgcn_s_waitcnt(0x0f70);      // vmcnt(0) only: the drain's image atomics retire here (drain_segment)
    };
    float4 nxt[4];                   // the next group of 4 x 256 points, requested before the arithmetic of the current one
    if (n_fast) {
#pragma unroll
        for (int u = 0; u < 4; ++u) nxt[u] = mapr[(uint32_t)u * kBlock + threadIdx.x];
    }
    // What a lane keeps of its 16 points of a tile between phase 1b's test and the queue: amin slot (bits 18+) | pixel, and one survivor bit each.  A
    // drain inside a tile (resume) keeps nothing else alive.
    uint32_t rec[kPtsPerThread];
    uint32_t svm = 0;
    bool resume = false;             // uniform: the queue of tile t is being filled from group jstart on, behind a drain
    uint32_t jstart = 0;
    for (uint32_t t = 0;;) {
        const float4* __restrict__ mapt = mapr + t * per_block;
        // The drain stands once in the code: taken when a group of a tile's survivors does not fit the segment (then the tile's queue is resumed at that
        // group), behind the run's last tile, and at every tile's top in the A/B form that resets the tables behind every tile.
        const bool last = t == n_fast;
        const bool reset = ((flags & kBmRunResetPerTile) != 0u) & (t != 0u) & !resume;
        if (resume | ((last | reset) & (nq != 0u))) {
            drain();
            if (!last) {      // the prefetched points were dropped: requested again behind the drain's full wait
                const float4* __restrict__ nx = !resume ? mapt : (t + 1u < n_fast ? mapt + per_block : mapt + 12 * kBlock);
#pragma unroll
                for (int u = 0; u < 4; ++u) nxt[u] = nx[(uint32_t)u * kBlock + threadIdx.x];
            }
        }
        if (last) break;
        if (!resume) {
        if (__builtin_expect(reset, 0)) {
            __syncthreads();
            for (int s = threadIdx.x; s < kSlots; s += kBlock) {
                const uint32_t tg = tags[s];
                if (tg != kEmptyTag && vals[s] != ~0ull) img_min_u64(imgk + tg, vals[s]);
                tags[s] = kEmptyTag; amin[s] = 0x7f800000u; vals[s] = ~0ull;
            }
            __syncthreads();
        }
        float rlo[kPtsPerThread];      // publish_bound's range lower bounds
        // ---- phase 1a (four points per lane in flight, the next four requested): every point of the tile publishes its range upper bound before the
        // tile's points are tested
#pragma unroll
        for (int j0 = 0; j0 < kPtsPerThread; j0 += 4) {
            float3 p[4];
            CullCand cc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bool ok;      // (uniform, part of n_fast)
                p[u] = xform_approx(ap, nxt[u], ok);
            }
            // (the request goes out behind the last use of this group's coordinates, as in k_vote_map_cull)
            const float4* __restrict__ nx = j0 < 12 ? mapt + (j0 + 4) * kBlock : (t + 1u < n_fast ? mapt + per_block : mapt + 12 * kBlock);
#pragma unroll
            for (int u = 0; u < 4; ++u) nxt[u] = nx[(uint32_t)u * kBlock + threadIdx.x];
#pragma unroll
            for (int u = 0; u < 4; ++u) cc[u] = cull_candidates<EL3>(pl, p[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                const bool certain = pixel_certain(pl, cc[u]);
                const uint32_t px = __umul24((uint32_t)cc[u].rb, (uint32_t)g.cols) + (uint32_t)cc[u].cb;
                rec[j] = certain ? px : kVoteQueuePxUncertain;
                rlo[j] = publish_bound<kRows, 64, kVoteQueuePxBits>(cc[u], certain, px, tags, amin, rec[j]);
            }
        }
        if (!(flags & kBmRunNoBarrier)) __syncthreads();      // (A/B form) the one barrier of a tile; a wave may be anywhere else in the run when another one waits here
        // ---- phase 1b: a point survives unless it owns a slot and some point of the run so far is provably nearer in the same pixel
        svm = 0;
#pragma unroll
        for (int j0 = 0; j0 < kPtsPerThread; j0 += 4) {
            float am[4];      // (read together, nothing branches on them, as in k_map_rimg_blockmin)
#pragma unroll
            for (int u = 0; u < 4; ++u) am[u] = u2f(amin[rec[j0 + u] >> kVoteQueuePxBits]);
#pragma unroll
            for (int u = 0; u < 4; ++u) svm |= (rlo[j0 + u] > am[u]) ? 0u : (1u << (j0 + u));
        }
        jstart = 0;
        }
        // ---- the survivors' queue words, group by group; a group that does not fit sends the wave to the drain above and back here
        const uint32_t word = (t << 28) | (lane << kVoteQueuePxBits);
        resume = false;
#pragma unroll
        for (int j0 = 0; j0 < kPtsPerThread; j0 += 4) {
            if ((uint32_t)j0 < jstart) continue;      // uniform
            bool sv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) sv[u] = ((svm >> (j0 + u)) & 1u) != 0u;
            const uint64_t b0 = __builtin_amdgcn_ballot_w64(sv[0]), b1 = __builtin_amdgcn_ballot_w64(sv[1]),
                           b2 = __builtin_amdgcn_ballot_w64(sv[2]), b3 = __builtin_amdgcn_ballot_w64(sv[3]);
            const uint32_t n0 = (uint32_t)__popcll(b0), n1 = (uint32_t)__popcll(b1), n2 = (uint32_t)__popcll(b2), n3 = (uint32_t)__popcll(b3);
            const uint32_t total = n0 + n1 + n2 + n3;
            if (!total) continue;
            if (__builtin_expect(nq + total > kBmRunSeg, 0)) { jstart = (uint32_t)j0; resume = true; break; }      // decided on the scalar unit; behind a drain total <= 256 fits
            const uint64_t bal[4] = {b0, b1, b2, b3};
            const uint32_t off[4] = {nq, nq + n0, nq + n0 + n1, nq + n0 + n1 + n2};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!sv[u]) continue;
                const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[u], 0u));
                seg[off[u] + below] = (word | ((uint32_t)(j0 + u) << 24)) | (rec[j0 + u] & kVoteQueuePxUncertain);
            }
            nq += total;
        }
        if (!resume) ++t;
    }
    if (__builtin_expect(n_fast < n_run, 0)) {      // ---- tiles that are not on the fast path (as exact_tiles)
        const Mat34 Tinv = load_mat(inv_pose);
        for (uint32_t t = n_fast; t < n_run; ++t) {
            const uint32_t block_base = run_base + t * per_block;
            const uint32_t nloc = min(per_block, M - block_base);
            for (uint32_t li = threadIdx.x; li < nloc; li += kBlock)
                exact_insert<B2L_IDENTITY, kRows, 64>(map, block_base + li, Tinv, b2l_h, g, vals, tags, imgk);
            if (nloc == per_block) nsurv += per_block / (kBlock / 64);      // statistics: a full tile down the exact path counts every point as a survivor
        }
    }
    if ((blockIdx.x & 63u) == 0u) {      // sampled diagnostic: the points of the run's full tiles, the survivors per wave
        if (threadIdx.x == 0) atomicAdd(&g_cull_stats[3], (unsigned long long)(n_full * per_block));
        if (lane == 0u && nsurv) atomicAdd(&g_cull_stats[2], (unsigned long long)nsurv);
    }
    __syncthreads();     // ucount and uqueue are final: every wave is behind its last drain
    uncertain_tail<B2L_IDENTITY, kRows, 64, kBmRunUQueue>(uqueue, ucount, map, run_base, inv_pose, b2l_h, g, vals, tags, imgk);
    __syncthreads();
    for (int s = threadIdx.x; s < kSlots; s += kBlock) {
        const uint32_t tg = tags[s];
        if (tg != kEmptyTag && vals[s] != ~0ull) img_min_u64(imgk + tg, vals[s]);
    }
}

hipError_t map_range_images(const float4* map, size_t M, const double* inv_poses_dev, const float* approx_poses_dev, size_t kb, size_t nb,
                            HostMat34 b2l, int b2l_identity, Geom g, uint64_t* map_img, hipStream_t s, const KernelOpts& ko)
{
    if (!M || !nb) return hipSuccess;
    const ProjLaunch pl = make_proj_launch(g, b2l, b2l_identity, M);      // once per launch, on the host
    if (ko.map_kernel_variant >= 2 && approx_poses_dev && pl.packable && !pl.vote_queueable) {
        // An image whose rows and columns fit the one-tile kernel's 9 + 11-bit record but whose pixel count is beyond the run kernel's 18-bit pixel field
        // (vfov 90 at alpha 3: 270 x 1080 = 291 600): the run kernel would send every tile down the exact path, the one-tile kernel keeps its pre-filter.
        const size_t per_block = (size_t)kBlock * kPtsPerThread;
        dim3 grid(tile_kf_grid((M + per_block - 1) / per_block, nb));
        LTM_LAUNCH_ID_EL3(k_map_rimg_blockmin, b2l_identity, g.el_fit != 0, grid, s, map, (uint32_t)M, inv_poses_dev, approx_poses_dev, (uint32_t)kb, (uint32_t)nb, b2l, pl,
                          map_img, nullptr, 0u, nullptr);
        return hipGetLastError();
    }
    if (ko.map_kernel_variant >= 2 && approx_poses_dev) {
        // a run of map_tile_run consecutive tiles per workgroup (the list-driven launch, map_range_images_pairs, keeps the one-tile kernel: its pairs are
        // sorted by (tile, keyframe) and hold no runs of tiles for one keyframe)
        // A run of T tiles divides the workgroups of a launch by T.  Unless the run length is given (LTM_MAP_TILE_RUN), a short launch -- one keyframe, a small
        // map -- halves it until kBmRunMinBlocks workgroups are left, about nine rounds of the 1792 that the device holds at once: with a fixed run of four, the
        // launches of a step other than the full-map ones were slower than with the one-tile kernel (the shortest 127 -> 211 us in the one-lane trace).
        uint32_t T = ko.map_tile_run > 0 ? (uint32_t)ko.map_tile_run : kBmRunDefaultT;
        if (ko.map_tile_run <= 0)
            while (T > 1u && (uint64_t)((pl.n_tiles + T - 1u) / T) * nb < kBmRunMinBlocks) T >>= 1;
        const RunLaunch rl = make_run_launch(pl.n_tiles, T);
        dim3 grid(run_kf_grid(rl, nb));
        const uint32_t flags = (ko.map_tile_barrier ? 0u : kBmRunNoBarrier) | (ko.map_tile_persist ? 0u : kBmRunResetPerTile);
        LTM_LAUNCH_ID_EL3(k_map_rimg_blockmin_run, b2l_identity, g.el_fit != 0, grid, s, map, (uint32_t)M, inv_poses_dev, approx_poses_dev, (uint32_t)kb, (uint32_t)nb, b2l, pl,
                          rl, flags, map_img);
        return hipGetLastError();
    }
    if (ko.map_kernel_variant >= 1) {
        const size_t per_block = (size_t)kBlock * kPtsPerThread;
        dim3 grid(tile_kf_grid((M + per_block - 1) / per_block, nb));
        if (b2l_identity) k_map_rimg_lds<true><<<grid, dim3(kBlock), 0, s>>>(map, (uint32_t)M, inv_poses_dev, (uint32_t)kb, (uint32_t)nb, b2l, pl, map_img);
        else k_map_rimg_lds<false><<<grid, dim3(kBlock), 0, s>>>(map, (uint32_t)M, inv_poses_dev, (uint32_t)kb, (uint32_t)nb, b2l, pl, map_img);
        return hipGetLastError();
    }
    dim3 grid(grid_for(M), (unsigned)nb);
    if (b2l_identity) k_map_rimg<true><<<grid, dim3(kBlock), 0, s>>>(map, M, inv_poses_dev, kb, b2l, pl, map_img);
    else k_map_rimg<false><<<grid, dim3(kBlock), 0, s>>>(map, M, inv_poses_dev, kb, b2l, pl, map_img);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Occlusion cull for the exact arg-min image on LARGE maps (KITTI scale: 45 M points = 11 000 tiles, 2000 keyframes).  There nearly every
// (tile, keyframe) pair is far from the sensor, subtends a pixel or two, and loses to nearer returns -- yet k_map_rimg_blockmin ran
// its ~130 instructions per point for all of them (reproject_map 484 of 887 ms per step).  Now, per batch of keyframes:
//   1. the pairs are visited in SHELLS of sensor-to-tile distance (r_near, 2 r_near, 4 r_near, ...); the first shell is projected as it
//      is (list-driven k_map_rimg_blockmin);
//   2. before every later shell a coarse image holds, per run of 8 pixels of an image row, the LARGEST range of the image built so far
//      (an empty pixel counts as 10000);
//   3. a pair of that shell is dropped iff every coarse block its bounding sphere can touch is covered by returns strictly nearer
//      than the sphere's nearest point: none of its points can then be the arg-min of any pixel (ties need an equal range, excluded
//      by the strict comparison with margins), so the final image is bit-identical; the others are projected and become occluders of
//      the shells behind them (a facade 80 m away hides what a single near / far split at 60 m could not).
// The sphere's pixel rectangle is conservative: centre direction from the float transform (1e-5 rad), angular radius asin(rho / d)
// enlarged, +-1 pixel, rows clamped like the reference clamps elevations; spheres that straddle the +-180 deg seam, reach above 80 deg
// of elevation, are nearer than two radii or touch more than 256 coarse entries are simply kept.
struct SphereRect { int r0, r1, c0, c1; float d_lo; bool cullable; };
__device__ __forceinline__ SphereRect sphere_rect(const RimgGeom& g, const float* __restrict__ ap, const float* __restrict__ tb)
{
    SphereRect o; o.cullable = false; o.r0 = o.r1 = o.c0 = o.c1 = 0; o.d_lo = 0.0f;
    const float smin = ap[15];
    if (!(smin > 0.999f)) return o;                                   // not (nearly) a rigid pose: angles are not preserved
    const float cx = 0.5f * (tb[0] + tb[3]), cy = 0.5f * (tb[1] + tb[4]), cz = 0.5f * (tb[2] + tb[5]);
    const float hx = 0.5f * (tb[3] - tb[0]), hy = 0.5f * (tb[4] - tb[1]), hz = 0.5f * (tb[5] - tb[2]);
    const float rho = __builtin_sqrtf(hx * hx + hy * hy + hz * hz) * 1.001f + 2.0e-3f;
    bool ok;
    const float3 l = xform_approx(ap, make_float4(cx, cy, cz, 0.0f), ok);
    const float d = __builtin_sqrtf(l.x * l.x + l.y * l.y + l.z * l.z);
    if (!ok || !(d > 2.0f * rho) || !(d < 8.0e3f)) return o;         // NaN-safe; beyond 8 km the 10000-sentinel arithmetic starts to matter
    const float ratio = rho / d;                                      // <= 0.5
    const float alpha = asinf(ratio) * 1.01f + 2.0e-4f;
    const float rxy = __builtin_sqrtf(l.x * l.x + l.y * l.y);
    const float el0 = atan2f(l.z, rxy), az0 = atan2f(l.y, l.x);
    if (!(fabsf(el0) + alpha < 1.39f)) return o;                      // 80 deg
    const float sa = sinf(alpha) / cosf(fabsf(el0) + alpha);
    if (!(sa < 0.95f)) return o;
    const float daz = asinf(sa) * 1.01f + 2.0e-4f;
    if (!(az0 - daz > -3.1415f && az0 + daz < 3.1415f)) return o;     // would wrap around the seam
    const float r2d = 57.29577951308232f;
    // same (monotone) pixel mapping as pixel_row_col, evaluated in plain float with a pixel of margin on either side
    const float row_hi_el = g.frows * (1.0f - ((el0 + alpha) * r2d + g.half_v) / g.vfov), row_lo_el = g.frows * (1.0f - ((el0 - alpha) * r2d + g.half_v) / g.vfov);
    const float col_lo = g.fcols * (((az0 - daz) * r2d + g.half_h) / g.hfov), col_hi = g.fcols * (((az0 + daz) * r2d + g.half_h) / g.hfov);
    o.r0 = (int)fminf(fmaxf(floorf(row_hi_el) - 1.0f, 0.0f), g.row_max);
    o.r1 = (int)fminf(fmaxf(ceilf(row_lo_el) + 1.0f, 0.0f), g.row_max);
    o.c0 = (int)fminf(fmaxf(floorf(col_lo) - 1.0f, 0.0f), g.col_max);
    o.c1 = (int)fminf(fmaxf(ceilf(col_hi) + 1.0f, 0.0f), g.col_max);
    o.d_lo = (d - rho) * 0.9995f - 2.0e-3f;                            // below the exact float range of every point of the tile
    o.cullable = o.d_lo > 0.0f;
    return o;
}

// One distance shell of the occlusion-culled launch: flags[tile * nb + kfb] = 1 iff the pair has not been projected yet, the tile's
// bounding box comes within [r_lo, r_hi) of the sensor (pairs that cannot be culled at all count as distance 0) and -- once a coarse
// maximum of the image built so far exists -- the tile is not hidden behind it.  done[] remembers projected / dropped pairs.
__global__ void __launch_bounds__(kBlock)
k_pair_shell_select(const float* __restrict__ approx_poses, uint32_t kb, uint32_t nb, const float* __restrict__ tile_bounds, uint32_t n_tiles, Geom gg,
                    float r_lo, float r_hi, const uint32_t* __restrict__ cmax, uint32_t rbs, uint32_t cbs, uint8_t* __restrict__ done, uint8_t* __restrict__ flags,
                    uint32_t* __restrict__ dirty, uint32_t dw, const float* __restrict__ sub_bounds, uint8_t* __restrict__ submask, unsigned long long* __restrict__ sub_stats)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles * nb) return;
    if (done[t]) { flags[t] = 0; return; }
    const uint32_t tile = t / nb, kfb = t % nb;
    const float* ap = approx_poses + 16 * (size_t)(kb + kfb);
    const float* tb = tile_bounds + 6 * (size_t)tile;
    float d2 = 0.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) { const float c = ap[9 + d]; const float e = fmaxf(fmaxf(tb[d] - c, c - tb[3 + d]), 0.0f); d2 = __builtin_fmaf(e, e, d2); }
    const RimgGeom g = make_geom(gg);
    const SphereRect sr = sphere_rect(g, ap, tb);
    if (!sr.cullable || !(d2 == d2)) d2 = 0.0f;                        // NaN bounds / unusable pose / too near: first shell, never dropped
    if (!(d2 >= r_lo * r_lo && d2 < r_hi * r_hi)) { flags[t] = 0; return; }
    bool live = true;
    if (cmax && sr.cullable) {
        const int cb0 = sr.c0 >> 3, cb1 = sr.c1 >> 3;
        if ((sr.r1 - sr.r0 + 1) * (cb1 - cb0 + 1) <= 256) {
            uint32_t m = 0;
            for (int r = sr.r0; r <= sr.r1; ++r)
                for (int cb = cb0; cb <= cb1; ++cb) m = max(m, cmax[((size_t)kfb * rbs + r) * cbs + cb]);
            live = !(u2f(m) < sr.d_lo);
        }
    }
    // round 6: a second look at the four 1024-point quarters of a tile that stays live -- a quarter's bounding sphere has about half the tile's radius,
    // so its pixel rectangle is a quarter of the area and its nearest point is farther: quarters behind the image built so far are masked out of the
    // projection kernel's phase 1 (the same argument as for the whole tile: every pixel the quarter can touch already holds a strictly nearer return)
    if (submask) {
        uint32_t m4 = 0xfu;
        if (live && cmax && sr.cullable && sub_bounds) {
            m4 = 0u;
            for (int qd = 0; qd < 4; ++qd) {
                const float* sb = sub_bounds + 6 * ((size_t)tile * 4 + qd);
                if (!(sb[0] <= sb[3])) continue;                      // empty quarter (past the end of the map)
                const SphereRect qr = sphere_rect(g, ap, sb);
                bool ql = true;
                if (qr.cullable) {
                    const int qb0 = qr.c0 >> 3, qb1 = qr.c1 >> 3;
                    if ((qr.r1 - qr.r0 + 1) * (qb1 - qb0 + 1) <= 256) {
                        uint32_t m = 0;
                        for (int r = qr.r0; r <= qr.r1; ++r)
                            for (int cb = qb0; cb <= qb1; ++cb) m = max(m, cmax[((size_t)kfb * rbs + r) * cbs + cb]);
                        ql = !(u2f(m) < qr.d_lo);
                    }
                }
                if (ql) m4 |= 1u << qd;
            }
            if (m4 == 0u) live = false;
        }
        submask[t] = (uint8_t)m4;
        if (sub_stats && live) { atomicAdd(&sub_stats[0], 4ull); atomicAdd(&sub_stats[1], (unsigned long long)__popc(m4)); }
    }
    done[t] = 1;
    flags[t] = live ? 1 : 0;
    // rows of keyframe kfb's image that the projection of this pair can lower: the rows of its pixel rectangle (the rectangle the cull itself
    // trusts to contain every pixel the tile can touch), all rows if it has none.  The coarse maximum is recomputed for those rows only.
    if (live && dirty) {
        uint32_t* dk = dirty + (size_t)kfb * dw;
        if (sr.cullable) {
            for (int w = sr.r0 >> 5; w <= sr.r1 >> 5; ++w) {
                const int lo = max(sr.r0, w * 32) & 31, hi = min(sr.r1, w * 32 + 31) & 31;
                const uint32_t m = (hi == 31 ? ~0u : ((1u << (hi + 1)) - 1u)) & ~((1u << lo) - 1u);
                if ((__hip_atomic_load(dk + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) != m) atomicOr(dk + w, m);
            }
        } else {
            for (uint32_t w = 0; w < dw; ++w) atomicOr(dk + w, ~0u);
        }
    }
}
// cmax[kfb][row][cb] = largest range bits of the 8 pixels cb*8 .. cb*8+7 of one image row (positive floats order like their bits; empty =
// 10000).  Row-granular on purpose: the rows just above what near facades were mapped at stay empty until far tiles fill them, and an
// 8 x 8 block would let those rows keep every far tile near the horizon alive.
__global__ void __launch_bounds__(kBlock)
k_coarse_max(const uint64_t* __restrict__ img, uint32_t rows, uint32_t cols, uint32_t cbs, uint32_t nb, uint32_t* __restrict__ cmax,
             const uint32_t* __restrict__ dirty, uint32_t dw)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nb * rows * cbs) return;
    const uint32_t cb = t % cbs, r = (t / cbs) % rows, kfb = t / (cbs * rows);
    // round 4: only rows that the previous shell's projections could lower are re-reduced (the pass used to re-read every image of the batch
    // before every shell: 27 ms per step on the KITTI-scale workload, a tenth of it now); an image row nothing was projected into keeps its maximum
    if (dirty && !((dirty[(size_t)kfb * dw + (r >> 5)] >> (r & 31u)) & 1u)) return;
    const uint64_t* __restrict__ im = img + ((size_t)kfb * rows + r) * cols;
    uint32_t m = 0;
    for (uint32_t cc = cb * 8; cc < min(cols, cb * 8 + 8); ++cc) m = max(m, (uint32_t)(im[cc] >> 32));
    cmax[t] = m;
}
struct FlagIs { uint8_t v; __host__ __device__ uint32_t operator()(uint8_t f) const { return f == v ? 1u : 0u; } };
__global__ void __launch_bounds__(kBlock)
k_pair_list_scatter(const uint8_t* __restrict__ flags, uint8_t v, const uint32_t* __restrict__ pos, uint32_t n, uint32_t* __restrict__ list, uint32_t* __restrict__ count)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const bool on = flags[t] == v;
    if (on) list[pos[t]] = t;
    if (t == n - 1) *count = pos[t] + (on ? 1u : 0u);
}

// one shell: [r_lo, r_hi) of sensor-to-tile distance; img = the image built so far (ignored for the first shell: use_cmax = 0)
// dirty = nb x ((rows + 31) / 32) words (or null: every row re-reduced): in, the rows the PREVIOUS shell's projections could lower (all ones before
// the second shell: the first one is not tracked); out, those of this shell's
hipError_t occlusion_shell_pairs(const float* approx_poses_dev, size_t kb, size_t nb, const float* tile_bounds_dev, size_t n_tiles, Geom g, float r_lo, float r_hi,
                                 const uint64_t* img, int use_cmax, uint32_t* cmax, uint8_t* done, uint8_t* flags, uint32_t* pos, uint32_t* list, uint32_t* count,
                                 void* temp, size_t temp_bytes, hipStream_t s, uint32_t* dirty, const float* sub_bounds_dev, uint8_t* submask, unsigned long long* sub_stats)
{
    const uint32_t n = (uint32_t)(n_tiles * nb);
    const uint32_t rbs = (uint32_t)g.rows, cbs = (uint32_t)(g.cols + 7) / 8;
    const uint32_t dw = (rbs + 31u) / 32u;
    if (use_cmax) k_coarse_max<<<dim3(grid_for((size_t)nb * rbs * cbs)), dim3(kBlock), 0, s>>>(img, (uint32_t)g.rows, (uint32_t)g.cols, cbs, (uint32_t)nb, cmax, dirty, dw);
    if (dirty) { hipError_t e0 = hipMemsetAsync(dirty, 0, (size_t)nb * dw * 4, s); if (e0 != hipSuccess) return e0; }
    k_pair_shell_select<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(approx_poses_dev, (uint32_t)kb, (uint32_t)nb, tile_bounds_dev, (uint32_t)n_tiles, g, r_lo, r_hi,
                                                                use_cmax ? cmax : nullptr, rbs, cbs, done, flags, dirty, dw, sub_bounds_dev, submask, sub_stats);
    auto it = rocprim::make_transform_iterator(flags, FlagIs{1});
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, it, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    k_pair_list_scatter<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(flags, 1, pos, n, list, count);
    return hipGetLastError();
}
// k_map_rimg_blockmin over an explicit list of n_pairs (tile * nb + keyframe) pairs
hipError_t map_range_images_pairs(const float4* map, size_t M, const double* inv_poses_dev, const float* approx_poses_dev, size_t kb, size_t nb,
                                  HostMat34 b2l, int b2l_identity, Geom g, uint64_t* map_img, const uint32_t* pairs, size_t n_pairs, hipStream_t s, const KernelOpts& ko,
                                  const uint8_t* submask)
{
    if (!n_pairs) return hipSuccess;
    dim3 grid((unsigned)(((n_pairs + 7) / 8) * 8));
    const ProjLaunch pl = make_proj_launch(g, b2l, b2l_identity, M);
    LTM_LAUNCH_ID_EL3(k_map_rimg_blockmin, b2l_identity, g.el_fit != 0, grid, s, map, (uint32_t)M, inv_poses_dev, approx_poses_dev, (uint32_t)kb, (uint32_t)nb, b2l, pl,
                      map_img, pairs, (uint32_t)n_pairs, submask);
    return hipGetLastError();
}

// Removerter.cpp:381-413 (+ the diff of :458 / :515 / :572)
__global__ void __launch_bounds__(kBlock)
k_compare_flag(const uint32_t* __restrict__ scan_img, const uint64_t* __restrict__ map_img, size_t n, float thr, int mode,
               uint8_t* __restrict__ labels)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t mv = map_img[i];
    const float map_r = u2f((uint32_t)(mv >> 32));
    const float scan_r = u2f(scan_img[i]);
    const float diff = (mode == 0) ? (scan_r - map_r) : (map_r - scan_r);
    if (diff < 200.0f /* kValidDiffUpperBound, utility.h:94 */ && diff > thr) labels[(uint32_t)mv] = 1;
}

hipError_t compare_and_flag(const uint32_t* scan_img, const uint64_t* map_img, size_t n, float thr, int mode, uint8_t* labels,
                            hipStream_t s)
{
    if (!n) return hipSuccess;
    k_compare_flag<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(scan_img, map_img, n, thr, mode, labels);
    return hipGetLastError();
}

__global__ void __launch_bounds__(kBlock)
k_single_rimg(const float4* __restrict__ pts, size_t n, HostMat34 T1, int has1, HostMat34 T2, int has2, Geom gg,
              uint64_t* __restrict__ img)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RimgGeom g = make_geom(gg);
    const float4 p4 = pts[i];
    float3 p = make_float3(p4.x, p4.y, p4.z);
    if (has1) p = xform(to_dev(T1), p);
    if (has2) p = xform(to_dev(T2), p);
    const Sph s = cart2sph(p.x, p.y, p.z);
    const int px = pixel_index(g, s.az, s.el);
    img_min_u64(img + px, ((uint64_t)f2u(s.r) << 32) | (uint64_t)(uint32_t)i);
}

hipError_t single_range_image(const float4* pts, size_t n, const HostMat34* T1, const HostMat34* T2, Geom g, uint64_t* img,
                              hipStream_t s)
{
    if (!n) return hipSuccess;
    HostMat34 z{};
    k_single_rimg<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(pts, n, T1 ? *T1 : z, T1 != nullptr, T2 ? *T2 : z, T2 != nullptr, g, img);
    return hipGetLastError();
}

// ---- the two small passes of ltm_reproject_twin around one exact-image launch over the points that two maps share
// img_a holds the image of the shared cloud S (words carry S indices).  Every pixel with a point gets its index replaced through the two tables: in place
// for map A, into img_b for map B.  Both tables are strictly increasing, so the minimum over S is the same point under any of the three labellings.  The
// empty word (no point has written the pixel) stays as it is.
__global__ void __launch_bounds__(kBlock)
k_image_relabel2(uint64_t* __restrict__ img_a, uint64_t* __restrict__ img_b, size_t n, const uint32_t* __restrict__ s2a, const uint32_t* __restrict__ s2b)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t v = img_a[i];
    if (v == ((uint64_t)kNoPointBits << 32)) { img_b[i] = v; return; }
    const uint32_t s = (uint32_t)v;
    const uint64_t r = v & 0xffffffff00000000ull;
    img_a[i] = r | s2a[s];
    img_b[i] = r | s2b[s];
}
hipError_t image_relabel2(uint64_t* img_a, uint64_t* img_b, size_t n, const uint32_t* s2a, const uint32_t* s2b, hipStream_t s)
{
    if (!n) return hipSuccess;
    k_image_relabel2<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(img_a, img_b, n, s2a, s2b);
    return hipGetLastError();
}
// The listed points of a map into the images of keyframes [kb, kb + gridDim.y): k_map_rimg's arithmetic and word (the point's own map index), one global
// minimum per (point, keyframe).  For the few points of a map that its twin does not share.
template <bool B2L_IDENTITY>
__global__ void __launch_bounds__(kBlock)
k_project_points_indexed(const float4* __restrict__ map, const uint32_t* __restrict__ list, size_t n_list, const double* __restrict__ inv_poses, size_t kb,
                         HostMat34 b2l_h, ProjLaunch pl, uint64_t* __restrict__ img)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_list) return;
    const uint32_t i = list[j];
    const size_t kf = kb + blockIdx.y;
    const Mat34 Tinv = load_mat(inv_poses + 12 * kf);
    const RimgGeom& g = pl.g;
    const float4 p4 = map[i];
    float3 p = xform(Tinv, make_float3(p4.x, p4.y, p4.z));
    if (B2L_IDENTITY) p = xform_identity(p); else p = xform(to_dev(b2l_h), p);
    const Sph s = cart2sph(p.x, p.y, p.z);
    const int px = pixel_index(g, s.az, s.el);
    img_min_u64(img + (size_t)blockIdx.y * (size_t)pl.npx + px, ((uint64_t)f2u(s.r) << 32) | (uint64_t)i);
}
hipError_t project_points_indexed(const float4* map, const uint32_t* list, size_t n_list, const double* inv_poses_dev, size_t kb, size_t nb, HostMat34 b2l,
                                  int b2l_identity, Geom g, uint64_t* map_img, hipStream_t s)
{
    if (!n_list || !nb) return hipSuccess;
    const ProjLaunch pl = make_proj_launch(g, b2l, b2l_identity, n_list);
    dim3 grid(grid_for(n_list), (unsigned)nb);
    if (b2l_identity) k_project_points_indexed<true><<<grid, dim3(kBlock), 0, s>>>(map, list, n_list, inv_poses_dev, kb, b2l, pl, map_img);
    else k_project_points_indexed<false><<<grid, dim3(kBlock), 0, s>>>(map, list, n_list, inv_poses_dev, kb, b2l, pl, map_img);
    return hipGetLastError();
}

__global__ void k_decode_image(const uint64_t* img, size_t npx, float* rimg, int32_t* ptidx)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    const uint64_t v = img[i];
    rimg[i] = u2f((uint32_t)(v >> 32));
    if (ptidx) ptidx[i] = (int32_t)(uint32_t)v;
}
hipError_t decode_image(const uint64_t* img, size_t npx, float* rimg, int32_t* ptidx, hipStream_t s)
{
    k_decode_image<<<dim3(grid_for(npx)), dim3(kBlock), 0, s>>>(img, npx, rimg, ptidx);
    return hipGetLastError();
}

__global__ void k_debug_project(const float* xyz, size_t n, Geom gg, float* sph, int32_t* rc)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RimgGeom g = make_geom(gg);
    const Sph s = cart2sph(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    sph[3 * i] = s.az; sph[3 * i + 1] = s.el; sph[3 * i + 2] = s.r;
    const int px = pixel_index(g, s.az, s.el);
    rc[2 * i] = px / g.cols; rc[2 * i + 1] = px % g.cols;
}
hipError_t debug_project(const float* xyz_dev, size_t n, Geom g, float* az_el_r, int32_t* row_col, hipStream_t s)
{
    if (!n) return hipSuccess;
    k_debug_project<<<dim3(grid_for(n)), dim3(kBlock), 0, s>>>(xyz_dev, n, g, az_el_r, row_col);
    return hipGetLastError();
}

__global__ void __launch_bounds__(kBlock)
k_selfcheck(float vfov, float hfov, unsigned long long* __restrict__ counts)
{
    const float inv_v = 1.0f / vfov, inv_h = 1.0f / hfov;
    unsigned long long bad0 = 0, bad1 = 0, bad2 = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float a = u2f((uint32_t)i);
        const float e0 = rad2deg_exact(a), f0 = rad2deg_fast(a);
        const float e1 = a / vfov, f1 = div_by_const(a, vfov, inv_v, true);
        const float e2 = a / hfov, f2 = div_by_const(a, hfov, inv_h, true);
        // NaN payloads are irrelevant (NaN never reaches a pixel index in a defined way): compare as "both NaN"
        bad0 += !((f2u(e0) == f2u(f0)) | ((e0 != e0) & (f0 != f0)));
        bad1 += !((f2u(e1) == f2u(f1)) | ((e1 != e1) & (f1 != f1)));
        bad2 += !((f2u(e2) == f2u(f2)) | ((e2 != e2) & (f2 != f2)));
    }
    if (bad0) atomicAdd(counts + 0, bad0);
    if (bad1) atomicAdd(counts + 1, bad1);
    if (bad2) atomicAdd(counts + 2, bad2);
}
hipError_t selfcheck_fast_math(float vfov, float hfov, unsigned long long* counts_dev, hipStream_t s)
{
    k_selfcheck<<<dim3(8192), dim3(kBlock), 0, s>>>(vfov, hfov, counts_dev);
    return hipGetLastError();
}

// debug (ltm_debug_proj_launch): the launch constants as the hot kernels get them, flattened -- from the host's make_proj_launch, or (on_device) from
// the same expressions evaluated by one device thread, which is what every thread of every workgroup did before the constants moved to the host
static void proj_launch_flatten(const ProjLaunch& pl, uint32_t nb, float* f, uint32_t* u)
{
    const RimgGeom& g = pl.g;
    const float ff[kProjLaunchFloats] = {g.half_v, g.half_h, g.inv_v, g.inv_h, g.frows, g.fcols, g.row_max, g.col_max, pl.row_scale, pl.col_scale,
                                         pl.row_bias, pl.col_bias, pl.certain_lim, pl.rmin2, g.eps, g.el_tclamp};
    const uint32_t uu[kProjLaunchWords] = {(uint32_t)g.rows, (uint32_t)g.cols, pl.npx, pl.steep_clamps ? 1u : 0u, pl.packable ? 1u : 0u, pl.n_tiles, pl.n_tg,
                                           pl.tg_magic, pl.tg_shift, tile_kf_grid(pl.n_tiles, nb), g.el_fit ? 1u : 0u, g.fast ? 1u : 0u};
    memcpy(f, ff, sizeof ff);
    memcpy(u, uu, sizeof uu);
}
__global__ void k_proj_launch_eval(Geom gg, HostMat34 b2l, int b2l_identity, size_t M, ProjLaunch* out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = make_proj_launch(gg, b2l, b2l_identity, M);
}
hipError_t proj_launch_debug(Geom g, HostMat34 b2l, int b2l_identity, size_t M, size_t nb, int on_device, float* f, uint32_t* u)
{
    ProjLaunch pl = make_proj_launch(g, b2l, b2l_identity, M);
    if (on_device) {
        ProjLaunch* d = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), sizeof(ProjLaunch));
        if (e != hipSuccess) return e;
        k_proj_launch_eval<<<dim3(1), dim3(64)>>>(g, b2l, b2l_identity, M, d);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(&pl, d, sizeof(ProjLaunch), hipMemcpyDeviceToHost);
        (void)hipFree(d);
        if (e != hipSuccess) return e;
    }
    proj_launch_flatten(pl, (uint32_t)nb, f, u);
    return hipSuccess;
}
void proj_launch_blocks(size_t M, size_t nb, uint32_t first_block, size_t n, uint32_t* tile, uint32_t* kf)
{
    Geom g{};
    g.vfov = g.hfov = 1.0f;
    const ProjLaunch pl = make_proj_launch(g, HostMat34{}, 1, M);
    for (size_t i = 0; i < n; ++i) {
        const TileKf t = tile_kf_of_block(first_block + (uint32_t)i, pl, (uint32_t)nb);
        tile[i] = t.valid ? t.tile : 0xffffffffu;
        kf[i] = t.valid ? t.kfb : 0xffffffffu;
    }
}
size_t vote_run_blocks(size_t M, size_t nb, int tile_run)
{
    const size_t per_block = (size_t)kBlock * kPtsPerThread;
    return (size_t)make_run_launch((uint32_t)((M + per_block - 1) / per_block), (uint32_t)std::max(tile_run, 1)).n_runs * nb;
}
unsigned vote_run_launch_blocks(size_t M, size_t nb, int tile_run, uint32_t first_block, size_t n, uint32_t* run, uint32_t* kf, uint32_t* run_len)
{
    const size_t per_block = (size_t)kBlock * kPtsPerThread;
    const RunLaunch rl = make_run_launch((uint32_t)((M + per_block - 1) / per_block), (uint32_t)std::max(tile_run, 1));
    for (size_t i = 0; i < n; ++i) {
        const RunKf t = run_kf_of_block(first_block + (uint32_t)i, rl, (uint32_t)nb);
        run[i] = t.valid ? t.run : 0xffffffffu;
        kf[i] = t.valid ? t.kfb : 0xffffffffu;
    }
    if (run_len) *run_len = rl.T;
    return run_kf_grid(rl, nb);
}
// debug (ltm_debug_vote_queue_word): the queue-word constants of k_vote_map_cull as make_proj_launch makes them, and the row and column that the
// kernel's drain derives from pixel indices px[0 .. n) (vote_queue_row_col, the same function)
void vote_queue_word_debug(Geom g, uint32_t* u, size_t n, const uint32_t* px, uint32_t* row, uint32_t* col)
{
    HostMat34 b2l{};
    const ProjLaunch pl = make_proj_launch(g, b2l, 1, 0);
    const uint32_t uu[kVoteQueueWords] = {(uint32_t)pl.g.rows, (uint32_t)pl.g.cols, pl.npx, pl.vote_queueable ? 1u : 0u, pl.px_magic, pl.px_shift, kVoteQueuePxBits, kVoteQueuePxLimit};
    memcpy(u, uu, sizeof uu);
    for (size_t i = 0; i < n; ++i) vote_queue_row_col(px[i], (uint32_t)pl.g.cols, pl.px_magic, pl.px_shift, row[i], col[i]);
}

} // namespace ltm
