// ltm_k_plane.hip -- RANSAC plane segmentation of records of points (the keyframes of a scan set, or one cloud): the counterpart of pcl::SACSegmentation with
// SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE and SAC_RANSAC.  The reference calls neither; the arithmetic is stated in include/ltm.h, "planes".
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
//
// A fixed sequence of launches for the whole batch, every record found through the batch's owner table (ltm_block_table.h):
//   k_plane_hypotheses  one thread per (record, hypothesis): the three drawn points, N, p0, T and the valid byte (axis test included)
//   k_plane_count       hypotheses x points.  A workgroup keeps kPlaneBlockPoints points of ONE record in registers, as doubles, and loops over the record's
//                       hypotheses.  The hypothesis is wave-uniform: its seven values come through scalar loads.  A point costs eight double operations and
//                       a compare; the wave's count is the popcount of the ballot, added on the scalar side; one LDS atomic per wave and hypothesis, one
//                       global integer atomic per workgroup and hypothesis with a non-zero count.
//   k_plane_best        one wavefront per record: arg-max by (count descending, h ascending); the unrefined coefficients
//   k_plane_moments     the moments of the best hypothesis's inliers about its p0 in 256-point chunks, each summed by a tree (the shape of "clusters")
//   k_plane_combine     one wavefront per record: chunk sums 64 at a time by a tree, groups in order; covariance, Jacobi (ltm_covariance.h), sign
//   k_plane_labels      one pass with the final plane; the final count by ballot and one integer atomic per wave
// No floating-point atomics: every double is a function of its record alone.
#include "ltm_kernels_common.h"
#include "ltm_covariance.h"
namespace ltm {

namespace {

// the 32-bit hash behind the draws (include/ltm.h, "planes"): murmur3's finaliser over seed + 0x9E3779B9 (3 h + j + 1)
__device__ __forceinline__ uint32_t plane_mix(uint32_t seed, uint32_t h, uint32_t j)
{
    uint32_t x = seed + 0x9E3779B9u * (3u * h + j + 1u);
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite3(const float4& p) { return finite_f(p.x) && finite_f(p.y) && finite_f(p.z); }
__device__ __forceinline__ bool finite_d(double v) { return (((uint64_t)__double_as_longlong(v) >> 52) & 0x7ffull) != 0x7ffull; }

// (a, b, c, d) of the unit normal n through point c0, with the canonical sign: towards the axis if there is one and n . A != 0, else the component of
// largest magnitude positive (the lower axis among equals)
__device__ void plane_coefficients(double nx, double ny, double nz, const double* c0, const PlaneLaunch& L, double* coeff)
{
    double big = nx;
    if (fabs(ny) > fabs(big)) big = ny;
    if (fabs(nz) > fabs(big)) big = nz;
    bool flip = big < 0.0;
    if (L.has_axis) {
        const double dot = (nx * L.axis[0] + ny * L.axis[1]) + nz * L.axis[2];
        if (dot > 0.0) flip = false;
        else if (dot < 0.0) flip = true;
    }
    if (flip) { nx = -nx; ny = -ny; nz = -nz; }
    coeff[0] = nx; coeff[1] = ny; coeff[2] = nz;
    coeff[3] = -((nx * c0[0] + ny * c0[1]) + nz * c0[2]);
}

} // namespace

__global__ void __launch_bounds__(kPlaneBlock)
k_plane_hypotheses(const PlaneRec* __restrict__ recs, PlaneLaunch L, uint32_t blocks_per_rec, PlaneHyp* __restrict__ hyp, uint8_t* __restrict__ valid,
                   PlaneOut* __restrict__ out)
{
    const uint32_t r = blockIdx.x / blocks_per_rec;
    const uint32_t h = (blockIdx.x - r * blocks_per_rec) * kPlaneBlock + threadIdx.x;
    const bool live = h < L.max_iterations;
    const uint32_t n = recs[r].n;
    PlaneHyp H;
    H.N[0] = H.N[1] = H.N[2] = 0.0; H.p0[0] = H.p0[1] = H.p0[2] = 0.0; H.T = 0.0; H.pad = 0.0;
    bool ok = false;
    if (live) {
        uint32_t s[3];
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) s[j] = (uint32_t)(((uint64_t)plane_mix(L.seed, h, j) * (uint64_t)n) >> 32);
        ok = n >= 3u && s[0] != s[1] && s[0] != s[2] && s[1] != s[2];      // fewer than three points: two positions coincide anyway; nothing is loaded
        if (ok) {
            const float4 a = recs[r].pts[s[0]], b = recs[r].pts[s[1]], c = recs[r].pts[s[2]];
            ok = finite3(a) && finite3(b) && finite3(c);
            if (ok) {
                const double p0x = (double)a.x, p0y = (double)a.y, p0z = (double)a.z;
                const double ux = (double)b.x - p0x, uy = (double)b.y - p0y, uz = (double)b.z - p0z;
                const double vx = (double)c.x - p0x, vy = (double)c.y - p0y, vz = (double)c.z - p0z;
                const double Nx = uy * vz - uz * vy, Ny = uz * vx - ux * vz, Nz = ux * vy - uy * vx;
                const double n2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
                ok = n2 > 0.0 && finite_d(n2);
                if (ok && L.constrained) {
                    const double dot = (Nx * L.axis[0] + Ny * L.axis[1]) + Nz * L.axis[2];
                    const double aa = (L.axis[0] * L.axis[0] + L.axis[1] * L.axis[1]) + L.axis[2] * L.axis[2];
                    ok = dot * dot >= (L.c2 * n2) * aa;
                }
                if (ok) {
                    H.N[0] = Nx; H.N[1] = Ny; H.N[2] = Nz; H.p0[0] = p0x; H.p0[1] = p0y; H.p0[2] = p0z;
                    H.T = (L.thr * L.thr) * n2;
                }
            }
        }
        const size_t at = (size_t)r * L.max_iterations + h;
        hyp[at] = H;
        valid[at] = ok ? 1 : 0;
    }
    const uint32_t nv = ballot_count(ok);
    if (nv && (threadIdx.x & 63u) == 0u) atomicAdd(&out[r].n_valid, nv);
}

__global__ void __launch_bounds__(kPlaneBlock)
k_plane_count(const PlaneRec* __restrict__ recs, const uint32_t* __restrict__ block_rec, const PlaneHyp* __restrict__ hyp, uint32_t H,
              uint32_t* __restrict__ counts, const PlaneOut* __restrict__ out, unsigned long long* __restrict__ stats)
{
    __shared__ uint32_t cnt[kPlaneMaxIterations];
    uint32_t first, r;
    const PlaneRec& R = block_record<kPlaneBlockPoints>(recs, block_rec, first, &r);
    const uint32_t tid = threadIdx.x, n = R.n;
    for (uint32_t h = tid; h < H; h += kPlaneBlock) cnt[h] = 0u;
    double qx[kPlanePointsPerThread], qy[kPlanePointsPerThread], qz[kPlanePointsPerThread];
    const double qnan = __builtin_nan("");
    uint32_t n_finite = 0;
#pragma unroll
    for (int k = 0; k < kPlanePointsPerThread; ++k) {
        const uint32_t i = first + (uint32_t)k * kPlaneBlock + tid;
        bool fin = false;
        qx[k] = qy[k] = qz[k] = qnan;      // a point that is not there, or not finite, fails every test: NaN < T is false
        if (i < n) {
            const float4 p = R.pts[i];
            fin = finite3(p);
            if (fin) { qx[k] = (double)p.x; qy[k] = (double)p.y; qz[k] = (double)p.z; }
        }
        n_finite += ballot_count(fin);
    }
    __syncthreads();
    const PlaneHyp* __restrict__ Hr = hyp + (size_t)r * H;
    for (uint32_t h = 0; h < H; ++h) {
        const double T = Hr[h].T;
        if (!(T > 0.0)) continue;      // invalid (or a T that underflowed: nothing is below it)
        const double Nx = Hr[h].N[0], Ny = Hr[h].N[1], Nz = Hr[h].N[2], px = Hr[h].p0[0], py = Hr[h].p0[1], pz = Hr[h].p0[2];
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < kPlanePointsPerThread; ++k) {
            const double dx = qx[k] - px, dy = qy[k] - py, dz = qz[k] - pz;
            const double s = (Nx * dx + Ny * dy) + Nz * dz;
            c += ballot_count(s * s < T);
        }
        if (c && (tid & 63u) == 0u) atomicAdd(&cnt[h], c);
    }
    __syncthreads();
    for (uint32_t h = tid; h < H; h += kPlaneBlock) {
        const uint32_t v = cnt[h];
        if (v) atomicAdd(&counts[(size_t)r * H + h], v);
    }
    if (n_finite && (tid & 63u) == 0u) atomicAdd(&stats[0], (unsigned long long)n_finite * (unsigned long long)out[r].n_valid);
}

__global__ void __launch_bounds__(64)
k_plane_best(const PlaneHyp* __restrict__ hyp, const uint8_t* __restrict__ valid, const uint32_t* __restrict__ counts, PlaneLaunch L, PlaneOut* __restrict__ out,
             unsigned long long* __restrict__ stats)
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
    PlaneOut& O = out[r];
    const double qnan = __builtin_nan("");
    O.n_inliers = 0u; O.refined = 0;
    atomicAdd(&stats[1], (unsigned long long)O.n_valid);
    atomicAdd(&stats[2], 1ull);
    if (!hi) {
        O.found = 0; O.best = -1; O.consensus = 0u;
        for (int d = 0; d < 4; ++d) O.coeff[d] = qnan;
        for (int d = 0; d < 3; ++d) O.point[d] = qnan;
        return;
    }
    const uint32_t h = ~lo;
    const PlaneHyp B = hyp[(size_t)r * H + h];
    O.found = 1; O.best = (int32_t)h; O.consensus = hi - 1u;
    const double len = sqrt((B.N[0] * B.N[0] + B.N[1] * B.N[1]) + B.N[2] * B.N[2]);
    plane_coefficients(B.N[0] / len, B.N[1] / len, B.N[2] / len, B.p0, L, O.coeff);
    for (int d = 0; d < 3; ++d) O.point[d] = B.p0[d];
}

__global__ void __launch_bounds__(kPlaneBlock)
k_plane_moments(const PlaneRec* __restrict__ recs, const uint32_t* __restrict__ block_rec, const PlaneHyp* __restrict__ hyp, uint32_t H,
                const PlaneOut* __restrict__ out, double* __restrict__ partials)
{
    __shared__ double sm[kPlaneMoments][kPlaneChunk];
    static_assert(kPlaneBlock == kPlaneChunk, "one thread per point of a chunk");
    uint32_t first, r;
    const PlaneRec& R = block_record<kPlaneBlockPoints>(recs, block_rec, first, &r);
    if (!out[r].found) return;      // uniform
    const PlaneHyp& B = hyp[(size_t)r * H + (uint32_t)out[r].best];
    const double Nx = B.N[0], Ny = B.N[1], Nz = B.N[2], px = B.p0[0], py = B.p0[1], pz = B.p0[2], T = B.T;
    const uint32_t tid = threadIdx.x, n = R.n;
    for (int k = 0; k < kPlanePointsPerThread; ++k) {
        const uint32_t base = first + (uint32_t)k * kPlaneChunk;
        if (base >= n) break;      // uniform
        const uint32_t i = base + tid;
        double v[kPlaneMoments];
#pragma unroll
        for (int m = 0; m < kPlaneMoments; ++m) v[m] = 0.0;      // a point that is no inlier enters as zeros
        if (i < n) {
            const float4 p = R.pts[i];
            if (finite3(p)) {
                const double dx = (double)p.x - px, dy = (double)p.y - py, dz = (double)p.z - pz;
                const double s = (Nx * dx + Ny * dy) + Nz * dz;
                if (s * s < T) {
                    v[0] = dx; v[1] = dy; v[2] = dz;
                    v[3] = dx * dx; v[4] = dx * dy; v[5] = dx * dz; v[6] = dy * dy; v[7] = dy * dz; v[8] = dz * dz;
                }
            }
        }
#pragma unroll
        for (int m = 0; m < kPlaneMoments; ++m) sm[m][tid] = v[m];
        for (uint32_t s = kPlaneChunk / 2; s > 0; s >>= 1) {
            __syncthreads();
            if (tid < s) {
#pragma unroll
                for (int m = 0; m < kPlaneMoments; ++m) sm[m][tid] = sm[m][tid] + sm[m][tid + s];
            }
        }
        if (tid == 0) {
            double* dst = partials + (size_t)(R.chunk0 + base / kPlaneChunk) * kPlaneMoments;
#pragma unroll
            for (int m = 0; m < kPlaneMoments; ++m) dst[m] = sm[m][0];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64)
k_plane_combine(const PlaneRec* __restrict__ recs, const PlaneHyp* __restrict__ hyp, PlaneLaunch L, const double* __restrict__ partials, PlaneOut* __restrict__ out,
                unsigned long long* __restrict__ stats)
{
    const uint32_t r = blockIdx.x, lane = threadIdx.x, H = L.max_iterations;
    PlaneOut& O = out[r];
    if (!O.found || O.consensus < 3u) return;      // uniform
    const uint32_t n_chunks = recs[r].n / kPlaneChunk + (recs[r].n % kPlaneChunk ? 1u : 0u), chunk0 = recs[r].chunk0;
    double sum[kPlaneMoments];
#pragma unroll
    for (int m = 0; m < kPlaneMoments; ++m) sum[m] = 0.0;
    for (uint32_t g = 0; g < n_chunks; g += 64u) {
        const uint32_t b = g + lane;
        const bool in = b < n_chunks;
#pragma unroll
        for (int m = 0; m < kPlaneMoments; ++m) {
            double v = in ? partials[(size_t)(chunk0 + b) * kPlaneMoments + m] : 0.0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
            sum[m] = sum[m] + v;
        }
    }
    if (lane != 0u) return;
    double nx, ny, nz, lam[3];
    const int e = smallest_axis_from_moments(sum, sum + 3, (int)O.consensus, nx, ny, nz, lam);
    const double second = e == 0 ? fmin(lam[1], lam[2]) : (e == 1 ? fmin(lam[0], lam[2]) : fmin(lam[0], lam[1]));
    if (!(second > lam[e]) || !finite_d(nx) || !finite_d(ny) || !finite_d(nz)) return;      // the two smallest coincide: the unrefined plane stands
    const PlaneHyp& B = hyp[(size_t)r * H + (uint32_t)O.best];
    const double cnt = (double)O.consensus;
    double c0[3];
    for (int d = 0; d < 3; ++d) c0[d] = B.p0[d] + sum[d] / cnt;
    plane_coefficients(nx, ny, nz, c0, L, O.coeff);
    for (int d = 0; d < 3; ++d) O.point[d] = c0[d];
    O.refined = 1;
    atomicAdd(&stats[3], 1ull);
}

__global__ void __launch_bounds__(kPlaneBlock)
k_plane_labels(const PlaneRec* __restrict__ recs, const uint32_t* __restrict__ block_rec, double thr, PlaneOut* out, uint8_t* __restrict__ labels)
{
    uint32_t first, r;
    const PlaneRec& R = block_record<kPlaneBlockPoints>(recs, block_rec, first, &r);
    const double a = out[r].coeff[0], b = out[r].coeff[1], c = out[r].coeff[2], cx = out[r].point[0], cy = out[r].point[1], cz = out[r].point[2];
    const uint32_t tid = threadIdx.x, n = R.n;
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < kPlanePointsPerThread; ++k) {
        const uint32_t i = first + (uint32_t)k * kPlaneBlock + tid;
        bool in = false;
        if (i < n) {
            const float4 p = R.pts[i];
            if (finite3(p)) {
                const double ex = (double)p.x - cx, ey = (double)p.y - cy, ez = (double)p.z - cz;
                in = fabs((a * ex + b * ey) + c * ez) < thr;      // no plane: the coefficients are NaN and nothing is below thr
            }
            labels[R.base + i] = in ? 1 : 0;
        }
        cnt += ballot_count(in);
    }
    if (cnt && (tid & 63u) == 0u) atomicAdd(&out[r].n_inliers, cnt);
}

hipError_t plane_segment(const PlaneRec* recs, const uint32_t* block_rec, uint32_t n_blocks, uint32_t n_recs, const PlaneLaunch& L, PlaneHyp* hyp, uint8_t* valid,
                         uint32_t* counts, double* partials, PlaneOut* out, uint8_t* labels, unsigned long long* stats4, hipStream_t s)
{
    if (!n_recs) return hipSuccess;
    if (L.max_iterations < 1u || L.max_iterations > (uint32_t)kPlaneMaxIterations) return hipErrorInvalidValue;
    const uint32_t bpr = (L.max_iterations + kPlaneBlock - 1) / kPlaneBlock;
    if ((uint64_t)n_recs * bpr >= BlockTable::kMaxBlocks) return hipErrorInvalidValue;
    k_plane_hypotheses<<<dim3(n_recs * bpr), dim3(kPlaneBlock), 0, s>>>(recs, L, bpr, hyp, valid, out);
    if (n_blocks) k_plane_count<<<dim3(n_blocks), dim3(kPlaneBlock), 0, s>>>(recs, block_rec, hyp, L.max_iterations, counts, out, stats4);
    k_plane_best<<<dim3(n_recs), dim3(64), 0, s>>>(hyp, valid, counts, L, out, stats4);
    if (L.refine && n_blocks) {
        k_plane_moments<<<dim3(n_blocks), dim3(kPlaneBlock), 0, s>>>(recs, block_rec, hyp, L.max_iterations, out, partials);
        k_plane_combine<<<dim3(n_recs), dim3(64), 0, s>>>(recs, hyp, L, partials, out, stats4);
    }
    if (n_blocks) k_plane_labels<<<dim3(n_blocks), dim3(kPlaneBlock), 0, s>>>(recs, block_rec, L.thr, out, labels);
    return hipGetLastError();
}

} // namespace ltm
