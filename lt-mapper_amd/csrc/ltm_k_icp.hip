// ltm_k_icp.hip -- batched point-to-point (and point-to-plane) ICP of source clouds against search indices: the counterpart of the pcl::IterativeClosestPoint runs of
// LTslam::doICPVirtualRelative / doICPGlobalRelative (ltslam/src/LTslam.cpp:187-301), one batch for all the loop pairs of addSCloops / addRSloops.
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
//
// One iteration of the WHOLE batch is two launches.  k_icp_correspond runs one thread per source point of every pair that has not stopped (the grid is
// over the concatenated sources, a per-block table names the pair): transform by the pair's accumulated T in double, round to float, exact 1-NN in the
// target's box tree (the walk of ltm_search_walk.h, so distances and ties are those of ltm_knn_search with k = 1), and the moments of the kept pairs
// (count, sum p, sum q, sum p q^T, sum d2) in double about the pair's origin -- map coordinates are kilometres from zero and raw second moments would
// cancel.  The moments of a workgroup are reduced by wave shuffles, then through LDS in wave order, and written as ONE record: no floating-point
// atomics anywhere, so the order of every sum is fixed by (source order, kIcpBlock) alone and a pair's result does not depend on what else is in the
// batch.  k_icp_update runs one workgroup per pair: the pair's records added in block order, the rigid transform by a one-sided Jacobi SVD of the 3 x 3
// cross-covariance in double, T <- T_iter T, PCL's stop tests, the trace row and the done flag.  The fitness score is one more pass of the first kernel
// in score mode (every finite point, no distance limit) and k_icp_fitness.
// Point-to-plane (ltm_icp_align_plane; include/ltm.h "icp, point-to-plane") is a third mode of the same two kernels: the correspondence kernel reads the target
// point's normal (ltm_k_normals.hip) and accumulates the 6 x 6 normal equations in a record of kIcpPlanePartial doubles, in the same fixed order; the update
// kernel solves them by Cholesky (plane_step) where the point-to-point mode takes the SVD.  Everything else -- transform, 1-NN, stop tests, trace -- is shared.
// Generalized ICP (ltm_icp_align_gicp; include/ltm.h "icp, generalized") is a fourth mode: both sides are search indices with normals, the source index's
// points are read in place in its own order, and the record (same layout as the plane record) holds the normal equations weighted per correspondence by
// the inverse of the two regularised covariances the normals imply; the update kernel's plane instantiation serves it unchanged.
#include "ltm_kernels_common.h"
#include "ltm_search_walk.h"      // search_key, knn_collect, seg_order_by_code
#include <cfloat>
namespace ltm {

namespace {

// sums over the workgroup of NV doubles per thread, in a fixed order: xor butterfly inside each wave, then waves 0..3 in order.  Thread c < NV returns the
// total of value c (the other threads return 0)
template <int NV, int STRIDE>
__device__ __forceinline__ double block_sum(double (&v)[NV], double (*lds)[STRIDE])
{
#pragma unroll
    for (int c = 0; c < NV; ++c) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_xor(v[c], off, 64);
    }
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int c = 0; c < NV; ++c) lds[wave][c] = v[c];
    }
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < (unsigned)NV) {
        r = lds[0][threadIdx.x];
        for (int w = 1; w < kIcpBlock / 64; ++w) r += lds[w][threadIdx.x];
    }
    return r;
}

// Rotation of the rigid transform that takes the p's onto the q's from their cross-covariance H = mean((p - pm)(q - qm)^T), row-major: with
// H = U S V^T, R = V diag(1, 1, det(V U^T)) U^T (Umeyama without scale).  One-sided Jacobi: the columns of A = H are rotated until they are
// orthogonal, A = U S and V collects the rotations.  u1, u2 are the two longest columns (the second orthogonalised against the first), u3 = u1 x u2
// -- whichever sign the third left singular vector has, the det term makes the product the same.  Rank 1: u2 is the unit vector most orthogonal
// to u1, made orthogonal; rank 0: R = I.  Always finite, orthonormal to rounding, det +1.
__device__ void rotation_from_covariance(const double* H, double* R)
{
    double A[3][3], V[3][3];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) { A[r][k] = H[3 * r + k]; V[r][k] = r == k ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int i = 0; i < 2; ++i)
            for (int j = i + 1; j < 3; ++j) {
                const double al = A[0][i] * A[0][i] + A[1][i] * A[1][i] + A[2][i] * A[2][i];
                const double be = A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j];
                const double ga = A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j];
                if (ga == 0.0 || fabs(ga) <= 1.0e-16 * sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int k = 0; k < 3; ++k) {
                    const double ai = A[k][i], aj = A[k][j], vi = V[k][i], vj = V[k][j];
                    A[k][i] = cs * ai - sn * aj; A[k][j] = sn * ai + cs * aj;
                    V[k][i] = cs * vi - sn * vj; V[k][j] = sn * vi + cs * vj;
                }
            }
        if (!rotated) break;
    }
    double s2[3];
    for (int k = 0; k < 3; ++k) s2[k] = A[0][k] * A[0][k] + A[1][k] * A[1][k] + A[2][k] * A[2][k];
    int k0 = 0, k1 = 1, k2 = 2;      // columns by descending length, the smaller index first among equals
    if (s2[k1] > s2[k0]) { const int x = k0; k0 = k1; k1 = x; }
    if (s2[k2] > s2[k1]) { const int x = k1; k1 = k2; k2 = x; }
    if (s2[k1] > s2[k0]) { const int x = k0; k0 = k1; k1 = x; }
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    if (!(s2[k0] > 0.0) || !isfinite(s2[k0])) return;
    double u1[3], u2[3], u3[3];
    const double n1 = sqrt(s2[k0]);
    for (int r = 0; r < 3; ++r) u1[r] = A[r][k0] / n1;
    double d = A[0][k1] * u1[0] + A[1][k1] * u1[1] + A[2][k1] * u1[2];
    for (int r = 0; r < 3; ++r) u2[r] = A[r][k1] - d * u1[r];
    double w2 = u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2];
    if (!(w2 > 1.0e-24 * s2[k0])) {      // rank 1
        int e = 0;
        if (fabs(u1[1]) < fabs(u1[e])) e = 1;
        if (fabs(u1[2]) < fabs(u1[e])) e = 2;
        for (int r = 0; r < 3; ++r) u2[r] = (r == e ? 1.0 : 0.0) - u1[e] * u1[r];
        w2 = u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2];
    }
    const double n2 = sqrt(w2);
    for (int r = 0; r < 3; ++r) u2[r] /= n2;
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double detV = V[0][k0] * (V[1][k1] * V[2][k2] - V[2][k1] * V[1][k2]) - V[0][k1] * (V[1][k0] * V[2][k2] - V[2][k0] * V[1][k2])
                      + V[0][k2] * (V[1][k0] * V[2][k1] - V[2][k0] * V[1][k1]);
    const double sg = detV < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) R[3 * r + k] = (V[r][k0] * u1[k] + V[r][k1] * u2[k]) + sg * V[r][k2] * u3[k];
}

// One point-to-plane step from the normal equations (ata: upper triangle of A^T A row-major, 21 entries; atb: A^T b): Cholesky without pivoting in
// double, x = (alpha, beta, gamma, t'), R = Rz(gamma) Ry(beta) Rx(alpha) as PCL's constructTransformationMatrix writes it, t = t' + o - R o (the system
// was formed about o).  false: a zero diagonal entry or a pivot d_j <= 1e-12 (A^T A)_jj -- the system does not determine all six unknowns.
__device__ bool plane_step(const double* ata, const double* atb, const double* o, double* R, double* t)
{
    double L[6][6];
    {
        int e = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) { L[c][r] = ata[e]; L[r][c] = ata[e]; ++e; }
    }
    for (int j = 0; j < 6; ++j) {
        const double ajj = L[j][j];
        double d = ajj;
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(ajj > 0.0) || !(d > 1.0e-12 * ajj)) return false;
        const double l = sqrt(d);
        L[j][j] = l;
        for (int i = j + 1; i < 6; ++i) {
            double v = L[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / l;
        }
    }
    double x[6];
    for (int i = 0; i < 6; ++i) {      // L y = A^T b
        double v = atb[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * x[k];
        x[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {     // L^T x = y
        double v = x[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    for (int i = 0; i < 6; ++i)
        if (!isfinite(x[i])) return false;
    const double sa = sin(x[0]), ca = cos(x[0]), sb = sin(x[1]), cb = cos(x[1]), sg = sin(x[2]), cg = cos(x[2]);
    R[0] = cg * cb; R[1] = -sg * ca + cg * sb * sa; R[2] = sg * sa + cg * sb * ca;
    R[3] = sg * cb; R[4] = cg * ca + sg * sb * sa;  R[5] = -cg * sa + sg * sb * ca;
    R[6] = -sb;     R[7] = cb * sa;                 R[8] = cb * ca;
    for (int r = 0; r < 3; ++r) t[r] = (x[3 + r] + o[r]) - ((R[3 * r] * o[0] + R[3 * r + 1] * o[1]) + R[3 * r + 2] * o[2]);
    return true;
}

} // namespace

// -------------------------------------------------------------------------------------------------- source order
// each source once into the code order of its target's frame (the shared order of ltm_search_walk.h, kIcpBlock points per workgroup)
hipError_t icp_order_sources(const IcpPair* pairs, const uint32_t* block_pair, uint32_t n_blocks, size_t n_pairs, const uint64_t* offsets, size_t total,
                             uint64_t* keys, uint64_t* keys_sorted, uint32_t* idx, uint32_t* order, float4* sorted, void* temp, size_t temp_bytes, hipStream_t s)
{
    static_assert(kIcpBlock == kSegBlock, "the correspondence grid and the source order share one owner table");
    return seg_order_by_code<IcpPair, 1>(pairs, block_pair, n_blocks, n_pairs, offsets, total, keys, keys_sorted, idx, order, sorted, temp, temp_bytes, s);
}

// ------------------------------------------------------------------------------------------------ correspondences
// MODE (IcpMode): kIcpPoint the moments of the SVD estimate, kIcpScore the fitness pass, kIcpPlane the normal equations of the point-to-plane estimate
// (include/ltm.h "icp, point-to-plane"): row [p x n, n], right side n . (q - p), with p, q about the pair's origin and n the target point's normal
// kIcpGicp the weighted normal equations of generalized ICP (include/ltm.h "icp, generalized"): per correspondence M = (2I - w (n_b n_b^T + m m^T))^-1 with
// n_b the target point's normal, m = R_T n_a the source point's normal turned by the current T and w = gicp_w = 1 - epsilon; the record is count,
// sum A^T M A (21), sum A^T M d (6), sum d2 with A = [-[p]x, I], d = q - p -- the layout of the plane record, so k_icp_update<true> solves it.  The
// sources of this mode are search indices read in place (P.src = the source index's points, P.snrm their normals): no sort, no copy; `sorted` is null
// then, also in the score pass that follows
template <int MODE>
__global__ void __launch_bounds__(kIcpBlock)
k_icp_correspond(const IcpPair* __restrict__ pairs, const IcpState* __restrict__ st, const uint32_t* __restrict__ block_pair, const float4* __restrict__ sorted,
                 double max_corr2, double* __restrict__ partials, double gicp_w)
{
    constexpr bool SCORE = MODE == kIcpScore;
    constexpr int NP = (MODE == kIcpPlane || MODE == kIcpGicp) ? kIcpPlanePartial : kIcpPartial;      // doubles per record
    __shared__ double lds[kIcpBlock / 64][NP];
    uint32_t local, pi;
    const IcpPair& P = block_record<kIcpBlock>(pairs, block_pair, local, &pi);
    local += threadIdx.x;
    const IcpState& S = st[pi];
    if (!SCORE && S.done) return;      // the whole workgroup: the flag was written by an earlier launch
    constexpr int NV = SCORE ? 2 : NP;
    double v[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) v[c] = 0.0;
    if (local < P.n) {
        const float4* base = (MODE == kIcpGicp || (SCORE && !sorted)) ? P.src : sorted + P.first;      // uniform over the workgroup
        const float4 p = base[local];
        if (finite3(p.x, p.y, p.z)) {
            const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
            const float qx = (float)(((S.T[0] * x + S.T[1] * y) + S.T[2] * z) + S.T[3]);
            const float qy = (float)(((S.T[4] * x + S.T[5] * y) + S.T[6] * z) + S.T[7]);
            const float qz = (float)(((S.T[8] * x + S.T[9] * y) + S.T[10] * z) + S.T[11]);
            // a transform that overflows float leaves no query: the point is skipped like a non-finite source point
            if (finite3(qx, qy, qz)) {
                const SearchTree t = P.t;
                KnnListReg<1> best; best.init(1);      // the nearest target point: distance, target index (INT_MAX: none), sorted position
                knn_collect(t, search_key(P.f, qx, qy, qz), 1u, qx, qy, qz, best.slots());
                const float bd = best.d[0];
                const int bi = best.w0[0];
                const uint32_t bj = best.w1[0];
                if constexpr (SCORE) {
                    if (bi != INT_MAX) { v[0] = 1.0; v[1] = (double)bd; }
                } else if constexpr (MODE == kIcpPlane) {
                    if (bi != INT_MAX && (double)bd <= max_corr2) {
                        const float4 tp = t.pts[bj], tn = P.nrm[bj];
                        if (finite3(tn.x, tn.y, tn.z)) {      // a correspondence without a normal is dropped
                            const double px = (double)qx - P.o[0], py = (double)qy - P.o[1], pz = (double)qz - P.o[2];
                            const double tx = (double)tp.x - P.o[0], ty = (double)tp.y - P.o[1], tz = (double)tp.z - P.o[2];
                            const double nx = (double)tn.x, ny = (double)tn.y, nz = (double)tn.z;
                            const double a[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
                            const double b = (nx * (tx - px) + ny * (ty - py)) + nz * (tz - pz);
                            v[0] = 1.0;
                            int e = 1;
#pragma unroll
                            for (int r = 0; r < 6; ++r)
#pragma unroll
                                for (int c = r; c < 6; ++c) v[e++] = a[r] * a[c];
#pragma unroll
                            for (int r = 0; r < 6; ++r) v[22 + r] = a[r] * b;
                            v[NP - 1] = (double)bd;
                        }
                    }
                } else if constexpr (MODE == kIcpGicp) {
                    if (bi != INT_MAX && (double)bd <= max_corr2) {
                        const float4 tp = t.pts[bj], tn = P.nrm[bj], sn = P.snrm[local];
                        if (finite3(tn.x, tn.y, tn.z) && finite3(sn.x, sn.y, sn.z)) {      // a correspondence without both normals is dropped
                            const double px = (double)qx - P.o[0], py = (double)qy - P.o[1], pz = (double)qz - P.o[2];
                            const double dx = ((double)tp.x - P.o[0]) - px, dy = ((double)tp.y - P.o[1]) - py, dz = ((double)tp.z - P.o[2]) - pz;
                            const double bx = (double)tn.x, by = (double)tn.y, bz = (double)tn.z;
                            const double ax = (double)sn.x, ay = (double)sn.y, az = (double)sn.z;
                            const double mx = (S.T[0] * ax + S.T[1] * ay) + S.T[2] * az;
                            const double my = (S.T[4] * ax + S.T[5] * ay) + S.T[6] * az;
                            const double mz = (S.T[8] * ax + S.T[9] * ay) + S.T[10] * az;
                            const double s00 = 2.0 - gicp_w * (bx * bx + mx * mx), s01 = -gicp_w * (bx * by + mx * my), s02 = -gicp_w * (bx * bz + mx * mz);
                            const double s11 = 2.0 - gicp_w * (by * by + my * my), s12 = -gicp_w * (by * bz + my * mz), s22 = 2.0 - gicp_w * (bz * bz + mz * mz);
                            const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
                            const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
                            const double rdet = 1.0 / ((s00 * c00 + s01 * c01) + s02 * c02);
                            const double M[3][3] = {{c00 * rdet, c01 * rdet, c02 * rdet}, {c01 * rdet, c11 * rdet, c12 * rdet}, {c02 * rdet, c12 * rdet, c22 * rdet}};
                            // G = M W with W = -[p]x (column j of W is e_j x p); A^T M A = [[p x G_j, G^T], [G, M]], A^T M d = [p x g, g] with g = M d
                            double G[3][3], g[3];
#pragma unroll
                            for (int r = 0; r < 3; ++r) {
                                G[r][0] = M[r][2] * py - M[r][1] * pz;
                                G[r][1] = M[r][0] * pz - M[r][2] * px;
                                G[r][2] = M[r][1] * px - M[r][0] * py;
                                g[r] = (M[r][0] * dx + M[r][1] * dy) + M[r][2] * dz;
                            }
                            v[0] = 1.0;
                            int e = 1;
#pragma unroll
                            for (int r = 0; r < 3; ++r) {
#pragma unroll
                                for (int k = r; k < 3; ++k) {      // row r of p x (column k of G)
                                    v[e++] = r == 0 ? py * G[2][k] - pz * G[1][k] : r == 1 ? pz * G[0][k] - px * G[2][k] : px * G[1][k] - py * G[0][k];
                                }
#pragma unroll
                                for (int k = 0; k < 3; ++k) v[e++] = G[k][r];
                            }
#pragma unroll
                            for (int r = 0; r < 3; ++r)
#pragma unroll
                                for (int k = r; k < 3; ++k) v[e++] = M[r][k];
                            v[22] = py * g[2] - pz * g[1]; v[23] = pz * g[0] - px * g[2]; v[24] = px * g[1] - py * g[0];
                            v[25] = g[0]; v[26] = g[1]; v[27] = g[2];
                            v[NP - 1] = (double)bd;
                        }
                    }
                } else if (bi != INT_MAX && (double)bd <= max_corr2) {
                    const float4 tp = t.pts[bj];
                    const double px = (double)qx - P.o[0], py = (double)qy - P.o[1], pz = (double)qz - P.o[2];
                    const double tx = (double)tp.x - P.o[0], ty = (double)tp.y - P.o[1], tz = (double)tp.z - P.o[2];
                    v[0] = 1.0;
                    v[1] = px; v[2] = py; v[3] = pz;
                    v[4] = tx; v[5] = ty; v[6] = tz;
                    v[7] = px * tx; v[8] = px * ty; v[9] = px * tz;
                    v[10] = py * tx; v[11] = py * ty; v[12] = py * tz;
                    v[13] = pz * tx; v[14] = pz * ty; v[15] = pz * tz;
                    v[16] = (double)bd;
                }
            }
        }
    }
    double* out = partials + (size_t)blockIdx.x * NP;
    if constexpr (SCORE) {
        double w[NV] = {v[0], v[1]};
        const double r = block_sum<NV>(w, lds);
        if (threadIdx.x < (unsigned)NV) out[threadIdx.x == 0 ? 0 : 16] = r;
    } else {
        const double r = block_sum<NP>(v, lds);
        if (threadIdx.x < (unsigned)NP) out[threadIdx.x] = r;
    }
}
hipError_t icp_correspond(const IcpPair* pairs, const IcpState* st, const uint32_t* block_pair, uint32_t n_blocks, const float4* sorted, double max_corr2,
                          int mode, double* partials, hipStream_t s, double gicp_w)
{
    if (!n_blocks) return hipSuccess;
    if (mode == kIcpScore) k_icp_correspond<kIcpScore><<<dim3(n_blocks), dim3(kIcpBlock), 0, s>>>(pairs, st, block_pair, sorted, max_corr2, partials, gicp_w);
    else if (mode == kIcpPlane) k_icp_correspond<kIcpPlane><<<dim3(n_blocks), dim3(kIcpBlock), 0, s>>>(pairs, st, block_pair, sorted, max_corr2, partials, gicp_w);
    else if (mode == kIcpGicp) k_icp_correspond<kIcpGicp><<<dim3(n_blocks), dim3(kIcpBlock), 0, s>>>(pairs, st, block_pair, nullptr, max_corr2, partials, gicp_w);
    else k_icp_correspond<kIcpPoint><<<dim3(n_blocks), dim3(kIcpBlock), 0, s>>>(pairs, st, block_pair, sorted, max_corr2, partials, gicp_w);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------------- update
template <bool PLANE>
__global__ void __launch_bounds__(64)
k_icp_update(const IcpPair* __restrict__ pairs, IcpState* __restrict__ st, const double* __restrict__ partials, int max_iterations, double eps_t, double eps_mse,
             double* __restrict__ trace, uint32_t* __restrict__ unfinished)
{
    constexpr int NP = PLANE ? kIcpPlanePartial : kIcpPartial;
    __shared__ double m[NP];
    const uint32_t pi = blockIdx.x;
    IcpState& S = st[pi];
    if (S.done) return;
    const IcpPair& P = pairs[pi];
    if (threadIdx.x < (unsigned)NP) {
        double a = 0.0;
        for (uint32_t b = 0; b < P.span.n_blocks; ++b) a += partials[(size_t)(P.span.block0 + b) * NP + threadIdx.x];      // block order
        m[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double n = m[0];
    const int it = S.iterations;
    const double mse = n > 0.0 ? m[NP - 1] / n : DBL_MAX;
    S.n_corr = (uint32_t)n;
    S.last_mse = mse;
    if (trace && it < max_iterations) {
        double* row = trace + ((size_t)pi * (size_t)max_iterations + (size_t)it) * 2;
        row[0] = n;
        if (n > 0.0) row[1] = mse;      // otherwise the NaN the buffer was filled with stays
    }
    int state = -1;
    double R[9], t[3];
    bool solved = n >= 3.0;
    if (!solved) {
        state = 0;
    } else if constexpr (PLANE) {
        solved = plane_step(m + 1, m + 22, P.o, R, t);
        if (!solved) state = 5;      // the system does not determine the step: T and the iteration count stay
    } else {
        double pm[3], qm[3], H[9];
        for (int k = 0; k < 3; ++k) { pm[k] = m[1 + k] / n; qm[k] = m[4 + k] / n; }
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) H[3 * r + k] = m[7 + 3 * r + k] / n - pm[r] * qm[k];
        rotation_from_covariance(H, R);
        // t = qm - R pm with the means taken back to the cloud's coordinates
        for (int r = 0; r < 3; ++r) {
            const double px = pm[0] + P.o[0], py = pm[1] + P.o[1], pz = pm[2] + P.o[2];
            t[r] = (qm[r] + P.o[r]) - ((R[3 * r] * px + R[3 * r + 1] * py) + R[3 * r + 2] * pz);
        }
    }
    if (solved) {
        double Tn[12];
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 4; ++k) Tn[4 * r + k] = (R[3 * r] * S.T[k] + R[3 * r + 1] * S.T[4 + k]) + R[3 * r + 2] * S.T[8 + k];
            Tn[4 * r + 3] += t[r];
        }
        for (int k = 0; k < 12; ++k) S.T[k] = Tn[k];
        S.iterations = it + 1;
        const double cos_angle = 0.5 * ((R[0] + R[4] + R[8]) - 1.0);
        const double t2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
        const double dm = fabs(mse - S.prev_mse);
        if (it + 1 >= max_iterations) state = 1;
        else if (cos_angle >= 1.0 - eps_t && t2 <= eps_t) state = 2;
        else if (dm < 1.0e-12) state = 3;
        else if (dm / S.prev_mse < eps_mse) state = 4;
        else S.prev_mse = mse;
    }
    if (state >= 0) {
        S.state = state;
        S.converged = state > 0 && state < 5 ? 1 : 0;
        S.done = 1;
        atomicSub(unfinished, 1u);
    }
}
hipError_t icp_update(const IcpPair* pairs, IcpState* st, size_t n_pairs, const double* partials, int max_iterations, double transformation_epsilon,
                      double euclidean_fitness_epsilon, double* trace, uint32_t* unfinished, hipStream_t s, int plane)
{
    if (!n_pairs) return hipSuccess;
    if (plane) k_icp_update<true><<<dim3((unsigned)n_pairs), dim3(64), 0, s>>>(pairs, st, partials, max_iterations, transformation_epsilon, euclidean_fitness_epsilon, trace, unfinished);
    else k_icp_update<false><<<dim3((unsigned)n_pairs), dim3(64), 0, s>>>(pairs, st, partials, max_iterations, transformation_epsilon, euclidean_fitness_epsilon, trace, unfinished);
    return hipGetLastError();
}

// fitness = mean d2 of the score pass (DBL_MAX if no point counted)
__global__ void __launch_bounds__(64)
k_icp_fitness(const IcpPair* __restrict__ pairs, IcpState* __restrict__ st, const double* __restrict__ partials)
{
    __shared__ double m[2];
    const IcpPair& P = pairs[blockIdx.x];
    if (threadIdx.x < 2) {
        const int c = threadIdx.x == 0 ? 0 : 16;
        double a = 0.0;
        for (uint32_t b = 0; b < P.span.n_blocks; ++b) a += partials[(size_t)(P.span.block0 + b) * kIcpPartial + c];
        m[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) st[blockIdx.x].fitness = m[0] > 0.0 ? m[1] / m[0] : DBL_MAX;
}
hipError_t icp_fitness(const IcpPair* pairs, IcpState* st, size_t n_pairs, const double* partials, hipStream_t s)
{
    if (!n_pairs) return hipSuccess;
    k_icp_fitness<<<dim3((unsigned)n_pairs), dim3(64), 0, s>>>(pairs, st, partials);
    return hipGetLastError();
}

} // namespace ltm
