// ltm_k_normals.hip -- surface normals and curvature of the target points of search indices: the counterpart of pcl::NormalEstimation (setKSearch,
// setViewPoint) over the cloud of a pcl::KdTreeFLANN.  The reference calls neither; the arithmetic is stated in include/ltm.h, "normals".
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
//
// One thread per finite target point, in the index's Morton order: the lanes of a wavefront are neighbours in space and walk the same part of the box
// tree, and the kNN seed is the point's own stored code (no query sort).  All indices of a call go through ONE launch over the batch's owner
// table (ltm_block_table.h).  The neighbour lists hold (d2, target index, sorted position) in
// ascending (d2, index) order -- in registers for k <= 16, in LDS [slot][lane] with one wavefront per workgroup above -- and the moments are summed in
// that order in double, so a normal depends on its index alone: no atomics, nothing that depends on the walk or on the rest of the batch.
#include "ltm_kernels_common.h"
#include "ltm_search_walk.h"      // pair_less (ltm_knn_list.h), walk, seed_leaves
#include "ltm_covariance.h"       // smallest_axis_from_moments: covariance, cyclic Jacobi, canonical sign
namespace ltm {

namespace {

// moments of the neighbours as differences from the query point, one neighbour at a time in list order
struct Moments {
    double s[3] = {0.0, 0.0, 0.0};
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // xx xy xz yy yz zz
    __device__ __forceinline__ void add(const float4& q, const float4& p)
    {
        const double dx = (double)q.x - (double)p.x, dy = (double)q.y - (double)p.y, dz = (double)q.z - (double)p.z;
        s[0] += dx; s[1] += dy; s[2] += dz;
        c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz; c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
    }
};

// normal and curvature from the moments of n >= 3 neighbours (include/ltm.h, "normals": covariance, cyclic Jacobi and canonical sign in ltm_covariance.h, then
// curvature and viewpoint flip)
__device__ float4 normal_from_moments(const Moments& M, int n, const float4& p, const double* vp)
{
    double nx, ny, nz, lam[3];
    const int e = smallest_axis_from_moments(M.s, M.c, n, nx, ny, nz, lam);
    const double tr = (lam[0] + lam[1]) + lam[2];
    const double lmin = fmax(lam[e], 0.0);
    const double curv = tr > 0.0 ? lmin / tr : 0.0;
    // flipNormalTowardsViewpoint
    const double dot = ((vp[0] - (double)p.x) * nx + (vp[1] - (double)p.y) * ny) + (vp[2] - (double)p.z) * nz;
    if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    return make_float4((float)nx, (float)ny, (float)nz, (float)curv);
}

__device__ __forceinline__ float4 nan4()
{
    const float q = __builtin_nanf("");
    return make_float4(q, q, q, q);
}

} // namespace

// (Both kernels write out the list of ltm_knn_list.h and the collect of ltm_search_walk.h: on knn_collect they ran 3 to 16 % slower)
// KT in {4, 8, 16}: the lists in registers, kept sorted by the insertion network of KnnListReg (ltm_knn_list.h) with two payload words, written out here
// (sentinels of distance -1 in the first KT - kk slots)
template <int KT>
__global__ void __launch_bounds__(kNormalsBlockReg)
k_normals_reg(const NormalsSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, int k)
{
    uint32_t j0;
    const NormalsSeg& S = block_record<kNormalsBlockReg>(segs, block_seg, j0);
    j0 += threadIdx.x;
    const SearchTree t = S.t;
    if (j0 >= t.Mf) return;
    const int kk = (int)min((uint32_t)k, t.Mf);
    if (kk < 3) { S.out[j0] = nan4(); return; }
    const float4 qp = t.pts[j0];
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
        for (uint32_t j = a; j < b; ++j) {
            const float4 p = t.pts[j];
            push(sqdist_l2simple(qp.x, qp.y, qp.z, p.x, p.y, p.z), (int)t.idx[j], j);
        }
    };
    uint32_t sa, sb;
    seed_leaves(t, t.keys[j0], (uint32_t)kk, sa, sb);
    for (uint32_t l = sa; l <= sb; ++l) visit(l);
    walk(t, qp.x, qp.y, qp.z, sa, sb, [&](double lb) { return lb > (double)bd[KT - 1]; }, visit);
    Moments M;
#pragma unroll
    for (int j = 0; j < KT; ++j)
        if (j >= KT - kk) M.add(t.pts[bj[j]], qp);
    S.out[j0] = normal_from_moments(M, kk, qp, S.vp);
}

// 16 < k <= 64: the lists in LDS, [slot][lane], one wavefront per workgroup (64 x 64 x 12 B = 48 KB)
__global__ void __launch_bounds__(kNormalsBlockLds)
k_normals_lds(const NormalsSeg* __restrict__ segs, const uint32_t* __restrict__ block_seg, int k)
{
    __shared__ float sd[kNormalsMaxK][kNormalsBlockLds];
    __shared__ int si[kNormalsMaxK][kNormalsBlockLds];
    __shared__ uint32_t sj[kNormalsMaxK][kNormalsBlockLds];
    uint32_t j0;
    const NormalsSeg& S = block_record<kNormalsBlockLds>(segs, block_seg, j0);
    j0 += threadIdx.x;
    const SearchTree t = S.t;
    const int lane = (int)threadIdx.x;
    if (j0 >= t.Mf) return;
    const int kk = (int)min((uint32_t)min(k, kNormalsMaxK), t.Mf);
    if (kk < 3) { S.out[j0] = nan4(); return; }
    const float4 qp = t.pts[j0];
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
        for (uint32_t j = a; j < b; ++j) {
            const float4 p = t.pts[j];
            push(sqdist_l2simple(qp.x, qp.y, qp.z, p.x, p.y, p.z), (int)t.idx[j], j);
        }
    };
    uint32_t sa, sb;
    seed_leaves(t, t.keys[j0], (uint32_t)kk, sa, sb);
    for (uint32_t l = sa; l <= sb; ++l) visit(l);
    walk(t, qp.x, qp.y, qp.z, sa, sb, [&](double lb) { return lb > (double)kth; }, visit);
    Moments M;
    for (int j = 0; j < cnt; ++j) M.add(t.pts[sj[j][lane]], qp);      // cnt == kk: the index holds at least kk points
    S.out[j0] = normal_from_moments(M, cnt, qp, S.vp);
}

int normals_block(int k) { return k > kKnnListRegSlots ? kNormalsBlockLds : kNormalsBlockReg; }

hipError_t estimate_normals(const NormalsSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, int k, hipStream_t s)
{
    if (!n_blocks) return hipSuccess;
    if (k < 3 || k > kNormalsMaxK) return hipErrorInvalidValue;
    knn_list_dispatch<false>(k, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if constexpr (KT == 0) k_normals_lds<<<dim3(n_blocks), dim3(kNormalsBlockLds), 0, s>>>(segs, block_seg, k);
        else k_normals_reg<KT><<<dim3(n_blocks), dim3(kNormalsBlockReg), 0, s>>>(segs, block_seg, k);
    });
    return hipGetLastError();
}

} // namespace ltm
