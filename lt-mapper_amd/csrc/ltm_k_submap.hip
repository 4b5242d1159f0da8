// ltm_k_submap.hip -- assembling the loop submaps: the keyframes around a key, each moved by its float affine, concatenated -- the loop bodies of
// Session::loopFindNearKeyframesLocalCoord / CentralCoord (ltslam/src/Session.cpp:98-104, :125-131) with transformPointCloud (ltslam/src/utility.cpp:80-103)
// for ALL the windows of a batch in one launch.
// (gfx950 / CDNA4, wave64; part of libltm_hip.so -- shared definitions in ltm_kernels_common.h, launch wrappers declared in ltm_kernels.h)
//
// One thread per output point, one float4 load and one float4 store: a streaming kernel, 32 B / point.  The grid is over the concatenated windows; the
// batch's owner table (ltm_block_table.h) names the piece (window, source keyframe, affine) a workgroup belongs to, so the piece's record is uniform
// over the workgroup and its loads are scalar.  The host lays the pieces out from the scan set's host offsets: no size is read back.
#include "ltm_kernels_common.h"
namespace ltm {

__global__ void __launch_bounds__(kBlock)
k_submap_gather(const float4* __restrict__ scans, const SubmapPiece* __restrict__ pieces, const uint32_t* __restrict__ block_piece,
                const float* __restrict__ affines12, float4* __restrict__ out)
{
    uint32_t local;
    const SubmapPiece P = block_record<kBlock>(pieces, block_piece, local);
    local += threadIdx.x;
    if (local >= P.n) return;
    const float* __restrict__ t = affines12 + (size_t)12 * P.affine;
    const float4 p = scans[P.src + local];
    // utility.cpp:97-99: transCur(r,0) * x + transCur(r,1) * y + transCur(r,2) * z + transCur(r,3), left to right, every operation rounded to float
    // (the unit is compiled with -ffp-contract=off: no fused multiply-add); an identity affine still runs, so -0.0 becomes +0.0 and inf makes NaNs
    float4 o;
    o.x = ((t[0] * p.x + t[1] * p.y) + t[2] * p.z) + t[3];
    o.y = ((t[4] * p.x + t[5] * p.y) + t[6] * p.z) + t[7];
    o.z = ((t[8] * p.x + t[9] * p.y) + t[10] * p.z) + t[11];
    o.w = p.w;
    out[P.dst + local] = o;
}

hipError_t submap_gather(const float4* scans, const SubmapPiece* pieces, const uint32_t* block_piece, uint32_t n_blocks, const float* affines12, float4* out,
                         hipStream_t s)
{
    if (!n_blocks) return hipSuccess;
    k_submap_gather<<<dim3(n_blocks), dim3(kBlock), 0, s>>>(scans, pieces, block_piece, affines12, out);
    return hipGetLastError();
}

} // namespace ltm
