// ltm_kernels.h -- host-callable launchers of the gfx950 kernels (definitions in the ltm_k_*.hip unit of their stage).
// All launchers enqueue on the given stream and return the hipError_t of the launch.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include "ltm_block_table.h"      // BlockSpan
#include "ltm_knn_list.h"         // kKnnListSlots

namespace ltm {

struct Geom {            // range-image geometry (utility.cpp:222-236 resetRimgSize + fov)
    float vfov, hfov;
    int rows, cols;
    int fast;            // 1: use the self-checked fast arithmetic forms (ltm_device_math.h), 0: plain IEEE divisions
    float cull_eps_px;   // half-width [pixels] of the band around a pixel-rounding boundary inside which the bounded-error projection
                         // does not trust its pixel (proportional to the image resolution: the angular error is fixed, see geom_for)
    // Elevation of the bounded-error projection when the field of view clamps everything steeper than vfov/2 + 2 deg < 45 deg:
    // atan(t) ~ t * (el_c[0] + u (el_c[1] + u (el_c[2] + u el_c[3]))), u = t^2, fitted on [0, tan(vfov/2 + 2 deg)] when the context is
    // created (fit_elevation_poly in ltm_api_core.cpp) and evaluated at min(t, el_tclamp); el_tclamp = tan(vfov/2 + one pixel) puts
    // every clamped elevation in the MIDDLE of the out-of-image row -1 / R, where its pixel (row 0 / R-1 after the clamp) is certain.
    int el_fit;          // 0: the fit is not good enough for this field of view, the kernels use the generic polynomial on [0, 1]
    float el_c[4];
    float el_tclamp;
};

// 3x4 row-major double (last row of the 4x4 is never used by PCL's se3 transformer)
struct HostMat34 { double m[12]; };

static const uint32_t kNoPointBits = 0x461C4000u;   // bit pattern of kFlagNoPOINT = 10000.0f (utility.h:93)

// ---- fills ----
hipError_t fill_u32(uint32_t* p, uint32_t v, size_t n, hipStream_t s);
hipError_t fill_u64(uint64_t* p, uint64_t v, size_t n, hipStream_t s);

// ---- projection / vote ----
// scan2RangeImg of keyframes [kb, kb+nb) into n_shapes (1 .. kMaxScanShapes) image shapes of one field of view in ONE pass over the points (k_scan_rimg_multi, one global
// atomic per point and shape, then k_image_max per shape): imgs[j][(kf-kb)*npx_j + px] = min range bits, imgs[j] pre-filled with the empty range by the caller.
// smax_bits[j] (nb entries, zeroed by the caller, nullable): per keyframe the float bits of the largest scan range.
static constexpr int kMaxScanShapes = 8;
hipError_t scan_range_images_multi(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t nb, uint64_t n_pts, uint64_t max_kf_pts, Geom g,
                                   int n_shapes, const int* rows, const int* cols, uint32_t* const* imgs, uint32_t* const* smax_bits, hipStream_t s);
// squared-range bound image of the range-culled vote kernel from finished scan images (see k_scan_qbound)
hipError_t scan_qbound(const uint32_t* scan_img, size_t n, float thr, float* qbound, hipStream_t s);
// The same images built in LDS and written once (k_scan_rimg_lds): one workgroup per (keyframe, band).  A band is, for every shape, a contiguous range of
// its rows -- band b of B holds rows [b rows / B, (b + 1) rows / B) -- so the bands cut every shape at (nearly) the same elevations and a point lands in
// one band, or two next to each other, for all shapes at once.  All row ranges of a band lie one behind the other in the workgroup's LDS, each rounded up to
// whole 16-byte words plus one (the kernel shifts a range by up to 3 pixels so that LDS and global addresses are aligned alike).
static constexpr int kScanLdsThreads = 1024;                                                            // 16 waves: the only workgroup of its CU
static constexpr size_t kScanLdsQueueBytes = (size_t)(kScanLdsThreads / 64) * 128 * 4;                  // per wave 128 queued points
static constexpr size_t kScanLdsReduceBytes = (size_t)kMaxScanShapes * (kScanLdsThreads / 64) * 4;      // per shape and wave one partial maximum
static constexpr size_t kScanLdsBudget = (size_t)160 * 1024 - kScanLdsQueueBytes - kScanLdsReduceBytes; // image bytes of a band: 155136
static constexpr int kMaxScanBands = 4096;
static constexpr double kScanBandMarginDeg = 0.01;      // how far the kernel's first reject stays outside a band's elevations
struct ScanBands { int n_shapes; int rows[kMaxScanShapes], cols[kMaxScanShapes]; int n_bands; size_t max_band_bytes; };
#ifdef __HIPCC__
#define LTM_HOST_DEVICE __host__ __device__
#else
#define LTM_HOST_DEVICE
#endif
LTM_HOST_DEVICE inline int scan_band_row0(int rows, int n_bands, int b) { return (int)(((long long)b * rows) / n_bands); }      // first row of band b (b = n_bands: rows)
LTM_HOST_DEVICE inline size_t scan_band_shape_words(int band_rows, int cols) { return (((size_t)band_rows * (size_t)cols + 3u) + 3u) & ~(size_t)3u; }
size_t scan_band_bytes(const ScanBands& p, int b);
// the plan with the fewest bands whose bytes fit `budget`; false when there is none (a single row of all shapes together is wider than the budget, more than
// kMaxScanShapes shapes, a shape without pixels, more than kMaxScanBands bands): those take scan_range_images_multi
bool make_scan_bands(int n_shapes, const int* rows, const int* cols, size_t budget, ScanBands* out);
// imgs[j] need no fill: every pixel is written exactly once.  smax_bits[j] zeroed by the caller.  qbounds (nullable, and each entry nullable): the bound image of
// scan_qbound for `thr`, written in the same pass.  Every image pointer 16-byte aligned; no keyframe longer than 2^32 - 1 points.
hipError_t scan_range_images_lds(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t nb, Geom g, const ScanBands& plan,
                                 uint32_t* const* imgs, uint32_t* const* smax_bits, float* const* qbounds, float thr, hipStream_t s);
// bounds[6*t..] = {min xyz, max xyz} of map points [4096 t, 4096 (t+1))
hipError_t tile_bounds(const float4* map, size_t M, float* bounds, hipStream_t s);
hipError_t subtile_bounds(const float4* map, size_t M, float* bounds, hipStream_t s);   // 4 x 6 floats per 4096-point tile: its 1024-point quarters
// Kernel variants and diagnostics, held by the context (ltm_ctx::kopts, read from the environment at ltm_create) and handed to the launchers: K contexts
// on K host threads (ltm_run --gpus K) share no mutable state.  The non-default values are A/B baselines and timing diagnostics, not product paths.
struct KernelOpts {
    int map_kernel_variant = 2;   // LTM_MAP_KERNEL   exact arg-min image: 0 one global atomic per point, 1 LDS pre-reduction, 2 + workgroup-local arg-min pre-filter
    int vote_cull = 1;            // LTM_VOTE_CULL    1: mode-0 votes use k_vote_map_cull, 0: the exact-image kernel
    int tile_cull = 1;            // LTM_TILE_CULL    whole-tile range cull inside k_vote_map_cull
    int vote_tile_run = 4;        // LTM_VOTE_TILE_RUN  consecutive map tiles that one workgroup of k_vote_map_cull takes for its keyframe (1 .. 16; 1, 2, 8 and 16 measured slower, profiles/vote_wave_queue_ab_kernels.txt)
    int map_tile_run = 0;         // LTM_MAP_TILE_RUN  consecutive map tiles that one workgroup of the exact-image kernel's plain launch (k_map_rimg_blockmin_run) takes for its keyframe: 1 .. 16, or 0 (not given) = 2, halved for launches that would keep fewer than 16384 workgroups (4 is 2 % faster on the lot workload's full-map launches and slower than the one-tile kernel on the street's plain launches; 1, 8 and 16 slower on both, profiles/blockmin_tile_run_ab_kernels.txt)
    int map_tile_persist = 1;     // LTM_MAP_TILE_PERSIST  0: that kernel's tables (pixel owners, range bounds, minima) are flushed and reset behind every tile of a run (A/B form: 9.06 against 8.55 ms)
    int map_tile_barrier = 0;     // LTM_MAP_TILE_BARRIER  1: a barrier between a tile's phase 1a and 1b in that kernel (A/B form: 8.55 against 8.34 ms per full-map launch)
    int stats_blockmin = 0;      // LTM_STATS_BLOCKMIN  ltm_debug_cull_stats reports the exact-image kernel's survivor counts instead of the vote kernel's
    float reproject_twin_min_shared = 0.75f;   // LTM_REPROJECT_TWIN_MIN_SHARED  ltm_reproject_twin projects the shared points once when they are at least this share of the larger map (break-even is near 0.5: the twin costs about (shared + both rests) / one map plain passes)
};
// transformGlobalMapToLocal + map2RangeImg: map_img[(kf-kb)*npx+px] = min (range_bits<<32 | idx)
// inv_poses_dev: 12 doubles per keyframe (3x4 row-major).  b2l: 12 doubles, b2l_identity skips the arithmetic.
hipError_t map_range_images(const float4* map, size_t M, const double* inv_poses_dev, const float* approx_poses_dev, size_t kb, size_t nb,
                            HostMat34 b2l, int b2l_identity, Geom g, uint64_t* map_img, hipStream_t s, const KernelOpts& ko);
// occlusion cull of the exact-image kernel on large maps (see ltm_kernels.hip): pair t = tile * nb + keyframe.  flags: n_tiles * nb bytes,
// done: n_tiles * nb zeroed bytes, pos / list: n_tiles * nb uint32, count: one uint32, cmax: nb * rows * ceil(cols/8) uint32, temp: scan_temp_bytes(n_tiles * nb)
hipError_t occlusion_shell_pairs(const float* approx_poses_dev, size_t kb, size_t nb, const float* tile_bounds_dev, size_t n_tiles, Geom g, float r_lo, float r_hi,
                                 const uint64_t* img, int use_cmax, uint32_t* cmax, uint8_t* done, uint8_t* flags, uint32_t* pos, uint32_t* list, uint32_t* count,
                                 void* temp, size_t temp_bytes, hipStream_t s, uint32_t* dirty_rows = nullptr,
                                 const float* sub_bounds_dev = nullptr, uint8_t* submask = nullptr, unsigned long long* sub_stats = nullptr);   // submask[pair]: live 1024-point quarters of the tile (bit q), sub_stats: {quarters of live pairs, quarters left alive}
hipError_t map_range_images_pairs(const float4* map, size_t M, const double* inv_poses_dev, const float* approx_poses_dev, size_t kb, size_t nb,
                                  HostMat34 b2l, int b2l_identity, Geom g, uint64_t* map_img, const uint32_t* pairs, size_t n_pairs, hipStream_t s, const KernelOpts& ko,
                                  const uint8_t* submask = nullptr);
// calcDescrepancyAndParseDynamicPointIdx over nb images; labels[idx] = 1 for flagged points
hipError_t compare_and_flag(const uint32_t* scan_img, const uint64_t* map_img, size_t n_px_total, float thr, int mode,
                            uint8_t* labels, hipStream_t s);
// vote form of the above: mode 0 may cull points that provably cannot be flagged (needs the finished scan images)
// approx_poses_dev: 16 floats per keyframe {A[9], c_hi[3], c_lo[3], ok} with p_local ~= A (p - c) (see xform_approx)
hipError_t vote_map_range_images(const float4* map, size_t M, const double* inv_poses_dev, const float* approx_poses_dev, size_t kb, size_t nb,
                                 HostMat34 b2l, int b2l_identity, Geom g, const float* qbound_img, const float* tile_bounds_dev,
                                 const uint32_t* smax_bits_dev, float thr, int mode, uint64_t* map_img, hipStream_t s, const KernelOpts& ko);
hipError_t count_live_tiles(const float* approx_poses_dev, size_t kb, size_t nb, const float* tile_bounds_dev, size_t n_tiles,
                            const uint32_t* smax_bits_dev, float thr, unsigned long long* live_dev, hipStream_t s);
// debug (ltm_debug_proj_launch): the launch constants of the projection kernels (ProjLaunch, ltm_kernels_common.h) for a map of M points and nb keyframes,
// evaluated on the host as every launch does (on_device: by one device thread instead); f / u in the order include/ltm.h documents
static constexpr int kProjLaunchFloats = 16, kProjLaunchWords = 12;
hipError_t proj_launch_debug(Geom g, HostMat34 b2l, int b2l_identity, size_t M, size_t nb, int on_device, float* f, uint32_t* u);
// (tile, keyframe) of workgroups [first_block, first_block + n) of a (tiles x keyframes) launch, 0xffffffff for a workgroup with nothing to do
void proj_launch_blocks(size_t M, size_t nb, uint32_t first_block, size_t n, uint32_t* tile, uint32_t* kf);
// the vote kernel's form of it: workgroups take runs of tile_run consecutive tiles (RunLaunch, ltm_kernels_common.h).  vote_run_blocks: workgroups with
// work, runs x keyframes.  vote_run_launch_blocks (debug, ltm_debug_vote_run_launch): (run, keyframe) of workgroups [first_block, first_block + n), the run
// length after clamping, and the grid size as its return value
size_t vote_run_blocks(size_t M, size_t nb, int tile_run);
unsigned vote_run_launch_blocks(size_t M, size_t nb, int tile_run, uint32_t first_block, size_t n, uint32_t* run, uint32_t* kf, uint32_t* run_len);
// debug (ltm_debug_vote_queue_word): u = rows, cols, rows * cols, fast path allowed, pixel-divisor magic, shift, pixel bits, largest rows * cols of the fast path;
// row / col of the pixel indices px[0 .. n) as the kernel's drain derives them
static constexpr int kVoteQueueWords = 8;
void vote_queue_word_debug(Geom g, uint32_t* u, size_t n, const uint32_t* px, uint32_t* row, uint32_t* col);
hipError_t cull_stats(unsigned long long* out2, int reset, hipStream_t s, int which_kernel);   // {survivors, points} since the last reset; 0 vote kernel, 1 exact-image kernel
hipError_t cull_check(const float* xyz_dev, size_t n, const HostMat34* T, const HostMat34* b2l, int b2l_identity, const float* approx_pose_dev,
                      Geom g, unsigned long long* bad_dev, hipStream_t s);
// n probe points on / beside the pixel-rounding boundaries of the image shape `g` (local frame, or moved into the map frame by `pose`): input of cull_check
hipError_t cull_probe_points(Geom g, size_t n, const HostMat34* pose, float* xyz_dev, hipStream_t s);
// generic single image with up to two explicit transforms (debug / parity)
hipError_t single_range_image(const float4* pts, size_t n, const HostMat34* T1, const HostMat34* T2, Geom g,
                              uint64_t* img, hipStream_t s);
hipError_t decode_image(const uint64_t* img, size_t npx, float* rimg, int32_t* ptidx, hipStream_t s);
// ltm_reproject_twin: img_a holds the exact image of the shared cloud (S indices); afterwards img_a carries map A's indices (s2a) and img_b map B's (s2b)
hipError_t image_relabel2(uint64_t* img_a, uint64_t* img_b, size_t n_px_total, const uint32_t* s2a, const uint32_t* s2b, hipStream_t s);
// ... and the points map[list[0 .. n_list)] into the images of keyframes [kb, kb + nb) with their own map indices (the plain kernel's arithmetic)
hipError_t project_points_indexed(const float4* map, const uint32_t* list, size_t n_list, const double* inv_poses_dev, size_t kb, size_t nb, HostMat34 b2l,
                                  int b2l_identity, Geom g, uint64_t* map_img, hipStream_t s);
// RViz images: diff of a scan image (float bits) and a decoded map image; JET colour mapping of float / int32 images (BGR8)
hipError_t viz_diff(const uint32_t* scan_bits, const float* map_r, size_t n, int mode, float* out, hipStream_t s);
hipError_t viz_colormap_f32(const float* src, size_t n, float a, float b, const uint8_t* lut, uint8_t* bgr, hipStream_t s);
hipError_t viz_colormap_i32(const int32_t* src, size_t n, double a, double b, const uint8_t* lut, uint8_t* bgr, hipStream_t s);
hipError_t debug_project(const float* xyz_dev, size_t n, Geom g, float* az_el_r, int32_t* row_col, hipStream_t s);
// exhaustive device self-check of the fast arithmetic forms against their exact definitions for (vfov, hfov):
// counts[0] rad2deg mismatches, counts[1] /vfov mismatches, counts[2] /hfov mismatches over all 2^32 binary32 inputs
hipError_t selfcheck_fast_math(float vfov, float hfov, unsigned long long* counts_dev, hipStream_t s);

// ---- compaction helpers (prefix sums via rocPRIM) ----
size_t scan_temp_bytes(size_t n);
// exclusive scan of (labels[i] != 0) into pos[i] (uint32); temp from scan_temp_bytes(n)
hipError_t exclusive_scan_u8(const uint8_t* labels, uint32_t* pos, size_t n, void* temp, size_t temp_bytes, hipStream_t s);
// exclusive scan of ((uint32)img[i] != 0)
hipError_t exclusive_scan_img_valid(const uint64_t* img, uint32_t* pos, size_t n, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t exclusive_scan_u32(const uint32_t* in, uint32_t* out, size_t n, void* temp, size_t temp_bytes, hipStream_t s);
// kept/flagged split in ascending index order: pos = exclusive scan of labels
hipError_t partition_scatter(const float4* in, const uint8_t* labels, const uint32_t* pos, size_t n,
                             float4* kept, float4* flagged, hipStream_t s);
// reprojection gather: out[pos[i]] = local-frame map point of pixel i (if valid)
hipError_t reproject_gather(const uint64_t* img, const uint32_t* pos, size_t npx, size_t nb, const float4* map,
                            const double* inv_poses_dev, size_t kb, HostMat34 b2l, int b2l_identity,
                            float4* out, hipStream_t s);
// gather arbitrary positions of a u32 array: out[j] = (idx[j] < n ? in[idx[j]] : tail)
hipError_t image_bounds(const uint32_t* pos, const uint64_t* img, size_t npx, size_t nb, uint32_t* out, hipStream_t s);
hipError_t flag_bounds(const uint32_t* pos, const uint8_t* flag, size_t n, const uint64_t* offsets_dev, size_t kf0, uint64_t first, size_t nb,
                       uint32_t* out, hipStream_t s);
hipError_t gather_u32(const uint32_t* in, const uint64_t* idx_dev, size_t m, size_t n, uint32_t tail_value_index_n,
                      uint32_t* out, hipStream_t s);

// ---- transforms ----
// out[i] = xform(second, xform(first, in[i])) with per-keyframe `second` (merge: first=L2B, second=pose[kf])
hipError_t transform_cloud(const float4* in, size_t n, const HostMat34* t1, const HostMat34* t2, float4* out, hipStream_t s);   // one or two rigid transforms of a cloud
hipError_t transform_scans(const float4* in, const uint64_t* offsets_dev, size_t n_kf, uint64_t n_pts,
                           HostMat34 first, int first_identity, const double* per_kf_dev, float4* out, hipStream_t s);
// out[k] = a[k] ++ b[k] ++ c[k] per keyframe; c (and oc) may alias b with an all-zero-length offsets array
hipError_t zip_concat(const float4* a, const uint64_t* oa, const float4* b, const uint64_t* ob, const float4* c, const uint64_t* oc,
                      const uint64_t* out_off_dev, size_t n_kf, uint64_t n, float4* out, hipStream_t s);
hipError_t preclean_flags(const float4* in, uint64_t n, float radius, uint8_t* keep, hipStream_t s);

// ---- voxel centroid ----
// bbox: 8 device words, initialised by bbox_init: min xyz, max xyz as ordered keys (ordered_unkey of ltm_device_prims.h gives the floats back), two extra words
hipError_t bbox_init(uint32_t* bbox, hipStream_t s);
hipError_t bbox_reduce(const float4* pts, size_t n, uint32_t* bbox, hipStream_t s);
struct OctreeFrame { double minx, miny, minz, res; unsigned depth; };
hipError_t bbox_reduce_check(const float4* pts, size_t n, OctreeFrame cached_frame, uint32_t* bbox8, hipStream_t s);   // box + "strictly increasing codes under cached_frame" (bbox8[6] = 1 if not)
size_t voxel_heads_starts_temp_bytes(size_t n);
hipError_t voxel_heads_starts(const uint64_t* sorted_keys, size_t n, unsigned shift, uint32_t* starts, void* temp, uint32_t* total_out_dev, hipStream_t s);
hipError_t morton_keys(const float4* pts, size_t n, OctreeFrame f, uint64_t* keys, uint32_t* idx, hipStream_t s);
// scan-set (segmented) forms: one bbox / octree frame per keyframe, composite sort key (kf << shift) | morton
hipError_t bbox_reduce_seg(const float4* pts, const uint64_t* offsets_dev, size_t n_kf, uint64_t n, uint32_t* bbox, hipStream_t s);
hipError_t morton_keys_seg(const float4* pts, const uint64_t* offsets_dev, size_t n_kf, uint64_t n, const OctreeFrame* frames_dev,
                           unsigned shift, uint64_t* keys, uint32_t* idx, hipStream_t s);
// pcl::VoxelGrid of the session loader for every keyframe of a scan set (Session.cpp:284-289): per-keyframe frame computed on the host
struct VoxelGridFrame { float inv; int min_b[3]; int div_b[3]; int passthrough; };
hipError_t voxelgrid_keys_seg(const float4* pts, const uint64_t* offsets_dev, size_t n_kf, uint64_t n, const VoxelGridFrame* frames_dev,
                              uint64_t* keys, uint32_t* idx, hipStream_t s);
hipError_t voxelgrid_centroids(const float4* pts, const uint64_t* sorted_keys, const uint32_t* sorted_idx, const uint32_t* starts,
                               const VoxelGridFrame* frames_dev, size_t n_vox, size_t n, float4* out, hipStream_t s);
size_t sort_temp_bytes(size_t n);
hipError_t scan_total_to(const uint8_t* flags, const uint32_t* pos, size_t n, uint32_t* out_dev, hipStream_t s);
hipError_t sort_pairs_u64(const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* val_in, uint32_t* val_out, size_t n,
                          unsigned end_bit, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t head_flags(const uint64_t* keys, size_t n, uint8_t* heads, hipStream_t s, unsigned shift = 0);   // compares keys >> shift
// Order-preserving compression of the Morton code: bit positions that are a FUNCTION OF MORE SIGNIFICANT BITS for every key the
// cloud can produce never decide a comparison and are left out (fewer radix passes).  With the octree box centred on the data, an
// axis whose extent is well below the cube's side has its second, third ... bits tied to its top bit (z of a 10 m high map in a
// 205 m cube: 4 of 12 bits).  The kept positions are given as up to kMaxKeyRuns runs of consecutive bits: out |= ((code >> src) & mask) << dst.
static constexpr int kMaxKeyRuns = 24;
struct KeyCompress { int n_runs; unsigned bits; unsigned char src[kMaxKeyRuns], dst[kMaxKeyRuns]; uint64_t mask[kMaxKeyRuns]; };
// packed voxel path: (compressed Morton << idx_bits) | index in one word, keys-only sort over the code bits
hipError_t morton_keys_packed(const float4* pts, size_t n, OctreeFrame f, KeyCompress kc, unsigned idx_bits, uint64_t* keys, hipStream_t s);
size_t sort_keys_temp_bytes(size_t n);
hipError_t sort_keys_u64(const uint64_t* keys_in, uint64_t* keys_out, size_t n, unsigned begin_bit, unsigned end_bit, void* temp,
                         size_t temp_bytes, hipStream_t s);
hipError_t voxel_centroids_packed(const float4* pts, const uint64_t* sorted_keys, uint64_t idx_mask, const uint32_t* starts, size_t n_vox,
                                  size_t n, float4* out, hipStream_t s);
hipError_t compact_keys(const uint64_t* keys, const uint8_t* flags, const uint32_t* pos, size_t n, uint64_t* keys_out, hipStream_t s);
// sharded voxel grid: 4096-bin histogram of (key >> shift), range flags, order-preserving compaction of (key, index)
static constexpr int kVoxelKeyBins = 4096;
hipError_t key_histogram(const uint64_t* keys, size_t n, unsigned shift, uint32_t* hist, hipStream_t s);
hipError_t key_range_flags(const uint64_t* keys, size_t n, uint64_t lo, uint64_t hi, uint8_t* flags, hipStream_t s);
hipError_t compact_pairs(const uint64_t* keys, const uint32_t* idx, const uint8_t* flags, const uint32_t* pos, size_t n,
                         uint64_t* keys_out, uint32_t* idx_out, hipStream_t s);
// starts[u] = j for every head j (u = pos[j])
hipError_t segment_starts(const uint8_t* heads, const uint32_t* pos, size_t n, uint32_t* starts, hipStream_t s);
hipError_t voxel_centroids(const float4* pts, const uint32_t* sorted_idx, const uint32_t* starts, size_t n_vox, size_t n,
                           float4* out, hipStream_t s);
// join of two grids of one frame (ltm_reproject_twin; see ltm_k_voxel.hip): codes of a cloud, the match of A's points in B (flag_b zeroed by the caller),
// the check of the pairing after both flag arrays were scanned (counts3 zeroed by the caller: shared in A, matched in B, out-of-order pairs), the tables
hipError_t octree_codes(const float4* pts, size_t n, OctreeFrame f, uint64_t* codes, hipStream_t s);
hipError_t twin_join(const float4* a, size_t na, const float4* b, const uint64_t* codes_b, size_t nb, OctreeFrame f, uint8_t* flag_a, uint32_t* match,
                     uint8_t* flag_b, hipStream_t s);
hipError_t twin_join_check(const uint8_t* flag_a, const uint32_t* pos_a, const uint32_t* match, size_t na, const uint8_t* flag_b, const uint32_t* pos_b,
                           size_t nb, uint32_t* counts3, hipStream_t s);
hipError_t twin_tables(const float4* pts, const uint8_t* flag, const uint32_t* pos, size_t n, float4* shared, uint32_t* s2own, uint32_t* only, hipStream_t s);

// ---- kNN ----
struct KnnGrid { double ox, oy, oz, inv_cell; long long nx, ny, nz; };
hipError_t cell_keys(const float4* pts, size_t n, KnnGrid g, uint64_t* keys, uint32_t* idx, hipStream_t s);
hipError_t gather_points(const float4* in, const uint32_t* idx, size_t n, float4* out, hipStream_t s);
hipError_t gather_u64(const uint64_t* in, const uint32_t* idx, size_t n, uint64_t* out, hipStream_t s);      // out[i] = in[idx[i]]
struct HashEntry { uint64_t key; uint32_t start, end; };
hipError_t hash_build(const uint64_t* sorted_keys, const uint32_t* starts, size_t n_cells, size_t n_pts,
                      HashEntry* table, uint32_t table_mask, hipStream_t s);
// queries in scan sets: g = pose*(first*p) ; label = coexist ; local = b2l*(inv*g)
hipError_t knn_query_scans(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t ke, uint64_t first_pt, uint64_t n_pts, uint64_t max_kf_pts,
                           const double* poses_dev, const double* inv_poses_dev, HostMat34 b2l, int b2l_identity,
                           const float4* sorted_target, size_t Mt, KnnGrid g, const HashEntry* table, uint32_t table_mask,
                           int k, float thr, float cell2_lo, uint8_t* coexist, float4* local_out, hipStream_t s);
// two-phase form for k <= 4 (see ltm_kernels.hip): 64-byte buckets of quantised cell points decide "certainly coexist", the rest is
// compacted and searched exactly.  buckets: n_buckets x 64 bytes, initialised to 0xff; pos / queue: n_pts uint32 each; count: one uint32
hipError_t knn_bucket_build(const float4* sorted_target, const uint64_t* sorted_keys, const uint32_t* starts, size_t n_cells, size_t n_pts, KnnGrid g,
                            void* buckets, uint32_t n_buckets, hipStream_t s);
// sparse occupancy bitmap of the grid (4 x 4 x 4 cells per hashed 64-bit word): word_mask + 1 zeroed uint64 words (a power of two); lets the
// exact search skip empty cells
hipError_t knn_bitmap_build(const uint64_t* sorted_keys, const uint32_t* starts, size_t n_cells, KnnGrid g, void* occ_words, uint32_t word_mask, hipStream_t s);
// phase 1: local_out for every query, coexist[i] = 1 (certainly coexist) / 0 (certainly diff: outside the grid) / 2 (undecided)
hipError_t knn_two_phase_fast(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t ke, uint64_t first_pt, uint64_t n_pts, uint64_t max_kf_pts,
                              const double* poses_dev, const double* inv_poses_dev, HostMat34 b2l, int b2l_identity, KnnGrid g, const void* buckets,
                              uint32_t n_buckets, int k, float thr, uint8_t* coexist, float4* local_out, hipStream_t s,
                              float4* gp_undecided = nullptr);      // gp_undecided[i] = the query's global point where coexist[i] == 2: phase 2 starts from it
// phase 2: the undecided queries are compacted (scan + scatter) and searched exactly; *count = their number
hipError_t knn_two_phase_exact(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t ke, uint64_t first_pt, uint64_t n_pts,
                               const double* poses_dev, HostMat34 b2l, int b2l_identity, const float4* sorted_target, size_t Mt, KnnGrid g,
                               const HashEntry* table, uint32_t table_mask, const void* bitmap, uint32_t bitmap_mask, int k, float thr, float cell2_lo, uint8_t* coexist,
                               uint32_t* pos, uint32_t* queue, uint32_t* count, void* temp, size_t temp_bytes, hipStream_t s);
// phase 2 over a queue sorted by cell id (queue word = cell id << ibits | query index): compaction, [host reads *count], sort + exact search
unsigned knn_sorted_queue_bits(KnnGrid g, uint64_t n_pts, unsigned* ibits_out);
hipError_t knn_two_phase_compact_keyed(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t ke, uint64_t first_pt, uint64_t n_pts, const double* poses_dev,
                                       HostMat34 b2l, int b2l_identity, KnnGrid g, unsigned ibits, const uint8_t* flags, uint32_t* pos, uint64_t* queue, uint32_t* count,
                                       void* temp, size_t temp_bytes, hipStream_t s, const float4* gp_undecided = nullptr);
hipError_t knn_two_phase_exact_sorted(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t ke, uint64_t first_pt, const double* poses_dev, HostMat34 b2l,
                                      int b2l_identity, const float4* sorted_target, size_t Mt, KnnGrid g, const HashEntry* table, uint32_t table_mask, const void* bitmap,
                                      uint32_t bitmap_mask, int k, float thr, float cell2_lo, uint8_t* coexist, const uint64_t* queue_in, uint64_t* queue_sorted, uint32_t n_und,
                                      unsigned ibits, unsigned kbits, void* temp, size_t temp_bytes, hipStream_t s, const float4* gp_undecided = nullptr);
hipError_t knn_query_cloud(const float4* query, size_t Q, const float4* sorted_target, size_t Mt, KnnGrid g,
                           const HashEntry* table, uint32_t table_mask, int k, float thr, float cell2_lo,
                           uint8_t* near, hipStream_t s);

// ---- exact k-NN / radius search index (ltm_k_search.hip) ----
static constexpr int kSearchLeaf = 32;          // target points per leaf of the box tree
static constexpr int kMaxSearchK = kKnnListSlots;
// Morton frame of the index: 21 bits per axis, q = floor((v - o) * scale) clamped to [0, 2^21)
struct SearchFrame { double ox, oy, oz, scale; };
// finite target points in Morton order (pts, their input indices idx, their codes keys), Mf of them, L = ceil(Mf / kSearchLeaf) leaves,
// P = L rounded up to a power of two; box: 2 float4 (lo, hi) per node of the implicit tree, nodes 1 .. 2P-1, leaf l = node P + l
struct SearchTree { const float4* pts; const uint32_t* idx; const uint64_t* keys; const float4* box; uint32_t Mf, L, P; };
// bbox8 (bbox_init): box of the finite points, bbox8[6] their number
hipError_t search_bbox(const float4* pts, size_t n, uint32_t* bbox8, hipStream_t s);
hipError_t search_keys(const float4* pts, size_t n, SearchFrame f, uint64_t* keys, uint32_t* idx, hipStream_t s);    // non-finite: key ~0
hipError_t search_tree_boxes(const float4* sorted_pts, uint32_t Mf, uint32_t L, uint32_t P, float4* box, hipStream_t s);
// queries in code order (temp: sort_temp_bytes(n)): order[j] = input index of the j-th query, keys_sorted[j] its code
hipError_t search_query_order(const float4* query, size_t n, SearchFrame f, uint64_t* keys, uint64_t* keys_sorted, uint32_t* idx, uint32_t* order,
                              void* temp, size_t temp_bytes, hipStream_t s);
// rows of k (1 <= k <= 64) at idx / d2 + input index * k
hipError_t knn_search(const float4* query, size_t n, const uint32_t* order, const uint64_t* qkeys_sorted, SearchTree t, int k,
                      int32_t* out_idx, float* out_d2, hipStream_t s);
hipError_t knn_empty_rows(size_t n, int32_t* idx, float* d2, hipStream_t s);
hipError_t radius_count(const float4* query, size_t n, const uint32_t* order, SearchTree t, float r2, uint32_t* count, hipStream_t s);
size_t     radius_scan_temp_bytes(size_t n);
// off[0..n]: exclusive scan of min(count, cap) (cap 0: no cap) and the total
hipError_t radius_offsets(const uint32_t* count, size_t n, uint32_t cap, uint64_t* off, void* temp, size_t temp_bytes, hipStream_t s);
size_t     radius_sort_temp_bytes(size_t total, size_t n);
// every hit into pairs (rows at full_off), rows sorted by (d2, index), the first out_off[q+1] - out_off[q] of each row into out_idx / out_d2
hipError_t radius_fill(const float4* query, size_t n, const uint32_t* order, SearchTree t, float r2, const uint64_t* full_off, uint64_t total_full,
                       const uint64_t* out_off, uint64_t* pairs, uint64_t* pairs_sorted, int32_t* out_idx, float* out_d2, void* temp, size_t temp_bytes, hipStream_t s);

// ---- batches (DESIGN.md "batches"): every record struct below has a BlockSpan `span`, its workgroups in the launches over the batch's owner table ----
// A cloud to be put in Morton order under a frame: src, n points; its slice [first, first + n) of the batch's keys / order / sorted points, of which the
// first n_gather sorted positions are gathered (the finite points sort in front: a non-finite point's code is ~0)
struct SegSource { SearchFrame f; const float4* src; uint64_t first; uint32_t n, n_gather; BlockSpan span; };
// every segment sorted by (key bits 0..64, not stable); offsets: n_segs + 1 slice bounds
size_t     seg_sort_pairs_temp_bytes(size_t n, size_t n_segs);
hipError_t seg_sort_pairs_u64(const uint64_t* keys, uint64_t* keys_sorted, const uint32_t* vals, uint32_t* vals_sorted, size_t n, size_t n_segs,
                              const uint64_t* offsets, void* temp, size_t temp_bytes, hipStream_t s);

// batched build (ltm_search_build_scanset): one segment per keyframe, kSearchSegChunk points per workgroup.  n_gather is Mf, the number of finite points;
// f, n_gather, L, P and box0 (first float4 of its tree in the batch's box array) are filled in by the host once the boxes are known
static constexpr int kSearchSegChunk = 1024;    // points per workgroup of the segmented build kernels
struct SearchSeg : SegSource { uint64_t box0; uint32_t L, P; };
// bbox8: 8 words per segment (initialised here): box of its finite points as ordered keys, word 6 their number; one commit per workgroup and segment
hipError_t search_bbox_seg(const SearchSeg* segs, size_t n_segs, const uint32_t* block_seg, uint32_t n_blocks, uint32_t* bbox8, hipStream_t s);
// keys[first + j] = code of point j under its segment's frame (non-finite: ~0), idx[first + j] = j; every segment sorted by code (offsets: n_segs + 1
// slice bounds; temp: seg_sort_pairs_temp_bytes(total, n_segs)); then sorted[first + j] = src[order[first + j]] for j < n_gather
hipError_t search_order_seg(const SearchSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, size_t n_segs, const uint64_t* offsets, size_t total,
                            uint64_t* keys, uint64_t* keys_sorted, uint32_t* idx, uint32_t* order, float4* sorted, void* temp, size_t temp_bytes, hipStream_t s);
// the box trees of all segments in one launch (one workgroup per segment): box + box0 of a segment is what search_tree_boxes gives for its points
hipError_t search_tree_boxes_seg(const SearchSeg* segs, size_t n_segs, const float4* sorted, float4* box, hipStream_t s);

// ---- normals of the target points of search indices (ltm_k_normals.hip; include/ltm.h "normals") ----
static constexpr int kNormalsBlockReg = 256;    // target points per workgroup, lists in registers (k <= 16)
static constexpr int kNormalsBlockLds = 64;     // ... lists in LDS (16 < k <= 64): one wavefront
static constexpr int kNormalsMaxK = kKnnListSlots;
// one index of the batch: its tree, where its Mf normals go (aligned with t.pts), the viewpoint; normals_block(k) target points per workgroup
struct NormalsSeg { SearchTree t; float4* out; double vp[3]; BlockSpan span; };
int        normals_block(int k);                // target points per workgroup of the kernel that k selects
// out[j] = (nx, ny, nz, curvature) of target point t.pts[j] from its min(k, Mf) nearest target points, for every index of the table in one launch
hipError_t estimate_normals(const NormalsSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, int k, hipStream_t s);

// ---- Euclidean clusters over the targets of search indices (ltm_k_cluster.hip; include/ltm.h "clusters") ----
static constexpr int kClusterBlock = 256;       // finite target points per workgroup of the per-point kernels
static constexpr int kClusterChunk = 256;       // points per partial sum of a cluster's centroid
// one listed index of the batch: its tree, its slice [fbase, fbase + Mf) of the batch's per-finite-point arrays (parent, root, size, ...), its slice
// [tbase, tbase + n_target) of the labels, log2 of its tree's P
struct ClusterSeg { SearchTree t; uint64_t fbase, tbase; uint32_t n_target, logP; BlockSpan span; };
// init (every position its own root, clique leaves united), hook pass, flatten (root[], size and lowest original index per root); stats6 += pairs tested,
// edges found, leaves visited, clique leaves among them, clique early exits, hook retries
hipError_t cluster_hook(const ClusterSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, float r2, int clique_on, uint32_t* parent, uint32_t* root,
                        uint32_t* size, uint32_t* minidx, int32_t* cid, unsigned long long* stats6, hipStream_t s);
// keep[i] = 1 for the roots whose component has min_size <= size <= max_size; counts[2 k], counts[2 k + 1] += clusters and clustered points of index k
hipError_t cluster_roots(const ClusterSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, const uint32_t* root, const uint32_t* size, uint32_t min_size,
                         uint32_t max_size, uint8_t* keep, unsigned long long* counts, hipStream_t s);
size_t     cluster_temp_bytes(size_t n_clusters, size_t n_segs);
// the kept roots (pos: exclusive scan of keep) sorted per index by (size descending, lowest original index): cluster c of the batch, c in [coff[k], coff[k + 1])
// for index k.  cid[root position] = c; csize / cfirst / cseg / cchunks per cluster (csize, cchunks: n_clusters + 1 entries), goff / choff their exclusive scans
hipError_t cluster_number(const uint8_t* keep, const uint32_t* pos, size_t total, const uint32_t* size, const uint32_t* minidx, uint32_t n_clusters,
                          const uint64_t* coff, uint32_t n_segs, uint64_t* keys, uint64_t* keys_sorted, uint32_t* vals, uint32_t* vals_sorted, int32_t* cid,
                          uint32_t* csize, int32_t* cfirst, uint32_t* cseg, uint32_t* cchunks, uint32_t* goff, uint32_t* choff, void* temp, size_t temp_bytes,
                          hipStream_t s);
// labels[tbase + original index] = cluster number inside its index (the caller filled -1); keys / vals: every clustered point as (cluster << 32 | original
// index, global position), unordered; cursor: one word
hipError_t cluster_labels(const ClusterSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, const uint32_t* root, const int32_t* cid, const uint64_t* coff,
                          int32_t* labels, uint64_t* keys, uint32_t* vals, uint32_t* cursor, hipStream_t s);
inline size_t cluster_max_chunks(size_t n_clusters, size_t n_points) { return n_points / kClusterChunk + n_clusters; }      // >= sum of ceil(size / kClusterChunk)
// from the sorted (cluster, original index) keys: the CSR point indices, and per cluster size, lowest index, box, centroid; offsets_out: n_clusters + n_segs
// entries zeroed by the caller, index k's n_k + 1 offsets at coff[k] + k.  psum / pbox: 3 doubles / 6 words per cluster_max_chunks(n_clusters, n_points)
hipError_t cluster_finish(const ClusterSeg* segs, const uint64_t* keys_sorted, const uint32_t* vals_sorted, uint32_t n_clusters, size_t n_points, const uint32_t* csize,
                          const int32_t* cfirst, const uint32_t* cseg, const uint32_t* goff, const uint32_t* choff, const uint64_t* coff, double* psum, uint32_t* pbox,
                          int32_t* idx_out, uint32_t* sizes_out, int32_t* first_out, float* box_out, double* centroid_out, uint64_t* offsets_out, hipStream_t s);

// ---- RANSAC plane segmentation of records of points (ltm_k_plane.hip; include/ltm.h "planes") ----
static constexpr int kPlaneBlock = 256;                                      // threads per workgroup of the per-point kernels
static constexpr int kPlanePointsPerThread = 8;                              // points a thread of the count kernel keeps in registers
static constexpr int kPlaneBlockPoints = kPlaneBlock * kPlanePointsPerThread;   // points of one record per workgroup (LTM_PLANE_BLOCK_POINTS)
static constexpr int kPlaneChunk = 256;                                      // points per partial record of the moments: the chunk of "clusters"
static constexpr int kPlaneMaxIterations = 4096;                             // counters of a workgroup in LDS
static constexpr int kPlaneMoments = 9;                                      // doubles per partial record: sum d (3), sum d d^T (xx xy xz yy yz zz)
// one record of the batch: its n points, base = its first point among the call's points (labels), its first chunk among the batch's partial records
// (ceil(n / kPlaneChunk) of them); kPlaneBlockPoints points per workgroup
struct PlaneRec { const float4* pts; uint64_t base; uint32_t n, chunk0; BlockSpan span; };
// one hypothesis: the seven values the count kernel reads (N, p0, T; T = 0 where the hypothesis is invalid) in a 64-byte row
struct PlaneHyp { double N[3], p0[3], T, pad; };
// what a record ends with (ltm_planes_download)
struct PlaneOut { double coeff[4], point[3]; int32_t best; uint32_t consensus, n_valid, n_inliers; uint8_t found, refined, pad[6]; };
struct PlaneLaunch { double thr, axis[3], c2; uint32_t max_iterations, seed; int constrained, has_axis, refine; };
static_assert(sizeof(PlaneRec) == 32 && sizeof(PlaneHyp) == 64 && sizeof(PlaneOut) == 80, "the plane records keep their sizes");
// The fixed launch sequence of ltm_scanset_segment_planes for n_recs records (out zeroed, counts zeroed by the caller): hypotheses, counts, best, moments
// and combine (refine only), labels.  hyp / valid / counts: n_recs x max_iterations; partials: kPlaneMoments doubles per chunk; labels[base + i]: point i
// of a record; stats4 += point-hypothesis tests, valid hypotheses, records, records refined
hipError_t plane_segment(const PlaneRec* recs, const uint32_t* block_rec, uint32_t n_blocks, uint32_t n_recs, const PlaneLaunch& L, PlaneHyp* hyp, uint8_t* valid,
                         uint32_t* counts, double* partials, PlaneOut* out, uint8_t* labels, unsigned long long* stats4, hipStream_t s);

// ---- outlier filters over the targets of search indices (ltm_k_outlier.hip; include/ltm.h "outlier filters") ----
static constexpr int kOutlierBlock = 256;       // finite target points per workgroup: distance lists in registers (at most 16 slots), radius counts
static constexpr int kOutlierBlockLds = 64;     // ... distance lists in LDS (17 .. 64 slots): one wavefront
static constexpr int kOutlierMaxSlots = kKnnListSlots;     // mean_k + 1 at most: the limit of ltm_knn_search
static constexpr int kOutlierChunk = 256;       // original positions per partial sum of the record statistics: the chunk of "clusters"
// one listed index of the batch: its tree, its slice [tbase, tbase + n_target) of the call's per-position arrays (labels, distances or counts); span: its
// workgroups over its finite points, tspan: its chunks (tspan.block0 is its first chunk among the call's partial sums)
struct OutlierSeg { SearchTree t; uint64_t tbase; uint32_t n_target, pad; BlockSpan span, tspan; };
// what a record ends with: the statistics (statistical filter; zeros for the radius filter) and the labels set
struct OutlierRec { double mean, stddev, threshold; uint32_t n_kept, pad; };
static_assert(sizeof(OutlierRec) == 32, "the outlier record keeps its size");
int        outlier_sor_block(int mean_k);       // finite points per workgroup of the distance kernel that mean_k selects
// The fixed launch sequence of ltm_search_filter_statistical for n_recs indices (dist and labels zeroed by the caller): rows, distances, moments, combine,
// labels.  block_seg: the owner table over finite points, outlier_sor_block(mean_k) per workgroup; chunk_seg: the owner table over chunks; partials: two
// doubles per chunk; stats4 += finite points, distance evaluations, (radius walks stopped early,) records
hipError_t outlier_statistical(const OutlierSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, const uint32_t* chunk_seg, uint32_t n_chunks, uint32_t n_recs,
                               int mean_k, double stddev_mul, float* dist, double* partials, OutlierRec* out, uint8_t* labels, unsigned long long* stats4,
                               hipStream_t s);
// ltm_search_filter_radius (counts and labels zeroed by the caller): rows, counts.  block_seg: kOutlierBlock finite points per workgroup
hipError_t outlier_radius(const OutlierSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, uint32_t n_recs, float r2, uint32_t min_neighbors,
                          uint32_t* counts, OutlierRec* out, uint8_t* labels, unsigned long long* stats4, hipStream_t s);

// ---- FPFH descriptors over the targets of search indices (ltm_k_fpfh.hip; include/ltm.h "fpfh") ----
static constexpr int kFpfhBlock = 256;          // finite target points per workgroup: lists in registers (k <= 16), and the threads of the fill
static constexpr int kFpfhBlockLds = 64;        // ... lists in LDS (16 < k <= 64): one wavefront
static constexpr int kFpfhMaxK = kKnnListSlots;
static constexpr int kFpfhWords = 4;            // 64-bit words of a point's SPFH: ten 6-bit counts (bins 0 .. 9) per feature in words 0 .. 2, the pairs counted in word 3
static constexpr uint64_t kFpfhListBudget = 16ull << 30;      // bytes of pooled scratch the neighbour lists of one call may take (8 per finite point and slot)
// one listed index of the batch: its tree, its normals (aligned with t.pts), its slice [tbase, tbase + n_target) of the call's rows and [fbase, fbase + Mf)
// of the call's finite points (the stored lists)
struct FpfhSeg { SearchTree t; const float4* nrm; uint64_t tbase, fbase; uint32_t n_target, pad; BlockSpan span; };
int        fpfh_block(int k);                   // finite points per workgroup of the kernels that k selects
// The fixed launch sequence of ltm_search_fpfh (spfh zeroed by the caller): fill, SPFH, weights.  block_seg: the owner table over finite points, fpfh_block(k)
// per workgroup; spfh: kFpfhWords words per position, desc: 33 floats per position, both in the targets' original order.  list_d2 / list_idx: k x total_f
// entries each, slot-major (slot j of the call's finite point g at j * total_f + g), written by the SPFH pass and read by the weights; both NULL: the weights
// collect the neighbourhoods again.  stats4 += finite points, distance evaluations (of every collect), pairs skipped, points that took the LDS list form
hipError_t fpfh_estimate(const FpfhSeg* segs, const uint32_t* block_seg, uint32_t n_blocks, uint64_t n_points, int k, unsigned long long* spfh, float* desc,
                         float* list_d2, int* list_idx, uint64_t total_f, unsigned long long* stats4, hipStream_t s);

// ---- feature-space correspondences between descriptor records (ltm_k_sac.hip; include/ltm.h "fpfh matches") ----
static constexpr int kMatchBlock = 256;         // source rows per workgroup, one per thread, each in 33 registers
static constexpr int kMatchTileRows = 128;      // target rows staged in LDS at a time (LTM_MATCH_TILE_ROWS): 33 words per row and one flag
static constexpr int kMatchRow = 33;            // floats per descriptor row
static constexpr int kMatchMaxK = kKnnListRegSlots;
// one pair of the batch: source rows src[0 .. n_source) matched against target rows tgt[0 .. n_target), its lists at row `obase` of the call's outputs;
// kMatchBlock source rows per workgroup
struct MatchPair { const float* src; const float* tgt; uint64_t obase; uint32_t n_source, n_target; BlockSpan span; };
static_assert(sizeof(MatchPair) == 40, "the match record keeps its size");
// ltm_fpfh_match: one launch for all pairs.  idx / dist: kc slots per source row, ascending by (distance, target row), unused slots (-1, +inf)
hipError_t fpfh_match(const MatchPair* pairs, const uint32_t* block_pair, uint32_t n_blocks, int kc, int32_t* idx, float* dist, hipStream_t s);

// ---- sample-consensus initial alignment from matches (ltm_k_sac.hip; include/ltm.h "initial alignment") ----
static constexpr int kSacBlock = 256;                                        // threads per workgroup of the vote kernel
static constexpr int kSacPointsPerThread = 4;                                // voting points a thread keeps in registers
static constexpr int kSacBlockPoints = kSacBlock * kSacPointsPerThread;      // voting points of one pair per workgroup (LTM_SAC_BLOCK_POINTS)
static constexpr int kSacMaxIterations = 16384;
// one index of the call whose rows are looked up by ORIGINAL position: row[base + idx[j]] = j for its Mf sorted positions; kSacBlock positions per workgroup
struct SacRows { const uint32_t* idx; uint64_t base; uint32_t Mf, pad; BlockSpan span; };
// one pair of the batch: the two trees, their row tables (original position -> sorted position, ~0: not finite), its match lists (n_rows x kc target rows);
// n_eval voting points (sorted positions 0, stride, 2 stride, ... of the source), kSacBlockPoints per workgroup
struct SacPair { SearchTree tt, st; const uint32_t* trow; const uint32_t* srow; const int32_t* match; uint32_t n_rows, n_eval; BlockSpan span; };
// one hypothesis: rows 0 .. 2 of the transform, row-major (R | t), 12 doubles
struct SacHyp { double T[12]; };
// what a record ends with (ltm_sac_download)
struct SacOut { double T[16]; int32_t best; uint32_t consensus, n_valid, n_prerejected, n_eval; uint8_t found, pad[3]; };
struct SacLaunch { double thr2, r2, inlier_fraction; uint32_t max_iterations, seed, stride; int kc; };
static_assert(sizeof(SacRows) == 32 && sizeof(SacPair) == 136 && sizeof(SacHyp) == 96 && sizeof(SacOut) == 152, "the sac records keep their sizes");
// The fixed launch sequence of ltm_sac_align for n_pairs pairs (rows filled with ~0, counts and out zeroed by the caller): row tables, hypotheses, votes,
// best.  hyp / valid / counts: n_pairs x max_iterations.  stats4 += point-hypothesis tests, hypotheses prerejected, walks ended by a hit, records
hipError_t sac_align(const SacRows* rows, const uint32_t* block_rows, uint32_t n_row_blocks, uint32_t* row, const SacPair* pairs, const uint32_t* block_pair,
                     uint32_t n_blocks, uint32_t n_pairs, const SacLaunch& L, SacHyp* hyp, uint8_t* valid, uint32_t* counts, SacOut* out,
                     unsigned long long* stats4, hipStream_t s);

// ---- loop submaps (ltm_k_submap.hip; ltslam/src/Session.cpp:91-142, utility.cpp:80-103) ----
// one piece of the batch: n points from scans[src ...] moved by affine `affine` (12 floats each) to out[dst ...]; 256 points per workgroup
struct SubmapPiece { uint64_t src, dst; uint32_t n, affine; BlockSpan span; };
hipError_t submap_gather(const float4* scans, const SubmapPiece* pieces, const uint32_t* block_piece, uint32_t n_blocks, const float* affines12, float4* out,
                         hipStream_t s);

// ---- batched point-to-point ICP over search indices (ltm_k_icp.hip; LTslam.cpp:187-301) ----
static constexpr int kIcpBlock = 256;           // source points per workgroup of the correspondence kernel = per partial record
static constexpr int kIcpPartial = 17;          // doubles per partial record: count, sum p (3), sum q (3), sum p q^T (9, row-major), sum d2
static constexpr int kIcpPlanePartial = 29;     // point-to-plane: count, A^T A (21, upper triangle row-major), A^T b (6), sum d2
enum IcpMode { kIcpPoint = 0, kIcpScore = 1, kIcpPlane = 2, kIcpGicp = 3 };      // kIcpGicp: records of kIcpPlanePartial doubles (sum A^T M A, sum A^T M d)
// one pair of the batch: the source as given under the target's frame (SegSource; n_gather = n, kIcpBlock points per workgroup), the target's tree; o: the
// origin the moments are taken about (the corner of the target's frame); nrm: the target's normals, aligned with t.pts (point-to-plane and generalized).
// Generalized ICP reads its sources in place: src is then the source index's own points (its finite points in its own code order, n = its Mf), snrm
// their normals, and `first` is not used
struct IcpPair : SegSource { SearchTree t; double o[3]; const float4* nrm; const float4* snrm; };
// what k_icp_update keeps per pair between iterations (T: rows 0..2 of the accumulated transform, row-major)
struct IcpState { double T[12]; double prev_mse, last_mse, fitness; int32_t iterations, state, converged, done; uint32_t n_corr, pad; };
// codes of every source point under its target's frame (keys) and its position in its source (idx), every source sorted by code (offsets: n_pairs + 1
// slice bounds; temp: seg_sort_pairs_temp_bytes(total, n_pairs)), then sorted[first + j] = src[order[first + j]]
hipError_t icp_order_sources(const IcpPair* pairs, const uint32_t* block_pair, uint32_t n_blocks, size_t n_pairs, const uint64_t* offsets, size_t total,
                             uint64_t* keys, uint64_t* keys_sorted, uint32_t* idx, uint32_t* order, float4* sorted, void* temp, size_t temp_bytes, hipStream_t s);
// one record per workgroup.  mode kIcpPoint: kIcpPartial doubles, correspondences within max_corr2 of the pairs not done yet; kIcpScore: count and sum d2
// of every finite point of every pair, no limit (in a record of kIcpPartial); kIcpPlane: kIcpPlanePartial doubles, the normal equations of the
// correspondences within max_corr2 whose target normal is finite; kIcpGicp: kIcpPlanePartial doubles, the weighted normal equations of the correspondences
// within max_corr2 whose two normals are finite (gicp_w = 1 - gicp_epsilon).  sorted == nullptr (kIcpGicp, and kIcpScore after it): the points are pairs[].src
hipError_t icp_correspond(const IcpPair* pairs, const IcpState* st, const uint32_t* block_pair, uint32_t n_blocks, const float4* sorted, double max_corr2,
                          int mode, double* partials, hipStream_t s, double gicp_w = 0.0);
// per pair: partials added in block order, transform estimate (plane: the 6 x 6 solve of the kIcpPlane records), stop tests; trace (nullable):
// n_pairs x max_iterations x 2; unfinished: one counter
hipError_t icp_update(const IcpPair* pairs, IcpState* st, size_t n_pairs, const double* partials, int max_iterations, double transformation_epsilon,
                      double euclidean_fitness_epsilon, double* trace, uint32_t* unfinished, hipStream_t s, int plane = 0);
hipError_t icp_fitness(const IcpPair* pairs, IcpState* st, size_t n_pairs, const double* partials, hipStream_t s);
static_assert(sizeof(SearchSeg) == 80 && sizeof(NormalsSeg) == 88 && sizeof(ClusterSeg) == 80 && sizeof(SubmapPiece) == 32 && sizeof(IcpPair) == 152,
              "the batch records keep their sizes");

// ---- scan context (ltm_k_scancontext.hip; Scancontext.cpp:69-324) ----
struct ScGeom { double lidar_height, max_radius; int R, S; };      // rings x sectors
// which kernel forms a shape gets (host arithmetic, the launch wrappers' own decisions): sc_scatter pre-reduces in LDS, sc_pair_distance stages both descriptors in LDS
void sc_paths(int R, int S, bool* scatter_in_lds, bool* pair_in_lds);
// makeScancontext for keyframes [kb, kb + nb): bins (zeroed by the caller, R * S uint32 per keyframe) receive the order-preserving key of the largest
// height of every bin; sc_finish turns them into the descriptor
hipError_t sc_scatter(const float4* scans, const uint64_t* offsets_dev, size_t kb, size_t nb, uint64_t max_kf_pts, ScGeom g, uint32_t* bins, hipStream_t s);
// n descriptors (row-major R x S doubles): heights from `bins` (nullptr: desc is given), ring keys (n x R float), sector keys and column norms (n x S double)
hipError_t sc_finish(const uint32_t* bins, size_t n, int R, int S, double* desc, float* ring_keys, double* sector_keys, double* norms, hipStream_t s);
// rd[q * nd + j] = nanoflann L2 distance (float) between ring key q of the queries and ring key j of the database
hipError_t sc_ring_distances(const float* qk, size_t nq, const float* dbk, size_t nd, int R, float* rd, hipStream_t s);
// pairs[(q * K + k) * 2] = {q, the k-th nearest database entry of query q by (rd, index)}; 1 <= K <= nd
hipError_t sc_candidates(const float* rd, size_t nq, size_t nd, int K, int32_t* pairs, hipStream_t s);
// (distance, shift) of distanceBtnScanContext(A[i], B[j]) for n_pairs (< 2^31) pairs (i, j) = pairs[2p], pairs[2p + 1], or (p / nd, p % nd) if pairs is null;
// radius: half-width of the shift search space around the sector-key alignment (>= S / 2: every shift)
hipError_t sc_pair_distance(const double* descA, const double* skA, const double* nrmA, const double* descB, const double* skB, const double* nrmB, int R, int S,
                            const int32_t* pairs, size_t nd, size_t n_pairs, int radius, double* dist, int32_t* shift, hipStream_t s);
// per query the best of its K consecutive pairs (candidate index pairs[2p + 1], or k if pairs is null): smallest distance, then (rd, index)
hipError_t sc_detect_reduce(const double* dist, const int32_t* shift, const int32_t* pairs, const float* rd, size_t nq, size_t nd, size_t K,
                            int32_t* nn_idx, double* min_dist, int32_t* nn_align, hipStream_t s);

} // namespace ltm
