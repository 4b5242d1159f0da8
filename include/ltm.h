/*
 * ltm.h -- C ABI of libltm_hip.so: the MI355X (gfx950) implementation of the LT-removert /
 * LT-map hot path of gisbi-kim/lt-mapper (package `removert`).
 *
 * The reference has no plugin/FFI boundary: Removerter/Session are
 * monolithic C++ classes.  This header is the boundary a maintainer binds instead of the
 * PCL/OpenCV/OpenMP bodies of the functions cited on each entry point below; the host-side
 * mirror of the class surface that calls it lives in lt-mapper_amd/host/ (C++) and
 * the ctypes binding lt-mapper_amd/capi.py (used by the tests and bench.py).  INTEGRATION.md shows the
 * reference-side patch.
 *
 * Conventions
 *  - C linkage, POD only, no torch/PCL/Eigen types.  Every call returns LTM_OK (0) or a
 *    negative LTM_E_* code; the library never throws and never exits.  ltm_last_error()
 *    gives the message for the last failing call on that context.
 *  - A context owns one HIP stream and all device memory reachable through its handles.
 *    Calls on ONE context serialise on a mutex of that context, so a handle may be freed from any
 *    thread; the pipeline of one context is still driven from one host thread (as the reference's
 *    run() is).  Independent chains of a run -- the two sessions' remove / revert passes
 *    (Removerter.cpp:1580-1587), the ND and PD filters (:1395-1411), the reprojections of Step 3
 *    (:1534-1575) -- may run side by side on LANES: further contexts on the same device, one host
 *    thread each, that exchange clouds without copies (section "lanes" below).
 *  - Clouds are XYZI float32, 16 B / point on the device.  Host buffers are described by a
 *    byte stride (16 = packed, 32 = pcl::PointXYZI: xyz+pad, intensity+pad).
 *  - Matrices are 4x4 row-major double (the layout of the pose text files, Session.cpp:102-114).
 *  - The library never keeps a host pointer after a call returns.  Calls are synchronous
 *    with respect to the host unless stated otherwise.
 *  - There is no CPU fallback: without a usable gfx950 device ltm_create() fails.
 */
#ifndef LTM_H
#define LTM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LTM_ABI_VERSION 1

enum {
    LTM_OK = 0,
    LTM_E_INVALID = -1,    /* bad argument / bad handle */
    LTM_E_DEVICE = -2,     /* HIP runtime error, no device */
    LTM_E_NOMEM = -3,      /* device or host allocation failed */
    LTM_E_UNSUPPORTED = -4 /* outside the supported domain (e.g. octree depth > 21) */
};

typedef struct ltm_ctx ltm_ctx;
typedef uint64_t ltm_cloud;   /* device-resident XYZI cloud; 0 is never a valid handle */
typedef uint64_t ltm_scanset; /* N per-keyframe clouds packed in one device array + offsets[N+1] */
typedef uint64_t ltm_poses;   /* N keyframe poses + inverse poses (double, device + host copy) */

/* RosParamServer.cpp:15-33 -- the parameters the hot path reads */
typedef struct {
    float  vfov, hfov;        /* removert/sequence_vfov, sequence_hfov (defaults 50, 360) */
    double lidar2base[16];    /* removert/ExtrinsicLiDARtoPoseBase; its inverse is derived inside */
    int    device;            /* HIP device ordinal (LOCAL_RANK for multi-process runs) */
    int    max_kf_batch;      /* keyframes whose range images are resident at once; 0 = default (512) */
} ltm_config;

int         ltm_abi_version(void);
int         ltm_create(const ltm_config* cfg, ltm_ctx** out);
void        ltm_destroy(ltm_ctx* ctx);
const char* ltm_last_error(const ltm_ctx* ctx);
int         ltm_synchronize(ltm_ctx* ctx);
/* drops derived data the context keeps between calls (finished scan range images, keyed by scan set + image shape).
 * Results never depend on it; benchmarks call it so that every timed run does the work of a fresh run. */
int         ltm_clear_caches(ltm_ctx* ctx);
/* the hipStream_t every kernel of this context is launched on (for events / interop) */
void*       ltm_stream(ltm_ctx* ctx);

/* ------------------------------------------------------------------ clouds ---- */
int ltm_cloud_upload(ltm_ctx*, const void* pts, size_t n, size_t stride_bytes, ltm_cloud* out);
int ltm_cloud_from_device(ltm_ctx*, const void* dev_xyzi, size_t n, ltm_cloud* out);  /* D2D copy of packed float4 */
int ltm_cloud_size(ltm_ctx*, ltm_cloud, size_t* n);
int ltm_cloud_download(ltm_ctx*, ltm_cloud, void* dst, size_t cap_pts, size_t stride_bytes);
int ltm_cloud_device_ptr(ltm_ctx*, ltm_cloud, const void** dev_xyzi);                 /* borrowed, valid until free */
int ltm_cloud_clone(ltm_ctx*, ltm_cloud, ltm_cloud* out);                              /* `*a = *b` deep copies */
/* A cloud that came out of ltm_voxel_centroid[_batch] remembers the octree frame it was gridded under; ltm_cloud_clone, ltm_cloud_lend / _give and the
 * kept / flagged parts of a partition keep it.  Writing the array behind ltm_cloud_device_ptr in place does NOT drop it: the cloud keeps the frame it was
 * gridded under.  That is safe because ltm_voxel_centroid never trusts the frame: every call re-derives the frame from the points' bounding box and
 * re-checks, point by point, that the cloud still is its own grid under it (codes strictly increasing, no -0.0) before it answers with a copy; rows
 * swapped, duplicated or overwritten are gridded in full (tests/test_gpu_voxel_edges.py, the stale-frame cases). */
int ltm_cloud_concat(ltm_ctx*, const ltm_cloud* in, size_t n, ltm_cloud* out);         /* `*a += *b` (order kept) */
/* pcl::transformPointCloud(cloud, out, Matrix4d) applied once or twice (row-major 4x4, NULL = skip), the float result of the first
 * being the input of the second: local2global = (T1 = lidar->base, T2 = pose), global2local / transformGlobalMapToLocal =
 * (T1 = inverse pose, T2 = base->lidar)  (utility.cpp:64-72, 160-168, 194-202) */
int ltm_cloud_transform(ltm_ctx*, ltm_cloud in, const double* T1, const double* T2, ltm_cloud* out);
/* pcl::ExtractIndices as used by parsePointcloudSubsetUsingPtIdx (Removerter.cpp:933-946): out[j] = in[idx[j]], order kept;
 * an index outside [0, n) is LTM_E_INVALID (undefined behaviour in the reference) */
int ltm_cloud_select(ltm_ctx*, ltm_cloud in, const int32_t* idx_host, size_t n_idx, ltm_cloud* out);
int ltm_cloud_free(ltm_ctx*, ltm_cloud);

/* an UNINITIALISED cloud of n points whose device array (ltm_cloud_device_ptr) a collective fills: the all-gather that assembles a
 * map from per-rank pieces writes straight into it (north_star: "RCCL all-gather over xGMI to assemble the final maps") */
int ltm_cloud_alloc(ltm_ctx*, size_t n, ltm_cloud* out);

/* ---------------------------------------------------------------- scan sets ---- */
/* keyframe_scans_ and friends (Session.h:41-58): offsets[n_kf+1] in points */
int ltm_scanset_upload(ltm_ctx*, const void* pts, size_t stride_bytes, const uint64_t* offsets, size_t n_kf, ltm_scanset* out);
int ltm_scanset_from_device(ltm_ctx*, const void* dev_xyzi, const uint64_t* host_offsets, size_t n_kf, ltm_scanset* out);
int ltm_scanset_info(ltm_ctx*, ltm_scanset, size_t* n_kf, size_t* n_points);
int ltm_scanset_offsets(ltm_ctx*, ltm_scanset, uint64_t* offsets /* n_kf+1 */);
int ltm_scanset_keyframe(ltm_ctx*, ltm_scanset, size_t kf, ltm_cloud* out);            /* one keyframe's scan as a cloud (D2D copy) */
int ltm_scanset_download(ltm_ctx*, ltm_scanset, void* dst, size_t cap_pts, size_t stride_bytes);
int ltm_scanset_device_ptr(ltm_ctx*, ltm_scanset, const void** dev_xyzi);
int ltm_scanset_as_cloud(ltm_ctx*, ltm_scanset, ltm_cloud* out);                       /* flat copy of all points */
/* concatenate per-rank scan sets keyframe-wise (multi-GPU assembly): out has sum(n_kf) keyframes */
int ltm_scanset_concat(ltm_ctx*, const ltm_scanset* in, size_t n, ltm_scanset* out);
/* per-keyframe `a[i] += b[i] (+= c[i])` of Session.cpp:365-371 ; c may be 0 */
int ltm_scanset_zip_concat(ltm_ctx*, ltm_scanset a, ltm_scanset b, ltm_scanset c, ltm_scanset* out);
/* the same for a scan set: keyframe layout given by host offsets[n_kf+1], points uninitialised (ltm_scanset_device_ptr) */
int ltm_scanset_alloc(ltm_ctx*, const uint64_t* offsets, size_t n_kf, ltm_scanset* out);
int ltm_scanset_free(ltm_ctx*, ltm_scanset);

/* ------------------------------------------------------- raw device buffers ---- */
/* Label masks and staging areas of the multi-GPU host: pooled device memory, ordered on the context's stream
 * (ltm_stream) -- a collective enqueued on that stream needs no extra synchronisation.  ltm_buffer_copy returns when the copy
 * has completed; kind: 0 = host->device, 1 = device->host, 2 = device->device. */
int ltm_buffer_alloc(ltm_ctx*, size_t bytes, void** dev);
int ltm_buffer_free(ltm_ctx*, void* dev);
int ltm_buffer_fill(ltm_ctx*, void* dev, int byte_value, size_t bytes);            /* asynchronous on the context's stream */
int ltm_buffer_copy(ltm_ctx*, void* dst, const void* src, size_t bytes, int kind);

/* --------------------------------------------- pipelined feeder / asynchronous fetch ---- */
/* f-1 (Session.cpp:266-302): a scan set assembled from chunks of consecutive keyframes WHILE the host is still
 * decoding the next files.  Each chunk is staged through one of two pinned buffers and copied on a dedicated copy stream, so the
 * host-side packing of chunk i+1 overlaps the DMA of chunk i (and both overlap the decode threads).  capacity_points is an upper
 * bound of the total (the POINTS fields of the PCD headers).  ltm_scanset_upload_chunk returns as soon as `pts` may be reused.
 * Two-stream rule: the device array comes from the context's stream-ordered pool, so ltm_scanset_upload_begin makes the copy stream
 * wait for everything already queued on the compute stream (a recycled block may still be read by queued kernels), and
 * ltm_scanset_upload_end waits for the copies before the scan set is handed to the compute stream.  An upload may therefore be
 * started at any time, not only while the context is idle. */
typedef uint64_t ltm_upload;
int ltm_scanset_upload_begin(ltm_ctx*, size_t capacity_points, ltm_upload* up);
int ltm_scanset_upload_chunk(ltm_ctx*, ltm_upload up, const void* pts, size_t stride_bytes, const uint64_t* kf_sizes, size_t n_kf);
int ltm_scanset_upload_end(ltm_ctx*, ltm_upload up, ltm_scanset* out);

/* f-2 (Removerter.cpp:1637-1650, 1446-1520): asynchronous device->host fetch for the output writer.  *_fetch_begin enqueues the
 * copy of the cloud / scan set as it is after everything already submitted to the context, on the copy stream, into a pinned host
 * buffer owned by the library; the context keeps computing.  ltm_fetch_wait blocks until that copy has completed and may be
 * called from ANY host thread (writer threads) -- it touches only the ticket.  The points are packed XYZI (16 B); for a scan set
 * `offsets` (n_kf + 1 entries, owned by the ticket) delimit the keyframes.  The source handle must stay alive until the wait has
 * returned; ltm_fetch_release recycles the pinned buffer and may also be called from any thread, as soon as the data has been
 * consumed (page-locking new buffers is what costs time, so hand them back early). */
typedef struct ltm_fetch ltm_fetch;
int ltm_cloud_fetch_begin(ltm_ctx*, ltm_cloud, ltm_fetch** out);
int ltm_scanset_fetch_begin(ltm_ctx*, ltm_scanset, ltm_fetch** out);
int ltm_fetch_wait(ltm_fetch*, const void** host_xyzi, size_t* n_points, const uint64_t** offsets, size_t* n_kf);
int ltm_fetch_release(ltm_ctx*, ltm_fetch*);
/* Chunked form of the same: nothing the size of an output is page-locked.  The context keeps a small ring of pinned chunks
 * (8 x 32 MB; LTM_FETCH_SLOTS, LTM_FETCH_CHUNK_MB) and a copier thread that, once the compute stream has reached the point of the
 * *_fetch_chunks_begin call, moves the points chunk by chunk into free ring slots.  Consumers -- any number of threads per ticket
 * -- take chunks with ltm_fetch_next_chunk (blocks; 1 = a chunk, 0 = no more, < 0 = error) and hand every one back with
 * ltm_fetch_chunk_done as soon as they have used it (the copier waits for free slots, the context thread never does).  A cloud
 * comes in consecutive ranges of points; a scan set in chunks of WHOLE keyframes [first_kf, first_kf + n_kf), whose points start
 * at offsets[first_kf] - first_point inside the chunk (LTM_E_INVALID from *_begin if one keyframe is larger than a chunk).
 * ltm_fetch_info gives the totals right away (a writer needs them for its header).
 * Contract of the chunked form (the in-tree writer, host/src/Removerter.cpp, is the model):
 *  - ONE copier thread serves the tickets strictly in the order of their *_begin calls through the shared ring, so tickets must
 *    also be CONSUMED in that order: a ticket nobody drains (or consumers that all block on a later ticket) stalls every later one;
 *  - the device source (cloud / scan set handle) must stay alive and unmodified until ltm_fetch_release has returned: the copier
 *    reads it asynchronously;
 *  - call ltm_fetch_release (any thread) exactly once, after every consumer thread of the ticket has seen ltm_fetch_next_chunk
 *    return 0 or an error and has handed back its chunks: release frees the ticket, a thread still inside ltm_fetch_next_chunk
 *    would touch freed memory. */
int ltm_cloud_fetch_chunks_begin(ltm_ctx*, ltm_cloud, ltm_fetch** out);
int ltm_scanset_fetch_chunks_begin(ltm_ctx*, ltm_scanset, ltm_fetch** out);
int ltm_fetch_info(ltm_fetch*, size_t* n_points, const uint64_t** offsets, size_t* n_kf);
int ltm_fetch_next_chunk(ltm_fetch*, const void** host_xyzi, size_t* first_point, size_t* n_points, size_t* first_kf, size_t* n_kf);
int ltm_fetch_chunk_done(ltm_fetch*, const void* host_xyzi);

/* -------------------------------------------------------------------- poses ---- */
/* keyframe_poses_ / keyframe_inverse_poses_ (Session.cpp:102-114).  inv may be NULL: then the
 * inverse is ltm_inverse4x4 of every pose. */
int ltm_poses_create(ltm_ctx*, size_t n_kf, const double* poses, const double* inv_or_null, ltm_poses* out);
/* `Eigen::Matrix4d::inverse()` as the reference uses it for the poses (Session.cpp:109-110) and the extrinsic
 * (RosParamServer.cpp:29-30): general 4x4 inverse in double with the operation order of Eigen 3.3.7's SSE2 kernel (2x2 block
 * adjugates; restated).  Row-major in and out, needs no context or device.  The ONE inverse of the
 * product: ltm_create uses it for the extrinsic, ltm_poses_create for missing inverses, the C++ host for the pose files.
 * Returns LTM_OK, or LTM_E_INVALID for a null argument or a singular / non-finite matrix (Eigen would return inf / NaN entries). */
int ltm_inverse4x4(const double* m16, double* inv16);
int ltm_poses_free(ltm_ctx*, ltm_poses);

/* ------------------------------------------------- the hot path, one call per stage ---- */

/* Session.cpp:506-533 precleaningKeyframes: drop points with range<radius & |z|<0.5 */
int ltm_preclean(ltm_ctx*, ltm_scanset in, float radius, ltm_scanset* out);

/* utility.cpp:170-192 mergeScansWithinGlobalCoordUtil / Session.cpp:186-202: local -> global concat */
int ltm_merge_to_global(ltm_ctx*, ltm_scanset scans, ltm_poses poses, ltm_cloud* out);

/* utility.cpp:204-219 octreeDownsampling (PCL OctreePointCloudVoxelCentroid): voxel centroids in octree DFS order */
int ltm_voxel_centroid(ltm_ctx*, ltm_cloud in, float leaf, ltm_cloud* out);
/* the same for n independent clouds at once (e.g. the static and the dynamic map after a vote pass, Removerter.cpp:894-903; the eight
 * maps of Removerter.cpp:1445-1476): identical results, but the host reads all bounding boxes and all voxel counts in two round
 * trips for the whole batch instead of two per cloud */
int ltm_voxel_centroid_batch(ltm_ctx*, size_t n, const ltm_cloud* in, const float* leaf, ltm_cloud* out);
/* multi-GPU form of the above: only the voxels of shard `shard` of `n_shards`.  The Morton key space of the
 * octree is cut into n_shards contiguous ranges of about equal point count (a pure function of `in`), so the outputs of
 * shards 0..n_shards-1 concatenated in order ARE ltm_voxel_centroid(in); each rank sorts 1/n_shards of the points. */
int ltm_voxel_centroid_shard(ltm_ctx*, ltm_cloud in, float leaf, uint32_t shard, uint32_t n_shards, ltm_cloud* out);
/* Key-range exchange: the voxel grid of a cloud whose POINTS are spread over the ranks -- the merge of
 * rank-local per-keyframe scans (utility.cpp:170-192 followed by :204-219) -- without gathering the points on every rank.  Every rank:
 *   ltm_cloud_bbox            box of its own points            -> the ranks combine them (min / max): the box of the whole cloud
 *   ltm_voxel_key_histogram   4096-bin histogram of its points' octree keys under the WHOLE cloud's frame (top bits of the compressed
 *                             Morton code)                     -> summed over the ranks; cut into n contiguous bin ranges of equal weight
 *   ltm_voxel_key_split       its points of every range, each in input order -> all-to-all: rank r receives range r from everybody, in
 *                             rank order = keyframe order = the input order of the single-GPU merge restricted to the range
 *   ltm_voxel_centroid_box    the voxel grid of what it received, under the whole cloud's frame (the box is given, not derived)
 * and the outputs of ranks 0..n-1 concatenated ARE ltm_voxel_centroid of the merged cloud: a bin is a prefix of the key, so no voxel
 * straddles a cut, and every voxel sums its points in the order the single-GPU grid does.  hist has 4096 entries; cut_bins n_parts + 1,
 * cut_bins[0] = 0, cut_bins[n_parts] = 4096.  An empty cloud has the box (+inf, -inf) and an all-zero histogram. */
int ltm_cloud_bbox(ltm_ctx*, ltm_cloud in, float mn[3], float mx[3]);
int ltm_voxel_key_histogram(ltm_ctx*, ltm_cloud in, const float mn[3], const float mx[3], float leaf, uint32_t hist[4096]);
int ltm_voxel_key_split(ltm_ctx*, ltm_cloud in, const float mn[3], const float mx[3], float leaf, uint32_t n_parts, const uint32_t* cut_bins, ltm_cloud* parts);
int ltm_voxel_centroid_box(ltm_ctx*, ltm_cloud in, const float mn[3], const float mx[3], float leaf, ltm_cloud* out);
/* the same applied to every keyframe of a scan set (Session.cpp:362-380 updateScansScanwise) */
int ltm_voxel_centroid_scanset(ltm_ctx*, ltm_scanset in, float leaf, ltm_scanset* out);

/* pcl::VoxelGrid as the session loader applies it to every scan it reads (Session.cpp:284-289, leaf = downsample_voxel_size), for all
 * keyframes of a scan set at once: centroids (x, y, z, intensity) per occupied leaf in ascending leaf index; a keyframe whose grid
 * would exceed INT32_MAX cells is returned unchanged (PCL's "leaf size is too small" early-out -- the common case for a raw 0.05 m
 * scan).  The float sums of a leaf run in the order PCL's std::sort on the leaf index leaves its points in (the permutation
 * is computed on host threads, one keyframe per task, by a restatement of libstdc++'s introsort that makes the same element moves without
 * the branch mispredictions -- csrc/ltm_pclsort.h, checked against std::sort itself; bit-identical to
 * the reference's sources compiled against stand-in PCL headers, oracle/_ref -- PCL itself is not available, so "as PCL 1.10 is understood to do it").  LTM_VOXELGRID_ORDER=input sums in input
 * order entirely on the device: faster, but the last bit of a centroid of three or more points may differ.  This is what makes a device-resident cascade hand over the scans the reference would
 * re-load from scans_updated/ (README.md:115-118; Removerter.cpp:1658-1660). */
int ltm_voxel_grid_scanset(ltm_ctx*, ltm_scanset in, float leaf, ltm_scanset* out);
/* The same in two halves, for a caller that has other work for the device meanwhile (the lifelong cascade: the next run's query session does not depend on
 * the re-loaded central scans -- Session.cpp:284-289 of the NEXT process, Removerter.cpp:1653-1660).  _begin enqueues the key kernels, sends the keys to the
 * host on the copy stream and starts the host threads that reproduce std::sort's order; it returns without waiting for either, and whatever is submitted to
 * the context afterwards runs beside them.  _end waits for the order and finishes the grid.  `in` must stay alive and unchanged until _end, which consumes
 * the ticket whatever it returns.  ltm_voxel_grid_scanset is _begin + _end back to back. */
typedef struct ltm_vgs ltm_vgs;
int ltm_voxel_grid_scanset_begin(ltm_ctx*, ltm_scanset in, float leaf, ltm_vgs** ticket);
int ltm_voxel_grid_scanset_end(ltm_ctx*, ltm_vgs* ticket, ltm_scanset* out);

/* Visibility vote, keyframes [kf_begin,kf_end) of `scans`/`poses` against `map`:
 *   scan2RangeImg (Removerter.cpp:109-156) + transformGlobalMapToLocal (utility.cpp:64-72) +
 *   map2RangeImg (utility.cpp:92-142) + calcDescrepancyAndParseDynamicPointIdx (Removerter.cpp:381-413),
 *   i.e. the loop body of calcDescrepancyAndParseDynamicPointIdxForEachScan[ForND|ForPD] (:429-593).
 * mode 0: diff = scan - map (remove / revert / PD);  mode 1: diff = map - scan (ND).
 * labels_dev: device buffer of M bytes; label 1 is OR-ed in for every flagged map point (the std::set
 * union of :589-590).  The caller zeroes it; ranks combine theirs with a MAX all-reduce. */
int ltm_visibility_vote(ltm_ctx*, ltm_cloud map, ltm_scanset scans, ltm_poses poses, size_t kf_begin, size_t kf_end,
                        float res_alpha, float diff_thres, int mode, uint8_t* labels_dev);
/* Optional: scan2RangeImg (Removerter.cpp:109-156) of keyframes [kf_begin,kf_end) of `scans` for ALL the listed resolutions in one pass over the points,
 * kept for the votes that follow (selfRemovert projects every scan at res and 0.95 res for each entry of remove_resolution_list: six image shapes whose
 * spherical coordinates are the same).  ltm_visibility_vote computes what it does not find, one shape at a time; the images are identical either way. */
int ltm_scanset_prepare_range_images(ltm_ctx*, ltm_scanset scans, size_t kf_begin, size_t kf_end, const float* res_alphas, size_t n_alphas);
/* The same, plus the threshold the votes that follow will be called with (diff_thres of ltm_visibility_vote; < 0: none, which is the entry above).
 * The images are built in the CU's LDS and written once (k_scan_rimg_lds: no fill, no global atomics), and with a threshold the bound images of the
 * range-culled vote for it come out of the same pass instead of a pass of their own at the first vote.  A vote with another threshold rebuilds its bound
 * image as before.  Context switch LTM_SCAN_IMG_LDS (read by ltm_create, default 1): 0 takes the fill / global-atomic / read-back kernels (k_scan_rimg_multi for one
 * shape or several, k_image_max, k_scan_qbound), which shape sets the LDS plan cannot serve (ltm_debug_scan_bands) take in any case.  Images, maxima and bound images are the same bits either way. */
int ltm_scanset_prepare_vote_images(ltm_ctx*, ltm_scanset scans, size_t kf_begin, size_t kf_end, const float* res_alphas, size_t n_alphas, float diff_thres);
/* partitionCurrentMap tail (Removerter.cpp:816-824, :675-687, :933-946): index-ascending split */
int ltm_partition_by_labels(ltm_ctx*, ltm_cloud map, const uint8_t* labels_dev, ltm_cloud* kept, ltm_cloud* flagged);
/* vote over all keyframes + partition (single-GPU convenience).  host_labels (M bytes) may be NULL. */
int ltm_visibility_partition(ltm_ctx*, ltm_cloud map, ltm_scanset scans, ltm_poses poses, float res_alpha,
                             float diff_thres, int mode, ltm_cloud* kept, ltm_cloud* flagged, uint8_t* host_labels);

/* parseProjectedPoints / Session::parseScansViaProjection (utility.cpp:74-89, Session.cpp:348-360):
 * out has (kf_end-kf_begin) keyframes of local-frame points, row-major pixel order, ptidx==0 dropped. */
int ltm_reproject(ltm_ctx*, ltm_cloud map, ltm_poses poses, size_t kf_begin, size_t kf_end, float res_alpha, ltm_scanset* out);
/* Two maps at once: out_a / out_b are exactly what ltm_reproject(map_a) and ltm_reproject(map_b) return.  Meant for two voxel grids of clouds that share
 * nearly all their points (map_global_updated_ and its "strong" twin, Removerter.cpp:1483-1524): where both maps carry the frame of their grid and the frames
 * and leaves are equal, the points that are bit-identical in both (all four floats; -0.0 and +0.0 differ) are projected ONCE by the exact-image kernel, the image's
 * point indices are replaced through two increasing tables, and the few points each map has alone are added with their own indices (the image is
 * a minimum, and both maps list the shared points in the same order).  Two plain reprojections instead when a cloud is empty or has no frame, the frames
 * differ, the shared points are fewer than LTM_REPROJECT_TWIN_MIN_SHARED (default 0.75) of the larger map, or the context was created with
 * LTM_REPROJECT_TWIN=0 (A/B switch).  ltm_debug_reproject_twin_stats counts which way the calls went. */
int ltm_reproject_twin(ltm_ctx*, ltm_cloud map_a, ltm_cloud map_b, ltm_poses poses, size_t kf_begin, size_t kf_end, float res_alpha, ltm_scanset* out_a,
                       ltm_scanset* out_b);
/* *applicable = 1 when ltm_reproject_twin would look for shared points (switch on, both clouds hold points and the frame of their grid, frames and leaves equal),
 * 0 when it is two plain reprojections from the start.  Host side only, nothing is launched: a caller with two lanes keeps the two maps on two lanes then. */
int ltm_reproject_twin_applicable(ltm_ctx*, ltm_cloud map_a, ltm_cloud map_b, int* applicable);

/* extractLowDynPointsViaKnnDiff / extractHighDynPointsViaKnnDiff (Session.cpp:393-427, 487-504, 537-642):
 * exact k-NN of every scan point (moved to the global frame) in `target`; coexist iff mean of the k squared
 * distances < thr.  Outputs are in the local frame, input order kept.  Either output may be NULL.
 * Domain (also of ltm_knn_split_cloud): 1 <= k <= 16 and thr > 0 (a NaN thr included), else LTM_E_INVALID.  k is clamped to the target
 * size for the search and stays the divisor of the mean, as pcl::KdTreeFLANN::nearestKSearch + Session.cpp:590-599 give; an empty target
 * makes every query "diff" / "far".  A query whose global-frame point has a non-finite coordinate (NaN, +-inf, or a finite value
 * whose squared distance overflows) is "diff" / "far" and keeps its input position.  A target of more than 64 points whose bounding
 * box is not finite (a +-inf coordinate, or a NaN that reaches the box) is LTM_E_INVALID; a NaN the box does not show is undefined, as
 * in the reference.  Targets of up to 64 points are searched by brute force, no box is taken and none is checked: a target point with
 * a +-inf coordinate is a point at infinite distance (it only counts where k exceeds the finite points, and then makes the query
 * "diff" / "far"), a NaN target coordinate is undefined there too. */
int ltm_knn_partition(ltm_ctx*, ltm_cloud target, ltm_scanset scans, ltm_poses poses, size_t kf_begin, size_t kf_end,
                      int k, float thr, ltm_scanset* coexist, ltm_scanset* diff);
/* removeWeakNDMapPointsHavingStrongNDInNear (Session.cpp:452-484): split `query` by k-NN distance to `target` */
int ltm_knn_split_cloud(ltm_ctx*, ltm_cloud target, ltm_cloud query, int k, float thr, ltm_cloud* near, ltm_cloud* far);

/* ----------------------------------------------------------- search index ---- */
/* The reference's pcl::KdTreeFLANN<PointType> members (Session.cpp:18-23; setInputCloud at :404, :457, :489; nearestKSearch at :471, :592, :627)
 * as a device-resident index with exact queries.  What this library takes KdTreeFLANN to do:
 *  - distance: squared L2 in float, evaluated as FLANN's L2_Simple, ((dx*dx)+dy*dy)+dz*dz, without fused multiply-adds;
 *  - kNN: the k smallest distances in ascending order; EQUAL DISTANCES ARE ORDERED BY THE SMALLER TARGET INDEX (FLANN leaves this unspecified);
 *    k is clamped to the number of (finite) target points as nearestKSearch clamps it, the rest of the row is index -1, distance +inf;
 *    1 <= k <= 64, anything else is LTM_E_INVALID;
 *  - radius: every target point with d2 < r2, r2 = (float)((double)radius * radius) (PCL's static_cast<float>(radius * radius), FLANN's strict <),
 *    ordered as for kNN; max_nn > 0 keeps only the max_nn nearest;
 *  - indices: int32 positions in the target cloud as it was given (the target must have fewer than 2^31 points);
 *  - target points with a non-finite coordinate are never returned; a query with one gets an empty row (all -1 for kNN, length 0 for radius);
 *    an empty target is valid and gives empty rows.
 * The result is exact for any distribution and any magnitude of finite points (the index is a tree of boxes over the target in Morton order, see
 * ltm_k_search.hip): it is what a scan of all finite target points in the float arithmetic above gives, also where that arithmetic underflows (a
 * cloud inside 1e-23 m has all distances 0 and every row is the k smallest indices), gives denormals, or overflows (a distance of +inf is a
 * distance like any other for kNN, ordered by index behind the finite ones, and is outside every radius, radius = +inf included).
 * Everything is asynchronous on the context's stream except ltm_radius_search, which reads the total hit count back.  The index and the
 * results come from the context's pool; the index keeps its own copy of the target (the cloud may be freed or changed afterwards).  Handles
 * belong to the context that made them (another context, a lane included, gets LTM_E_INVALID); ltm_destroy releases whatever is still open. */
typedef struct ltm_search ltm_search;
typedef struct ltm_search_result ltm_search_result;
/* kdtree->setInputCloud(target) (Session.cpp:404, :457, :489) */
int ltm_search_build(ltm_ctx*, ltm_cloud target, ltm_search** out);
int ltm_search_free(ltm_ctx*, ltm_search*);
/* number of target points the index was built over, and how many of them are finite (searchable) */
int ltm_search_info(ltm_ctx*, ltm_search*, size_t* n_target, size_t* n_finite);
/* kdtree->nearestKSearch(query[i], k, idx, d2) for every point of `query` (Session.cpp:471, :592, :627): n_query x k rows, row-major, in the
 * caller's device buffers idx_dev (int32) and d2_dev (float) */
int ltm_knn_search(ltm_ctx*, ltm_search*, ltm_cloud query, int k, int32_t* idx_dev, float* d2_dev);
/* kdtree->radiusSearch(query[i], radius, idx, d2, max_nn) for every point of `query` (no call site in the reference; LT-SLAM's loop search):
 * CSR result, row i = [offsets[i], offsets[i+1]) of idx / d2 */
int ltm_radius_search(ltm_ctx*, ltm_search*, ltm_cloud query, float radius, int max_nn, ltm_search_result** out);
/* the result's device arrays (offsets: n_query + 1 entries), borrowed until ltm_search_result_free */
int ltm_search_result_info(ltm_ctx*, ltm_search_result*, size_t* n_query, size_t* total,
                           const uint64_t** offsets_dev, const int32_t** idx_dev, const float** d2_dev);
int ltm_search_result_free(ltm_ctx*, ltm_search_result*);

/* ---------------------------------------------------------------- normals ---- */
/* pcl::NormalEstimation (setKSearch(k), setViewPoint(vx, vy, vz), compute) over the target of a search index: one (nx, ny, nz, curvature) per target
 * point.  The reference calls neither NormalEstimation nor a method that needs normals; PCL is not available to compare against.  This is the arithmetic
 * this library takes PCL 1.10's NormalEstimation (computePointNormal, flipNormalTowardsViewpoint) to do, as understood; tools/normals_numpy.py restates it
 * in numpy and the tests compare against that.
 *  - Neighbourhood of a finite target point: its min(k, n_finite) nearest target points, ITSELF INCLUDED at distance 0, in ltm_knn_search order
 *    (L2_Simple in float, ties to the smaller target index).  3 <= k <= 64, anything else is LTM_E_INVALID.
 *  - Fewer than 3 neighbours (a target with fewer than 3 finite points): normal and curvature are NaN (computePointNormal returns false there).
 *  - Covariance, in double: with d_i = (double)q_i - (double)p the neighbours as differences from the point p itself, summed in the neighbourhood's
 *    ascending (d2, index) order, m = sum d_i / n, C = sum d_i d_i^T / n - m m^T.
 *  - Normal: the eigenvector of the smallest eigenvalue of C (the lower axis among equal eigenvalues) by cyclic Jacobi rotations in double, normalised to
 *    unit length; CANONICAL SIGN: the component of largest magnitude is made positive (the lower axis among equals); then flipNormalTowardsViewpoint:
 *    negated if ((vx - px) nx + (vy - py) ny) + (vz - pz) nz < 0, evaluated in double; then rounded to float.
 *  - Curvature: lambda_min / (lambda_0 + lambda_1 + lambda_2) in double, rounded to float; negative rounding residue of lambda_min is clamped to 0, and a
 *    trace that is not positive gives 0.
 *  - Degenerate neighbourhoods: when the two smallest eigenvalues coincide (collinear or coincident neighbours) the direction is not unique; the normal is
 *    then only promised to be finite, of unit length, and reproducible.
 *  - Target points with a non-finite coordinate are not in the index: they are nobody's neighbour and ltm_search_normals_download writes NaN to all four
 *    of their fields.
 *  DEPARTURES from PCL: PCL accumulates the nine raw moments in float about the origin and takes the eigenvector with the closed-form eigen33; here the
 *  moments are doubles about the point itself and the eigenvector comes from Jacobi rotations, so map coordinates kilometres from zero lose nothing.  PCL
 *  leaves the sign before the viewpoint flip to eigen33; here it is canonical.  PCL's curvature divides by the trace of the float covariance.
 * ltm_search_estimate_normals estimates the normals of ALL listed indices with one k in one kernel launch (viewpoints3_or_null: n_idx x 3 floats, NULL =
 * (0, 0, 0) for every index) and reads nothing back.  The normals live with the index: one float4 per finite target point in the index's own order, in ONE
 * pool block per call that the handles of the call share; it goes back to the pool when the last of them is freed or estimated again (a second estimate
 * replaces the first).  Handles of ltm_search_build and of ltm_search_build_scanset may be mixed; the same handle twice in one call, a handle of another
 * context, a non-finite viewpoint: LTM_E_INVALID, and every index stays as it was. */
int ltm_search_estimate_normals(ltm_ctx*, size_t n_idx, ltm_search* const* idx, int k,
                                const float* viewpoints3_or_null /* n_idx x 3, NULL = (0,0,0) for all */);
/* k the normals were estimated with (0 = none) and the device array (n_finite float4 in the index's order; NULL without normals or finite points), borrowed
 * until the index is freed or estimated again */
int ltm_search_normals_info(ltm_ctx*, ltm_search*, int* k /* 0 = none */, const void** normals_dev /* borrowed */);
/* (nx, ny, nz, curvature) of every target point in the target's ORIGINAL order; an index without normals is LTM_E_INVALID */
int ltm_search_normals_download(ltm_ctx*, ltm_search*, float* nxyzc_host /* n_target x 4, the target's ORIGINAL order */);

/* ----------------------------------------------------------- scan context ---- */
/* Scan Context place recognition, the step of the reference that decides which keyframes of two sessions see the same place before LT-removert diffs
 * them: SCManager (ltslam/src/Scancontext.cpp:69-324, ltslam/include/ltslam/Scancontext.h:58-121) as LTslam::detectInterSessionSCloops drives it
 * (ltslam/src/LTslam.cpp:304-333).  A descriptor set holds N descriptors (num_ring x num_sector doubles, row-major [ring][sector]) with their ring keys
 * (float), sector keys (double) and column norms on the device.  What this library takes the reference to do:
 *  - bin of a point (:166-179): r = (float)sqrt(x*x + y*y), the sum in float without fused multiply-add (a float sqrtf and a double sqrt rounded to float
 *    agree here); theta = xy2theta (:23-36) with the quotient in float, atan in DOUBLE, the four quadrant forms in double, the result rounded to float.
 *    (An unqualified atan of a float could also resolve to the float overload, depending on what the reference's includes pull in; the two readings differ
 *    only for points within rounding of a sector edge.  The device's double atan may differ from glibc's in the last bits, which moves the float theta of
 *    about one point in 10^8.)  ring = clamp(int(ceil(r / max_radius * num_ring)), 1, num_ring) in double, sector likewise from theta / 360.0.  Points with
 *    r > max_radius are skipped.
 *  - quirks, mirrored as x86 gives them: x == 0 && y == 0 has a NaN quotient whose int conversion is INT_MIN, so the point lands in sector 1, ring 1;
 *    x == -0.0f takes the x >= 0 branches.  A point with a non-finite coordinate is SKIPPED (undefined behaviour in the reference: its bin index is garbage).
 *  - height (:168, :182-190): value = (float)((double)z + lidar_height), stored as a double; a bin holds the maximum over its points starting from -1000, and
 *    a bin still at -1000 at the end becomes 0 -- bins whose every point had a value <= -1000 included.  Negative heights are legal and win against -1000.
 *    (-0.0 and +0.0 compare equal in the reference and the first in point order stays; here +0.0 stays.)
 *  - keys (:198-246): ring key = row mean in double, stored as float (eig2stdvec); sector key = column mean in double.  Sums run in index order; Eigen's
 *    order is not specified, so the last bits of a mean may differ.
 *  - distDirectSC (:69-90): all in double; a column pair is skipped when either norm is 0; if no column counts the distance is NaN, as the reference gives.
 *  - distanceBtnScanContext (:116-148): the FIRST minimal sector-key shift wins (strict <, ascending shift); search radius = round(0.5 * search_ratio *
 *    num_sector) around it (search_ratio >= 1: every shift); the shift set is visited in ascending order and the first minimum wins; if every distance is NaN
 *    the result is (10000000, 0).
 *  - detect (:263-324): candidates are the num_candidates nearest ring keys under nanoflann's L2_Adaptor in float -- groups of four,
 *    result += d0*d0 + d1*d1 + d2*d2 + d3*d3, then the tail -- found by brute force; TIES GO TO THE SMALLER INDEX (nanoflann leaves this unspecified; a NaN
 *    key distance sorts last).  num_candidates is clamped to the database size (the reference reads uninitialised indices there); 0 = every database entry.
 *    Candidates are visited in ascending (key distance, index) order and the first minimal distance wins.  loop_id = nn_idx if min_dist < dist_thres, else -1.
 *    yaw_diff_rad = deg2rad(nn_align * (360.0 / num_sector)) as :17-20 and :319 compute it: the degrees rounded to float (deg2rad's parameter), times M_PI,
 *    divided by 180.0 in double, rounded to float.  An empty database gives loop_id -1, nn_idx 0, min_dist 10000000, nn_align 0 for every query.
 * Domain: 1 <= num_ring <= 64, 1 <= num_sector <= 256, num_candidates <= 64 unless it reaches the database size, and in one ltm_sc_detect
 * n_query x n_database < 2^31 (the ring-key distances of all of them are held at once, 4 bytes each) (LTM_E_UNSUPPORTED beyond; LTM_E_INVALID for
 * values that make no sense: counts < 1, max_radius <= 0, negative search_ratio, non-finite values).  A NULL parameter pointer means the defaults.  In
 * ltm_sc_distance / ltm_sc_detect the parameters' num_ring / num_sector must be those of the handles, and two handles with different counts are
 * LTM_E_INVALID.  Handles belong to the context that made them (another context, a lane included, gets LTM_E_INVALID); memory comes from the context's pool;
 * ltm_destroy releases whatever is still open.  ltm_sc_from_scanset is asynchronous on the context's stream; the calls that read or write host arrays return
 * when those are done. */
typedef struct ltm_sc ltm_sc;
typedef struct {
    double lidar_height;    /* 2.0   LIDAR_HEIGHT, Scancontext.h:84 */
    int    num_ring;        /* 20    PC_NUM_RING, 1..64 */
    int    num_sector;      /* 60    PC_NUM_SECTOR, 1..256 */
    double max_radius;      /* 80.0  PC_MAX_RADIUS */
    int    num_candidates;  /* 3     NUM_CANDIDATES_FROM_TREE; 0 = every database entry (exhaustive) */
    double search_ratio;    /* 0.1   SEARCH_RATIO; >= 1.0 = every shift */
    double dist_thres;      /* 0.3   SC_DIST_THRES */
} ltm_sc_params;
void ltm_sc_default_params(ltm_sc_params*);      /* host only, needs no device */
/* makeAndSaveScancontextAndKeys (:249-260) for every keyframe of [kf_begin, kf_end) of a scan set */
int  ltm_sc_from_scanset(ltm_ctx*, ltm_scanset, size_t kf_begin, size_t kf_end, const ltm_sc_params*, ltm_sc** out);
/* saveScancontextAndKeys (:236-246) for n descriptors read elsewhere (the SCD files of LTslam.cpp): desc_host is n x num_ring x num_sector, row-major */
int  ltm_sc_from_descriptors(ltm_ctx*, const double* desc_host, size_t n, const ltm_sc_params*, ltm_sc** out);
int  ltm_sc_info(ltm_ctx*, ltm_sc*, size_t* n, int* num_ring, int* num_sector);
/* descriptors (n x ring x sector), ring keys (n x ring), sector keys (n x sector) into host arrays; any may be NULL */
int  ltm_sc_download(ltm_ctx*, ltm_sc*, double* desc, float* ring_keys, double* sector_keys);
/* distanceBtnScanContext(a[i], b[j]) (:116-148) for n_pairs pairs (i, j) = pairs_host[2k], pairs_host[2k + 1]; reads search_ratio; outputs may be NULL */
int  ltm_sc_distance(ltm_ctx*, ltm_sc* a, ltm_sc* b, const int32_t* pairs_host, size_t n_pairs, const ltm_sc_params*, double* dist_host, int32_t* shift_host);
/* detectLoopClosureIDBetweenSession (:263-324) for every descriptor of `queries` against `database`; reads num_candidates, search_ratio, dist_thres; host
 * outputs of n_query entries each, any may be NULL */
int  ltm_sc_detect(ltm_ctx*, ltm_sc* database, ltm_sc* queries, const ltm_sc_params*, int32_t* loop_id, int32_t* nn_idx, double* min_dist, int32_t* nn_align,
                   float* yaw_diff_rad);
int  ltm_sc_free(ltm_ctx*, ltm_sc*);

/* -------------------------------------------------------------------- icp ---- */
/* Batched point-to-point ICP of source clouds against search indices: the step of the reference that verifies the loop pairs Scan Context proposes.
 * LTslam::addSCloops / addRSloops (ltslam/src/LTslam.cpp:370-416, :508-560) run pcl::IterativeClosestPoint for up to kNumSCLoopsUpperBound = 1000 pairs
 * (doICPVirtualRelative / doICPGlobalRelative, :187-301) and accept a pair only if hasConverged() and getFitnessScore() <= loopFitnessScoreThreshold.
 * Here all pairs of one call advance together, two kernel launches per iteration for the whole batch.  PCL is not available to compare against; this is
 * the arithmetic this library takes PCL 1.10's IterativeClosestPoint (TransformationEstimationSVD, DefaultConvergenceCriteria) to do.  tools/icp_numpy.py
 * restates it in numpy and the tests compare against that.
 *  Iteration, per pair, with T the accumulated source->target transform (T = init at the start):
 *   1. every source point with three finite coordinates is transformed by T in double, x' = ((T00 x + T01 y) + T02 z) + T03 and likewise y', z', without
 *      fused multiply-adds, and rounded to float: the query.  (A query that overflows float is skipped like a non-finite point.)
 *   2. its nearest target point is found exactly as ltm_knn_search with k = 1 finds it: FLANN's L2_Simple in float, ties to the smaller target index;
 *   3. the pair (query, target point) is kept iff (double)d2 <= max_corr_dist * max_corr_dist;
 *   4. fewer than 3 kept pairs: the pair stops, converged = 0, state = 0; T and `iterations` stay as they are, n_corr / last_mse / the trace row record
 *      what was found;
 *   5. otherwise the rigid transform from the queries p onto their target points q (both as doubles) by SVD, Umeyama without scale:
 *      H = mean((p - pm)(q - qm)^T), H = U S V^T, R = V diag(1, 1, det(V U^T)) U^T, t = qm - R pm, all in double;
 *   6. T <- T_iter T with T_iter = [R t]; iterations += 1; then the stop tests.
 *  DEPARTURES from PCL: PCL keeps Matrix4f transforms and re-transforms the already transformed cloud in float every iteration, so its rounding errors
 *  accumulate over the iterations; this library keeps T in double and always transforms the ORIGINAL source.  Sums run in a fixed order (source points in
 *  the code order of the target's frame, 256 per partial sum, partial sums in order) and about the corner of the target's bounding box, so a run is
 *  bit-reproducible, a pair's result does not depend on the rest of the batch, and map coordinates kilometres from zero lose nothing.  Eigen's JacobiSVD
 *  is replaced by a one-sided Jacobi SVD; the two agree to rounding when H has rank >= 2.
 *  Stop tests after step 6, in PCL's order (DefaultConvergenceCriteria with max_iterations_similar_transforms_ = 0), mse = mean of the kept float d2 summed
 *  in double, prev_mse = DBL_MAX at the start and the previous iteration's mse afterwards:
 *   1. iterations >= max_iterations                                                                   -> state 1
 *   2. 0.5 * (trace(R) - 1) >= 1 - transformation_epsilon and |t|^2 <= transformation_epsilon         -> state 2
 *   3. |mse - prev_mse| < 1e-12                                                                       -> state 3
 *   4. |mse - prev_mse| / prev_mse < euclidean_fitness_epsilon                                        -> state 4
 *  each with converged = 1.  (PCL evaluates the mse only when tests 1 and 2 fail; here last_mse and the trace always hold it.)
 *  Fitness (getFitnessScore() with its default, unlimited max_range): after the loop, the mean over the finite source points, transformed by the final T
 *  as in step 1, of the d2 to their nearest target point; DBL_MAX if no point counts.
 *  Edge cases: an empty source, a target without a finite point, or max_iterations < 1: T = init, iterations = 0, converged = 0, state = 0, n_corr = 0,
 *  fitness = last_mse = DBL_MAX.  Non-finite source points are skipped everywhere.  last_mse is DBL_MAX when the last iteration kept no pair.  When H has
 *  rank < 2 (all kept target points on one line, or one point) the rotation is not unique: the result is then only promised to be finite, orthonormal with
 *  det +1, and reproducible.
 *  trace (n_pairs x max_iterations x 2 doubles, may be NULL): row i of a pair = (n_corr, mse) of its iteration i, counted from 0, the iteration that stopped
 *  in step 4 included (mse NaN if it kept nothing); rows that never ran are NaN.
 *  targets[i] is an index from ltm_search_build or ltm_search_build_scanset (the same index may serve many pairs), sources[i] a cloud; both belong to this context (a handle of
 *  another context is LTM_E_INVALID).  init16_or_null: n_pairs row-major 4x4 doubles whose last row is taken to be 0 0 0 1, NULL = identity.  A NULL
 *  parameter pointer means the defaults.  Each source (< 2^31 points, < 2^31 in all) is copied in sorted order for the call; all device memory comes from
 *  the context's pool and is back when the call returns, on every error path too.  The call returns when the host arrays are written.
 *  The submaps themselves come from the section "loop submaps" below.  Point-to-plane and generalized ICP are the next two sections.  Out of scope: Euler / gtsam::Pose3 conversions. */
typedef struct {
    double max_corr_dist;             /* 150.0  setMaxCorrespondenceDistance, LTslam.cpp:207 */
    int    max_iterations;            /* 100    :208 */
    double transformation_epsilon;    /* 1e-6   :209 */
    double euclidean_fitness_epsilon; /* 1e-6   :210 */
} ltm_icp_params;
typedef struct {
    double   T[16];          /* final source->target transform, row-major */
    double   fitness;        /* getFitnessScore(): mean squared 1-NN distance of the transformed source; DBL_MAX if no point counts */
    double   last_mse;       /* mean squared correspondence distance of the last iteration */
    int32_t  converged;      /* hasConverged() */
    int32_t  iterations;
    int32_t  state;          /* why it stopped: 0 too few correspondences / nothing to do, 1 iterations, 2 transform, 3 absolute MSE, 4 relative MSE;
                                point-to-plane and generalized only: 5 degenerate system */
    uint32_t n_corr;         /* correspondences of the last iteration */
} ltm_icp_result;
void ltm_icp_default_params(ltm_icp_params*);     /* host only, needs no device */
int  ltm_icp_align(ltm_ctx*, size_t n_pairs, ltm_search* const* targets, const ltm_cloud* sources,
                   const double* init16_or_null /* n_pairs x 16, NULL = identity */, const ltm_icp_params*,
                   ltm_icp_result* results_host, double* trace_host_or_null /* n_pairs x max_iterations x 2: (n_corr, mse) per iteration, rest NaN */);
/* the same routine with sources[i] = keyframe source_kf[i] of the scan set `sources` (a submap of ltm_submaps_assemble) read in place, no cloud handle and
 * no copy per pair; a keyframe outside the set is LTM_E_INVALID.  Results are those of ltm_icp_align on ltm_scanset_keyframe of the same keyframes, bit for bit. */
int  ltm_icp_align_scanset(ltm_ctx*, size_t n_pairs, ltm_search* const* targets, ltm_scanset sources, const uint32_t* source_kf /* n_pairs */,
                           const double* init16_or_null, const ltm_icp_params*, ltm_icp_result* results_host, double* trace_host_or_null);

/* ------------------------------------------------- icp, point-to-plane ---- */
/* The same batch with the point-to-plane error: pcl::IterativeClosestPointWithNormals (TransformationEstimationPointToPlaneLLS), as understood; the
 * reference does not call it.  Arguments, ltm_icp_params, ltm_icp_result and the trace are those of ltm_icp_align / ltm_icp_align_scanset; every target
 * must carry normals (ltm_search_estimate_normals), else LTM_E_INVALID.  Two kernel launches per iteration for the whole batch.  tools/icp_plane_numpy.py
 * restates the arithmetic below and the tests compare against it.
 *  Steps 1-3 of an iteration (transform of the ORIGINAL source in double -> float query, exact 1-NN, distance limit), the stop tests, mse, fitness, the
 *  trace and the edge cases are those of the section "icp", unchanged.  Then:
 *   4. a kept correspondence whose target normal is not finite is DROPPED: it counts neither in n_corr nor in the mse;
 *   5. fewer than 3 correspondences: the pair stops, converged = 0, state = 0, as in "icp";
 *   6. linear system: with the query p, its target point q and the target point's normal n as doubles, p and q taken about the pair's origin o (the corner
 *      of the target's bounding box), every correspondence gives the row a = [p x n, n] and the right side b = n . (q - p).  A^T A (21 entries), A^T b (6),
 *      the count and the sum of d2 are accumulated in double in the fixed order of "icp" (256 source points per partial sum, partial sums in order);
 *   7. solve (A^T A) x = A^T b by Cholesky in double WITHOUT pivoting.  A diagonal entry (A^T A)_jj that is not positive or a pivot
 *      d_j <= 1e-12 (A^T A)_jj stops the pair: converged = 0, state = 5 ("degenerate system", these entry points only), T and `iterations` stay as they
 *      are, n_corr / last_mse / the trace row record what was found.  The threshold is relative to the entry's own scale, so the mixed units of rotation
 *      and translation do not matter; a single exact plane gives exact zeros on three diagonal entries;
 *   8. x = (alpha, beta, gamma, t'): R = Rz(gamma) Ry(beta) Rx(alpha), entry by entry as PCL's constructTransformationMatrix has it,
 *        R00 = cg cb    R01 = -sg ca + cg sb sa    R02 =  sg sa + cg sb ca
 *        R10 = sg cb    R11 =  cg ca + sg sb sa    R12 = -cg sa + sg sb ca
 *        R20 = -sb      R21 =  cb sa               R22 =  cb ca              (sa = sin alpha, ca = cos alpha, ...)
 *      t = t' + o - R o;  T <- [R t] T;  iterations += 1;  the stop tests of "icp" with this R and t.
 *  DEPARTURES from PCL, beyond those of "icp": the system is formed about o and not about the coordinate origin.  The linearised problem is the same
 *  about any origin; the nonlinear R applied about o differs from PCL's in the second order of the angles only (t = t' + o - R o instead of t').  PCL
 *  solves with Eigen's inverse(); here Cholesky, and a system that does not determine all six unknowns is reported (state 5) instead of solved. */
int  ltm_icp_align_plane(ltm_ctx*, size_t n_pairs, ltm_search* const* targets, const ltm_cloud* sources,
                         const double* init16_or_null, const ltm_icp_params*, ltm_icp_result* results_host, double* trace_host_or_null);
int  ltm_icp_align_plane_scanset(ltm_ctx*, size_t n_pairs, ltm_search* const* targets, ltm_scanset sources, const uint32_t* source_kf /* n_pairs */,
                                 const double* init16_or_null, const ltm_icp_params*, ltm_icp_result* results_host, double* trace_host_or_null);

/* ------------------------------------------------------ icp, generalized ---- */
/* The same batch with the plane-to-plane error of generalized ICP (Segal, Haehnel, Thrun; pcl::GeneralizedIterativeClosestPoint), as understood; the
 * reference does not call it.  ltm_icp_params, ltm_icp_result and the trace are those of ltm_icp_align.  BOTH sides of a pair are search indices
 * (ltm_search_build or ltm_search_build_scanset; the same handle may serve many pairs and may be the target of one pair and the source of another) and both
 * must carry normals (ltm_search_estimate_normals, any k; PCL's k_correspondences_ is 20), else LTM_E_INVALID.  gicp_epsilon must be finite and in
 * (0, 1] (PCL's default 0.001), else LTM_E_INVALID; so are a NULL handle, a handle of another context and NaN parameters.  Two kernel launches per
 * iteration for the whole batch.  The sources are read in place from their indices: no per-call sort, no copy.  All device memory comes from the
 * context's pool and is back when the call returns, on every error path too.  tools/icp_gicp_numpy.py restates the arithmetic below and the tests
 * compare against it.
 *  The covariances: GICP gives every point the covariance of its neighbourhood with the singular values replaced by (1, 1, epsilon), which is
 *  C = I - (1 - epsilon) n n^T with n the unit eigenvector of the smallest eigenvalue -- the normal the index already holds (its sign does not matter).
 *  No covariance is computed or stored: with w = 1 - epsilon, C_B + R C_A R^T = 2I - w (n_b n_b^T + m m^T), m = R n_a.
 *  The source's points are the finite points of its index (non-finite points are not in an index and so are skipped everywhere, as in "icp").
 *  Steps 1-3 of an iteration (transform of the ORIGINAL source point by T in double -> float query, exact 1-NN with ties to the smaller target index,
 *  distance limit), the stop tests, mse, fitness, the trace and the edge cases are those of the section "icp", unchanged.  Then, all in double and
 *  without fused multiply-adds:
 *   4. a kept correspondence whose target normal n_b or source normal n_a is not finite is DROPPED: it counts neither in n_corr nor in the mse;
 *   5. fewer than 3 correspondences: the pair stops, converged = 0, state = 0, as in "icp";
 *   6. m = R_T n_a, R_T the upper-left 3 x 3 of the current T (taken to be a rotation; an init that is none is undefined in result, not a fault):
 *        m_r = (T_r0 a_x + T_r1 a_y) + T_r2 a_z;
 *      S = 2I - w (n_b n_b^T + m m^T), symmetric:  s00 = 2 - w (b_x b_x + m_x m_x), s01 = -w (b_x b_y + m_x m_y), ... s22 = 2 - w (b_z b_z + m_z m_z);
 *      M = adj(S) / det(S), entry by entry:
 *        c00 = s11 s22 - s12 s12    c01 = s02 s12 - s01 s22    c02 = s01 s12 - s02 s11
 *        c11 = s00 s22 - s02 s02    c12 = s01 s02 - s00 s12    c22 = s00 s11 - s01 s01
 *        det = (s00 c00 + s01 c01) + s02 c02,  M_ij = c_ij * (1 / det)   (M is symmetric and, for unit normals, positive definite: eigenvalues in
 *        [1/2, 1/(2 epsilon)]);
 *   7. with the query p and its target point q taken about the pair's origin o (the corner of the target's bounding box), d = q - p and
 *      A = [-[p]x, I] (3 x 6: A x = omega x p + t' for x = (omega, t')), the pair minimises sum (d - A x)^T M (d - A x) over its correspondences:
 *      the record is the count, the 21 upper entries of sum A^T M A, the 6 of sum A^T M d and sum d2 (the float d2 of the search) -- the layout of
 *      the point-to-plane record.  With G = M (-[p]x) and g = M d:  A^T M A = [[p x G_0, p x G_1, p x G_2 | G^T], [G | M]] (G_k the columns of G),
 *      A^T M d = [p x g, g].  SUMMATION ORDER: the source index's own order (its finite points in the code order of the source's OWN frame, the order
 *      of its tree) read in place, 256 per partial sum (the 64 points of a wavefront by a butterfly, the four wavefronts in order), partial sums in
 *      order.  It is a pure function of the pair's two handles: a pair's result does not depend on the rest of the batch, there are no floating-point
 *      atomics, and a run is bit-reproducible;
 *   8. solve and update exactly as point-to-plane steps 7-8: Cholesky without pivoting with the relative pivot test (state = 5 when it fails -- with M
 *      positive definite that needs degenerate geometry, for instance all correspondences on one line; a single exact plane does NOT give state 5
 *      here, epsilon constrains the in-plane unknowns weakly), x = (alpha, beta, gamma, t'), R = Rz Ry Rx, t = t' + o - R o, T <- [R t] T,
 *      iterations += 1, the stop tests of "icp".
 *  DEPARTURES from PCL: PCL minimises the same sum with BFGS over the correspondences of an outer iteration, recomputing M only per outer iteration,
 *  and keeps float transforms; here it is ONE Gauss-Newton step per correspondence search, about o, with T in double.  PCL computes its own
 *  covariances from k_correspondences_ neighbours by SVD; here they are those the index's normals imply (the same matrix whenever the smallest
 *  eigenvalue is simple).  PCL's rotation-epsilon test differs from its ICP's; here the stop tests are those of "icp". */
int  ltm_icp_align_gicp(ltm_ctx*, size_t n_pairs, ltm_search* const* targets, ltm_search* const* sources,
                        const double* init16_or_null, const ltm_icp_params*, double gicp_epsilon,
                        ltm_icp_result* results_host, double* trace_host_or_null);

/* ----------------------------------------------------------- loop submaps ---- */
/* The step between a loop proposal and its ICP verification: the two clouds of every ICP run of LTslam::doICPVirtualRelative / doICPGlobalRelative
 * (ltslam/src/LTslam.cpp:187-301) are built by Session::loopFindNearKeyframesLocalCoord / CentralCoord (ltslam/src/Session.cpp:91-142) -- the keyframes
 * within +-searchNum of a key, each moved by the float Eigen::Affine3f that pcl::getTransformation makes of a 6-D pose (ltslam/src/utility.cpp:80-103),
 * concatenated and put through pcl::VoxelGrid at 0.3 m (Session.cpp:18-19) -- and a kd-tree is built over every target.  Here all windows of a batch are
 * assembled by ONE gather launch and gridded together, and all their search indices are built together.  What this library takes the reference to do:
 *  - pose -> affine (ltm_pose6d_to_affine3f; host only, needs no device): pcl::getTransformation(x, y, z, roll, pitch, yaw) in float as PCL 1.10 writes it
 *    (common/impl/eigen.hpp; PCL is not available here, so "as understood"): A = cosf(yaw), B = sinf(yaw), C = cosf(pitch), D = sinf(pitch), E = cosf(roll),
 *    F = sinf(roll), DE = D*E, DF = D*F; row 0 = (A*C, A*DF - B*E, B*F + A*DE, x), row 1 = (B*C, A*E + B*DF, B*DE - A*F, y), row 2 = (-D, C*F, C*E, z); every
 *    product and sum a separate float rounding.  xyzrpy: n x 6 floats (x y z roll pitch yaw), affine12: n x 12 floats, rows 0..2 row-major.
 *  - window w of ltm_submaps_assemble holds the points of keyframes keys[w] - search_num ... keys[w] + search_num in ascending order; a keyframe index
 *    outside [0, n_kf) is skipped (Session.cpp:101), so any int32 key is legal; a window with no point is an empty keyframe of `out` (:106).
 *  - every point is moved by its keyframe's affine as utility.cpp:97-99 does: x' = ((t00*x + t01*y) + t02*z) + t03 in float, left to right, without fused
 *    multiply-adds, likewise y', z'; the intensity is copied.  affine12 = NULL means the identity for every keyframe (the LocalCoord form, whose pose is the
 *    origin): the arithmetic is still performed, so -0.0 becomes +0.0 and an infinite coordinate makes NaNs, as the reference's multiply by identity does.
 *  - each window is then gridded by pcl::VoxelGrid at `leaf` with the machinery of ltm_voxel_grid_scanset, unchanged: the same frames, the same "leaf size
 *    is too small" pass-through, the same treatment of non-finite points.  order = 1 sums a voxel's points in the order PCL's std::sort leaves them in
 *    (through the host threads of that path), order = 0 in input order, entirely on the device (the last bit of a centroid of three or more points may
 *    differ).  LTM_VOXELGRID_ORDER is not read here.
 * DEPARTURES: leaf == 0 means no grid -- `out` is the transformed concatenation (the reference always grids).  The reference transforms on 8 OpenMP threads
 * and grids each window alone; neither changes a result.
 * Domain: search_num < 0, a negative or non-finite leaf, an order other than 0 or 1 are LTM_E_INVALID; a batch whose windows hold 2^32 - 1 points or more
 * before the grid (the grid's 32-bit point indices) is LTM_E_UNSUPPORTED -- split the batch.  All scratch memory is back in the pool when the call returns,
 * on every error path too. */
int ltm_pose6d_to_affine3f(const float* xyzrpy /* n x 6: x y z roll pitch yaw */, size_t n, float* affine12 /* n x 12, rows 0..2 row-major */);
int ltm_submaps_assemble(ltm_ctx*, ltm_scanset scans, const float* affine12_host_or_null /* n_kf x 12; NULL = identity for every keyframe */,
                         const int32_t* keys_host, size_t n_windows, int search_num, float leaf, int order, ltm_scanset* out);
/* kdtree->setInputCloud for every keyframe of [kf_begin, kf_end) of a scan set at once (the submaps above): out receives kf_end - kf_begin handles, each
 * interchangeable with ltm_search_build of that keyframe as a cloud -- the same frame (the keyframe's own finite bounding box, 2097151 / extent), the same
 * finite count, leaf size and box tree -- so every query through it (ltm_knn_search, ltm_radius_search, ltm_icp_align) returns the bytes the single build
 * returns.  (The promise is on query results, not on the index arrays: the batch is ordered by ONE segmented radix sort, which need not be stable, so points
 * with equal codes may sit in another order; the search is exact and ties are ordered by target index.)  The whole batch is a fixed number of launches --
 * segmented bounding boxes with finite counts, keys, sort, gather, all box trees -- and ONE read-back by the host (the boxes), where n single builds pay one
 * each.  Every handle is freed on its own with ltm_search_free; the pool blocks the batch shares return when its last handle is freed (ltm_destroy
 * releases what is left).  Empty keyframes and keyframes without a finite point give valid empty indices; a range outside the set is LTM_E_INVALID, a batch
 * of 2^31 points or more LTM_E_UNSUPPORTED.  On an error no handle is returned and nothing stays allocated. */
int ltm_search_build_scanset(ltm_ctx*, ltm_scanset, size_t kf_begin, size_t kf_end, ltm_search** out /* kf_end - kf_begin handles */);

/* ---------------------------------------------------------------- clusters ---- */
/* Euclidean cluster extraction over the target of a search index: pcl::EuclideanClusterExtraction (setClusterTolerance, setMinClusterSize,
 * setMaxClusterSize, extract), the step that turns a map of changed points (nd_map, pd_map, scans_pd...) into objects, and the usual pre-filter before ICP,
 * normals or one Scan Context per object.  The reference does not call it and PCL is not available to compare against; this is what this library takes PCL
 * 1.10's extractEuclideanClusters / EuclideanClusterExtraction::extract to do, as understood.  tools/cluster_numpy.py restates it with scipy and the tests
 * compare against that, for equality.
 *  Graph: the vertices are the finite target points of the index; i and j are adjacent iff d2(i, j) < r2, with d2 the index's own distance (FLANN's
 *   L2_Simple in float, ((dx*dx)+dy*dy)+dz*dz, no fused multiply-add) and r2 = (float)((double)tolerance * tolerance), strict <: exactly the relation of
 *   ltm_radius_search.  The float expression is symmetric in its two points, so the relation is.  A cluster is a connected component; coincident points are
 *   adjacent (0 < r2).  The relation holds as stated at every finite tolerance > 0, down to r2 = 2^-149 and up to r2 = +inf: the shortcut that unites a
 *   whole leaf of the index without testing its pairs (ltm_box_bound.h, box_is_clique) is taken only where the exact diagonal of the leaf's box, with
 *   the float expression's relative error and the half denormal each of its three squares can gain when it underflows, stays below r2.
 *  Filter: a component is kept iff min_size <= size <= max_size (max_size = 0: no upper limit).  The points of dropped components and the points with a
 *   non-finite coordinate have label -1.
 *  Order: clusters are numbered 0 .. n_clusters - 1 by size descending; TIES GO TO THE CLUSTER WHOSE LOWEST ORIGINAL POINT INDEX IS SMALLER (PCL's extract
 *   sorts by size with an unstable sort).  Inside a cluster the point indices are listed in ascending original index.
 *  Per cluster: size; lowest original index; bounding box, float min / max per axis, exact (-0.0 orders below +0.0); centroid, the mean of x, y, z in double.
 *   The centroid's sum runs over the cluster's points in ascending original index in a fixed shape: chunks of 256 consecutive points, the last one padded
 *   with zeros, each summed by a binary tree (entries 128 apart first, then 64, ... 1); the chunk sums 64 at a time, the last group padded with zeros, each
 *   group by a binary tree (entries 32 apart first, then 16, ... 1), the group sums added in order; then divided by the size.  There are no floating-point
 *   atomics: two runs give the same bytes, and the result is a function of the cluster's point set alone.
 *  The partition, the numbering and every per-cluster value depend neither on the order of the input cloud (up to the renaming of the indices) nor on the
 *   rest of the batch nor on the schedule.
 *  Domain: tolerance finite and > 0; 1 <= min_size <= max_size or max_size = 0; a NULL handle, a handle of another context (a lane included): anything else
 *   is LTM_E_INVALID, detected before the device is touched.  An empty index, or one without a finite point, is valid and gives zero clusters.  The same
 *   index may be listed more than once.  All indices of a call together: fewer than 2^31 target points (LTM_E_UNSUPPORTED beyond).
 *  DEPARTURES from PCL: PCL lists the points of a cluster in the breadth-first order of its region growing and leaves the order of clusters of equal size to
 *   std::sort; here both are canonical.  PCL's max_size default is INT_MAX; here 0 says "no limit".  PCL grows one cluster after the other on one thread
 *   with a radius search per point; here all points of all listed indices hook into a lock-free union-find at once (ltm_k_cluster.hip), which gives the
 *   same partition.
 * ltm_search_cluster clusters ALL listed indices in ONE fixed sequence of launches with ONE read-back by the host (the cluster and point counts of every
 * index, which size the handles); out receives n_idx handles.  Memory comes from the context's pool; the handles of one call share their blocks, which
 * return to the pool when the last of them is freed (ltm_destroy releases what is left); all scratch is back when the call returns, on every error path
 * too, and then no handle is returned.  A cluster set keeps no reference to its index: either may be freed first. */
typedef struct ltm_clusters ltm_clusters;
typedef struct {
    double   tolerance;   /* 0 (must be set)  setClusterTolerance [m] */
    uint32_t min_size;    /* 1                setMinClusterSize */
    uint32_t max_size;    /* 0 = no limit     setMaxClusterSize */
} ltm_cluster_params;
void ltm_cluster_default_params(ltm_cluster_params*);      /* host only, needs no device */
int  ltm_search_cluster(ltm_ctx*, size_t n_idx, ltm_search* const* idx, const ltm_cluster_params*, ltm_clusters** out /* n_idx handles */);
int  ltm_clusters_info(ltm_ctx*, ltm_clusters*, size_t* n_target, size_t* n_clusters, size_t* n_clustered_points);
/* the set's device arrays, borrowed until ltm_clusters_free: labels (int32, n_target, the target's ORIGINAL order, -1 = in no cluster), CSR offsets
 * (n_clusters + 1, uint64) and point indices (int32, n_clustered_points; row c = the points of cluster c in ascending original index) */
int  ltm_clusters_device(ltm_ctx*, ltm_clusters*, const int32_t** labels_dev, const uint64_t** offsets_dev, const int32_t** idx_dev);
/* host copies, any pointer may be NULL: labels n_target, sizes n_clusters, first_idx n_clusters (lowest original index), box6 n_clusters x 6 floats (min xyz, max
 * xyz), centroid3 n_clusters x 3 doubles */
int  ltm_clusters_download(ltm_ctx*, ltm_clusters*, int32_t* labels, uint32_t* sizes, int32_t* first_idx, float* box6, double* centroid3);
/* the clustered points of `cloud` -- the cloud the index was built over: n_target points, else LTM_E_INVALID -- as an ordinary scan set, keyframe c = cluster c in
 * the order of its CSR row: one PCD per object, gridding, Scan Context and ltm_search_build_scanset over the objects work on it unchanged */
int  ltm_clusters_extract(ltm_ctx*, ltm_clusters*, ltm_cloud cloud, ltm_scanset* out);
int  ltm_clusters_free(ltm_ctx*, ltm_clusters*);

/* ------------------------------------------------------------------ planes ---- */
/* RANSAC plane segmentation of the keyframes of a scan set, or of one cloud: pcl::SACSegmentation (setModelType SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE,
 * setMethodType SAC_RANSAC, setDistanceThreshold, setMaxIterations, setAxis, setEpsAngle, setOptimizeCoefficients, segment), the step that takes the ground out
 * of a scan before it is clustered.  The reference does not call it and PCL is not available to compare against; this is what this library takes PCL 1.10's
 * SACSegmentation::segment (RandomSampleConsensus::computeModel over SampleConsensusModelPlane / ...PerpendicularPlane, then optimizeModelCoefficients and
 * selectWithinDistance) to do, as understood.  tools/plane_numpy.py restates this text in numpy and the tests compare against that: for equality in everything
 * but the coefficients.
 *  A RECORD is one keyframe of the range, or the cloud.  Each record is handled on its own: its result depends neither on the rest of the batch, nor on its
 *   keyframe number, nor on the schedule.  Points are the record's points in its own order, position 0 .. n - 1.
 *  Hypotheses: hypothesis h (0 <= h < max_iterations) of a record of n points draws the three positions s_j = ((uint64)mix(seed, h, j) * n) >> 32, j = 0, 1, 2,
 *   with mix the 32-bit hash  x = seed + 0x9E3779B9 * (3 h + j + 1);  x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16  (all modulo
 *   2^32: murmur3's finaliser).  The hypothesis is INVALID if two positions coincide or a drawn point has a non-finite coordinate; there is no redraw.  With
 *   p0, p1, p2 the drawn points converted to double, u = p1 - p0, v = p2 - p0 and N = u x v, every component the difference of two products
 *   (Nx = uy vz - uz vy, Ny = uz vx - ux vz, Nz = ux vy - uy vx), n2 = (Nx Nx + Ny Ny) + Nz Nz; the hypothesis is invalid unless n2 > 0 and finite.
 *   T = (thr thr) n2 with thr the double distance_threshold.
 *  Axis constraint (SACMODEL_PERPENDICULAR_PLANE: the plane's normal lies within eps_angle of the axis): with A the axis and c2 = cos(eps_angle)^2 (the C
 *   library's cos, on the host), the hypothesis is invalid unless  ((Nx Ax + Ny Ay) + Nz Az)^2 >= (c2 n2) ((Ax Ax + Ay Ay) + Az Az).  An axis of (0, 0, 0) means no
 *   constraint, and so does eps_angle >= pi / 2 (1.5707963267948966).
 *  Inlier test: point q is an inlier of a valid hypothesis iff its three coordinates are finite and, with d = (double)q - p0 and
 *   s = (Nx dx + Ny dy) + Nz dz,  s s < T  (strict, as PCL's countWithinDistance).  The count of an invalid hypothesis is 0.  Up to here there is no square
 *   root, no division and no fused multiply-add: only + - x in double.
 *  Best hypothesis: the valid hypothesis with the largest inlier count (its CONSENSUS), ties to the smaller h.  A record without a valid hypothesis (fewer than
 *   three finite points, all coincident, all collinear, every normal outside the angle) has no plane: found = 0, best = -1, coefficients and plane point NaN,
 *   every label 0.
 *  Coefficients (a, b, c, d), a^2 + b^2 + c^2 = 1, and the PLANE POINT the device keeps with them.  Unrefined: n = N / sqrt(n2), plane point p0,
 *   d = -((a p0x + b p0y) + c p0z).  Sign: with a non-zero axis, (a Ax + b Ay) + c Az > 0; without one, or where that sum is 0, the component of largest
 *   magnitude is positive (the lower axis among equals), the rule of "normals".
 *  Refinement (refine != 0; setOptimizeCoefficients(true), PCL's default): the moments of the best hypothesis's inliers about its p0 in double -- sum d and the
 *   six sums dx dx, dx dy, dx dz, dy dy, dy dz, dz dz; the count is the consensus -- summed in the fixed shape of "clusters" over the record's points in their
 *   own order: chunks of 256 consecutive points of the record, points that are no inliers entering as zeros and the last chunk padded with zeros, each chunk
 *   by a binary tree (entries 128 apart first, then 64, ... 1); the chunk sums 64 at a time, the last group padded with zeros, each group by a binary tree
 *   (32 apart first, ... 1), the group sums added in order.  The normal is the eigenvector of the smallest eigenvalue of the covariance
 *   (sum d d^T / count - m m^T, m = sum d / count, with 1 / count formed once and multiplied) by the cyclic Jacobi iteration of "normals" -- one routine for
 *   both (ltm_covariance.h) -- normalised, signed as above.  The plane point is c = p0 + sum d / count (a division), d = -((a cx + b cy) + c cz).  The
 *   refinement is SKIPPED, and the unrefined plane stands with refined = 0, when the consensus is below 3, when the two smallest eigenvalues coincide, or
 *   when the eigenvector is not finite.
 *  Labels: the inliers are selected again with the final plane, refined or not (PCL: selectWithinDistance after optimizeModelCoefficients): label 1 iff the
 *   point is finite and |(a ex + b ey) + c ez| < thr with e = (double)q - plane point.  n_inliers is the number of labels set; without refinement it may
 *   differ from the consensus by points within rounding of the threshold, because the unit normal is rounded.
 *  Domain: distance_threshold finite and > 0; 1 <= max_iterations <= 4096; axis finite; with a non-zero axis eps_angle finite and >= 0; kf_begin <= kf_end <=
 *   n_kf; a record has fewer than 2^31 points (LTM_E_UNSUPPORTED beyond).  A handle of another context (a lane included), a NULL pointer or anything else
 *   outside the domain: LTM_E_INVALID before the device is touched, and no handle is returned (*out = NULL).  An empty range and empty keyframes are valid.
 *  DEPARTURES from PCL: all max_iterations hypotheses are always evaluated (PCL stops early by its probability rule); the draws come from the hash above, not
 *   rand(), and a degenerate draw is not repeated; PCL's perpendicular-plane model tests the angle with acos, here squared cosines are compared; the sign of
 *   the coefficients is canonical; PCL's optimizeModelCoefficients takes the eigenvector from Eigen's solver, here from the Jacobi iteration.
 * The count kernel gives a workgroup LTM_PLANE_BLOCK_POINTS consecutive points of one record (ltm_plane_block_points() returns it).
 * ltm_scanset_segment_planes segments ALL keyframes of the range in ONE fixed sequence of launches and returns ONE handle; it reads nothing back from the
 * device (two small tables go up) and returns with the launches queued on the context's stream.  Memory comes from the context's pool; scratch is back when
 * the call returns, on every error path too; ltm_destroy releases open handles. */
#define LTM_PLANE_BLOCK_POINTS 2048
typedef struct ltm_planes ltm_planes;
typedef struct {
    double   distance_threshold;   /* 0 (must be set)  setDistanceThreshold [m] */
    uint32_t max_iterations;       /* 128              setMaxIterations: hypotheses per record, all evaluated */
    uint32_t seed;                 /* 0                of the draws */
    double   axis[3];              /* (0, 0, 0)        setAxis; zero = SACMODEL_PLANE, non-zero = SACMODEL_PERPENDICULAR_PLANE */
    double   eps_angle;            /* 0                setEpsAngle [rad] */
    int32_t  refine;               /* 1                setOptimizeCoefficients */
} ltm_plane_params;
void     ltm_plane_default_params(ltm_plane_params*);      /* host only, needs no device */
uint32_t ltm_plane_block_points(void);                     /* LTM_PLANE_BLOCK_POINTS; host only */
int  ltm_scanset_segment_planes(ltm_ctx*, ltm_scanset, size_t kf_begin, size_t kf_end, const ltm_plane_params*, ltm_planes** out /* one handle */);
int  ltm_cloud_segment_plane(ltm_ctx*, ltm_cloud, const ltm_plane_params*, ltm_planes** out /* one record */);
int  ltm_planes_info(ltm_ctx*, ltm_planes*, size_t* n_records, size_t* n_points, uint32_t* max_iterations);
/* the set's device arrays, borrowed until ltm_planes_free: labels (uint8, n_points, the order of the scan set's range / the cloud), hypothesis inlier counts
 * (uint32, n_records x max_iterations, 0 where invalid) and valid bytes (uint8, n_records x max_iterations) */
int  ltm_planes_device(ltm_ctx*, ltm_planes*, const uint8_t** labels_dev, const uint32_t** hyp_counts_dev, const uint8_t** hyp_valid_dev);
/* host copies, any pointer may be NULL: per record found, best (-1: none), consensus, n_valid (valid hypotheses), n_inliers (labels set), refined, coeff4
 * (n_records x 4 doubles), point3 (n_records x 3 doubles); labels n_points; hyp_counts and hyp_valid n_records x max_iterations */
int  ltm_planes_download(ltm_ctx*, ltm_planes*, uint8_t* found, int32_t* best, uint32_t* consensus, uint32_t* n_valid, uint32_t* n_inliers, uint8_t* refined,
                         double* coeff4, double* point3, uint8_t* labels, uint32_t* hyp_counts, uint8_t* hyp_valid);
/* The scan set the handle was made from -- the same keyframe range with the same point counts, else LTM_E_INVALID -- split by the labels into two scan sets
 * with the keyframes of the range: the inliers and the rest, input order kept (the order-preserving compaction of ltm_knn_partition).  The ONE call of the
 * section that reads back (the sizes).  ltm_planes_split_cloud is its twin for a handle of ltm_cloud_segment_plane and returns two clouds. */
int  ltm_planes_split_scanset(ltm_ctx*, ltm_planes*, ltm_scanset, ltm_scanset* inliers, ltm_scanset* rest);
int  ltm_planes_split_cloud(ltm_ctx*, ltm_planes*, ltm_cloud, ltm_cloud* inliers, ltm_cloud* rest);
int  ltm_planes_free(ltm_ctx*, ltm_planes*);

/* --------------------------------------------------------- outlier filters ---- */
/* Statistical and radius outlier removal over the targets of search indices: pcl::StatisticalOutlierRemoval (setMeanK, setStddevMulThresh, filter) and
 * pcl::RadiusOutlierRemoval (setRadiusSearch, setMinNeighborsInRadius, filter), the filters that go between the other steps: they take the isolated speckle
 * out of a change map before it is clustered and the stray returns out of a scan before normals, ICP, RANSAC or a Scan Context see them.  The reference
 * calls neither and PCL is not available to compare against; this is what this library takes PCL 1.10's two applyFilterIndices to do, as understood.
 * tools/outlier_numpy.py restates this text in numpy and the tests compare against that, for equality.
 *  A RECORD is one listed index (ltm_search_build or ltm_search_build_scanset; the same index may be listed more than once).  A record's result is a function
 *   of its index and the parameters alone: it depends neither on the rest of the batch nor on the schedule, and there are no floating-point atomics.  The
 *   points are the index's target points in their ORIGINAL order, position 0 .. n_target - 1; n_finite of them have three finite coordinates.  d2 is the
 *   index's own distance (FLANN's L2_Simple in float, ((dx*dx)+dy*dy)+dz*dz, no fused multiply-add).
 *  STATISTICAL, 1 <= mean_k <= 63 (the neighbourhood is mean_k + 1 <= 64 points, the limit of ltm_knn_search), stddev_mul finite (negative allowed, as in
 *   PCL):
 *   Neighbourhood of a finite point: its min(mean_k + 1, n_finite) nearest finite target points in the order of ltm_knn_search, the point itself among them
 *    at distance 0.
 *   Distance d_i = (float)(S / mean_k), S the sum in double of sqrt((double)d2_j) over the neighbours AFTER THE FIRST in ascending d2 (equal d2 give equal
 *    terms, so the order among them cannot matter); sqrt and / are the correctly rounded IEEE operations.  mean_k stays the divisor when the index holds
 *    fewer than mean_k + 1 finite points (the convention of ltm_knn_partition).  A non-finite point has d_i = 0.
 *   Record statistics in double over the d_i in original order (n_target entries, the zeros of the non-finite points included, as PCL adds them):
 *    sum = SUM d_i and sq_sum = SUM (double)d_i (double)d_i, each in the fixed shape of "clusters": chunks of 256 consecutive positions, the last one padded
 *    with zeros, each summed by a binary tree (entries 128 apart first, then 64, ... 1); the chunk sums 64 at a time, the last group padded with zeros, each
 *    group by a binary tree (32 apart first, ... 1), the group sums added in order to 0.  With n = n_finite:  mean = sum / n;  variance =
 *    (sq_sum - (sum sum) / n) / (n - 1), and a variance that is not above 0 is 0;  stddev = sqrt(variance);  threshold = mean + stddev_mul stddev -- in
 *    the order written, no fused multiply-add.  n < 2: stddev = 0.  n = 0: mean = stddev = threshold = 0.
 *   Label 1 (kept) iff the point is finite and (double)d_i <= threshold.
 *  RADIUS, radius finite and > 0, min_neighbors >= 1:
 *   neighbours_i = the number of finite target points j, i itself included, with d2(i, j) < r2, r2 = (float)((double)radius * radius), strict <: exactly the
 *    relation of ltm_radius_search and of "clusters".  The stored count is min(neighbours_i, min_neighbors): the walk stops as soon as it is reached.
 *   Label 1 (kept) iff the point is finite and its count equals min_neighbors.  A non-finite point has count 0.
 *  Both: labels are uint8 in the target's original order; per record n_target, n_finite and n_kept (labels set), for the statistical filter also mean, stddev
 *   and threshold.
 *  Domain: the parameter ranges above; a NULL pointer, a NULL handle, a handle of another context (a lane included) or a parameter outside its range is
 *   LTM_E_INVALID before the device is touched, and no handle is returned (*out = NULL).  An empty index, one without a finite point and an empty list are
 *   valid.  All indices of a call together: fewer than 2^31 target points (LTM_E_UNSUPPORTED beyond).
 *  DEPARTURES from PCL: non-finite points are removed (PCL 1.10 gives them distance 0 and so keeps them; they still enter the statistics as zeros over
 *   n_finite, as written above); the variance is clamped at 0 (PCL takes the square root of a negative rounding residue and then removes every point);
 *   stddev = 0 below two points; the sums have the fixed shape above (PCL adds in index order); there are no `negative` / `keep_organized` flags (the split
 *   gives both sides); the radius filter's counts saturate at min_neighbors.
 * Each filter call handles ALL listed indices in ONE fixed sequence of launches and returns ONE handle with n_idx records; it reads nothing back from the
 * device (small tables go up) and returns with the launches queued on the context's stream.  Memory comes from the context's pool; scratch is back when the
 * call returns, on every error path too; the handle keeps no reference to its indices (either may be freed first); ltm_destroy releases open handles. */
#define LTM_OUTLIERS_STATISTICAL 0
#define LTM_OUTLIERS_RADIUS      1
typedef struct ltm_outliers ltm_outliers;
typedef struct {
    uint32_t mean_k;          /* 1     setMeanK (PCL's constructor) */
    double   stddev_mul;      /* 0.0   setStddevMulThresh */
} ltm_sor_params;
typedef struct {
    double   radius;          /* 0 (must be set)  setRadiusSearch [m] */
    uint32_t min_neighbors;   /* 1                setMinNeighborsInRadius */
} ltm_ror_params;
void ltm_sor_default_params(ltm_sor_params*);      /* host only, needs no device; NULL is a no-op */
void ltm_ror_default_params(ltm_ror_params*);
/* pcl::StatisticalOutlierRemoval::filter / pcl::RadiusOutlierRemoval::filter over every listed index */
int  ltm_search_filter_statistical(ltm_ctx*, size_t n_idx, ltm_search* const* idx, const ltm_sor_params*, ltm_outliers** out /* one handle */);
int  ltm_search_filter_radius(ltm_ctx*, size_t n_idx, ltm_search* const* idx, const ltm_ror_params*, ltm_outliers** out /* one handle */);
int  ltm_outliers_info(ltm_ctx*, ltm_outliers*, int* kind /* LTM_OUTLIERS_... */, size_t* n_records, size_t* n_points /* the records' n_target, summed */);
/* the set's device arrays, borrowed until ltm_outliers_free: record offsets (uint64, n_records + 1: record r has positions [off[r], off[r + 1])), labels (uint8,
 * n_points) and, per position, distances (float; NULL for a radius set) or counts (uint32; NULL for a statistical set) */
int  ltm_outliers_device(ltm_ctx*, ltm_outliers*, const uint64_t** offsets_dev, const uint8_t** labels_dev, const float** distances_dev,
                         const uint32_t** counts_dev);
/* host copies, any pointer may be NULL: per record n_target, n_finite, n_kept, mean, stddev, threshold; per position labels, distances, counts.  Asking a
 * radius set for statistics or distances, or a statistical set for counts, is LTM_E_INVALID */
int  ltm_outliers_download(ltm_ctx*, ltm_outliers*, uint32_t* n_target, uint32_t* n_finite, uint32_t* n_kept, double* mean, double* stddev, double* threshold,
                           uint8_t* labels, float* distances, uint32_t* counts);
/* A scan set with one keyframe per record, keyframe r with as many points as record r's target (the scan set the indices were built over), else
 * LTM_E_INVALID, split by the labels into two scan sets with the same keyframes: the kept points and the removed ones, input order kept on both sides (the
 * planes' split path).  The ONE call of the section that reads back (the sizes).  ltm_outliers_split_cloud is its twin for a handle of ONE record and
 * returns two clouds. */
int  ltm_outliers_split_scanset(ltm_ctx*, ltm_outliers*, ltm_scanset, ltm_scanset* kept, ltm_scanset* removed);
int  ltm_outliers_split_cloud(ltm_ctx*, ltm_outliers*, ltm_cloud, ltm_cloud* kept, ltm_cloud* removed);
int  ltm_outliers_free(ltm_ctx*, ltm_outliers*);

/* -------------------------------------------------------------------- fpfh ---- */
/* Fast Point Feature Histograms (Rusu, Blodow, Beetz 2009) of the target points of search indices: pcl::FPFHEstimation (setInputCloud, setInputNormals,
 * setKSearch, compute), 33 floats per point, the local shape descriptor that feature matching and a sample-consensus initial alignment start from.  The
 * reference does not call it and PCL is not available to compare against; this is what this library takes PCL 1.10's computeFeature, computePairFeatures,
 * computePointSPFHSignature and weightPointSPFHSignature to do, as understood.  tools/fpfh_numpy.py restates this text in numpy and the tests compare
 * against that, for equality.
 *  A RECORD is one listed index (ltm_search_build or ltm_search_build_scanset, mixed freely) that has normals (ltm_search_estimate_normals); the normals
 *   are the stored (nx, ny, nz) as floats.  A record's result is a function of its index and k alone: it depends neither on the rest of the batch nor on
 *   the schedule, and there are no floating-point atomics.  Rows are in the target's ORIGINAL order.  2 <= k <= 64.
 *  NEIGHBOURHOOD of a finite point p: its kk = min(k, n_finite) nearest finite target points in the order of ltm_knn_search (float L2_Simple,
 *   ((dx*dx)+dy*dy)+dz*dz, ties to the smaller target index), as (d2_j, q_j), j = 0 .. kk - 1.  p is among them unless k or more points coincide with it.
 *  PAIR FEATURES of (p, q) for every q of the neighbourhood with a different target index, in double with + - * / sqrt only, each rounded once (no
 *   fused multiply-add); a dot product is (a.x b.x + a.y b.y) + a.z b.z, a cross product a x b = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x):
 *    1. d = q - p, f4 = sqrt(d.d).  f4 == 0: the pair is skipped.  A q whose normal has a non-finite component: skipped as well.
 *    2. a1 = (n_p.d) / f4, a2 = (n_q.d) / f4.
 *    3. |a1| < |a2|: u = n_q, o = n_p, d = -d, phi = -a2; otherwise u = n_p, o = n_q, phi = a1.
 *    4. v = d x u, vn = sqrt(v.v).  vn == 0: skipped.  v = v / vn (three divisions), w = u x v.
 *    5. alpha = v.o, y = w.o, x = u.o (theta would be atan2(y, x)).
 *  BINS, 11 per feature.  alpha and phi: floor(11 ((f + 1) 0.5)) clamped to 0 .. 10.  theta, without a transcendental: the number of boundaries
 *   theta_j = -pi + 2 pi j / 11, j = 1 .. 10, that the direction (x, y) has reached.  With (c_j, s_j) the doubles nearest (cos theta_j, sin theta_j),
 *     j  1  (-0.8412535328311811,  -0.5406408174555978)     j  6  ( 0.9594929736144975,   0.2817325568414295)
 *     j  2  (-0.4154150130018863,  -0.9096319953545184)     j  7  ( 0.6548607339452851,   0.7557495743542583)
 *     j  3  ( 0.14231483827328512, -0.9898214418809327)     j  8  ( 0.14231483827328512,  0.9898214418809327)
 *     j  4  ( 0.6548607339452851,  -0.7557495743542583)     j  9  (-0.41541501300188616,  0.9096319953545186)
 *     j  5  ( 0.9594929736144975,  -0.2817325568414295)     j 10  (-0.8412535328311813,   0.5406408174555974)
 *   side_j = (c_j y - s_j x >= 0) (two products, one difference) and upper = (the sign bit of y is clear: y > 0 or y == +0).  Boundary j <= 5 is reached
 *   iff upper or side_j; boundary j >= 6 iff upper and side_j.  x == 0 and y == 0 (either sign): bin 5.  So y == +0 with x < 0 (theta = +pi) is bin 10,
 *   y == -0 with x < 0 (theta = -pi) is bin 0, y == +-0 with x > 0 is bin 5, as PCL's floor(11 (theta + pi) / (2 pi)), clamped, gives them.  The rule and
 *   that expression on numpy's arctan2 differ only within 1e-15 rad of a boundary (tests/test_fpfh_cases_cpu.py measures it).
 *  SPFH of p: 33 integer counts, count[f][b] += 1 per feature f of every pair that was not skipped (at most 63 per feature).  On the device: four 64-bit
 *   words per point, bins 0 .. 9 of feature f as 6-bit fields of word f (bin b at bit 6 b), the number of counted pairs in word 3; bin 10 is that number
 *   less the ten fields.  ltm_fpfh_download unpacks them to uint8 [33].
 *  FPFH of p: S_b = SUM_j (1.0 / (double)d2_j) * (double)count_{q_j}[b], added in list order to 0.0, a j with d2_j == 0 left out (so p's own SPFH is not
 *   in it, as in weightPointSPFHSignature).  Per group of 11 bins, T = the sum of its S_b in bin order; row[b] = (float)(100.0 * S_b / T), the product
 *   first; a group with T == 0 stays 0.
 *  DEGENERATE ROWS: a position with a non-finite coordinate, and a point whose normal has a non-finite component, have 33 NaN floats and zero counts.
 *   An index with fewer than 3 finite points has NaN normals ("normals"), so a target with fewer than 2 finite points gives NaN rows throughout.
 *  Domain: a NULL pointer, a NULL handle, a handle of another context (a lane included), an index without normals, the same index listed twice or k
 *   outside 2 .. 64 is LTM_E_INVALID before the device is touched; no handle is returned (*out = NULL) and every index stays as it was.  An empty index and
 *   an empty list are valid.  All indices of a call together: fewer than 2^31 target points (LTM_E_UNSUPPORTED beyond).
 *  DEPARTURES from PCL: step 3 compares |a1| < |a2| where PCL compares acos(|a1|) > acos(|a2|) (different only where the two roundings differ); the
 *   theta bin by sign tests as above; the SPFH holds counts where PCL adds 100 / (n - 1) in float per pair (the factor is the same for every point of an
 *   index and cancels in the normalisation); the weighted sums and the normalisation are double, rounded to float once (PCL: float throughout); a pair
 *   with a non-finite normal is skipped and such a point has a NaN row (PCL requires finite normals); only k neighbourhoods (no setRadiusSearch).
 * The call handles ALL listed indices in ONE fixed sequence of launches and returns ONE handle with n_idx records; it reads nothing back from the device
 * (small tables go up) and returns with the launches queued on the context's stream.  Memory comes from the context's pool; the handle keeps no reference
 * to its indices (either may be freed first, and estimating normals again does not touch it); ltm_destroy releases open handles.  The neighbour lists of
 * the first pass are kept as scratch for the second where they take at most 16 GiB (8 bytes per finite point and k) and the pool has them; otherwise, and
 * in a context created with LTM_FPFH_LISTS=0, the second pass collects the neighbourhoods again: the same bytes either way. */
typedef struct ltm_fpfh ltm_fpfh;
int  ltm_search_fpfh(ltm_ctx*, size_t n_idx, ltm_search* const* idx, int k, ltm_fpfh** out /* one handle, one record per index */);
int  ltm_fpfh_info(ltm_ctx*, ltm_fpfh*, size_t* n_records, size_t* n_points /* the records' n_target, summed */, int* k);
/* the set's device arrays, borrowed until ltm_fpfh_free: record offsets (uint64, n_records + 1: record r has rows [off[r], off[r + 1])), the descriptors
 * (float, n_points x 33, row-major) and the SPFH words (uint64, n_points x 4, as above).  Any pointer may be NULL */
int  ltm_fpfh_device(ltm_ctx*, ltm_fpfh*, const uint64_t** offsets_dev, const float** desc_dev /* n_points x 33 */, const void** spfh_dev);
/* host copies, any pointer may be NULL: per record n_target and n_finite; per position the descriptor and the unpacked counts */
int  ltm_fpfh_download(ltm_ctx*, ltm_fpfh*, uint32_t* n_target, uint32_t* n_finite, float* desc /* n_points x 33 */, uint8_t* spfh_counts /* n_points x 33, nullable */);
int  ltm_fpfh_free(ltm_ctx*, ltm_fpfh*);
/* A descriptor set from rows the caller supplies: n_records records, record r the rows [offsets[r], offsets[r + 1]) of desc_host (offsets[0] = 0, not
 * decreasing, fewer than 2^31 rows in all), 33 floats per row, copied as they are (NaN and infinite components included).  Its k reads 0, its SPFH words
 * and counts are zero, n_target of a record is its row count and n_finite the number of its rows without a NaN component; everything else behaves as for
 * a handle of ltm_search_fpfh.  For matching any 33-float descriptor (below).  A NULL pointer or offsets outside the rule: LTM_E_INVALID, *out = NULL. */
int  ltm_fpfh_upload(ltm_ctx*, size_t n_records, const uint64_t* offsets /* n_records + 1 */, const float* desc_host /* rows x 33 */, ltm_fpfh** out);

/* ------------------------------------------------------------ fpfh matches ---- */
/* Feature-space correspondences between records of descriptor sets: for every row of a SOURCE record its kc nearest rows of a TARGET record, the search that
 * pcl::SampleConsensusPrerejective (setSourceFeatures, setTargetFeatures, setCorrespondenceRandomness) runs over its FPFH rows and the first half of an
 * initial alignment from descriptors.  The reference does not call it and PCL is not available to compare against.  tools/sac_numpy.py restates this text
 * in numpy and the tests compare against that: target rows for equality, distances bit for bit.
 *  A RECORD of the result is one PAIR: pair i matches the rows of record source_rec[i] of source_set against the rows of record target_rec[i] of
 *   target_set.  The two sets may be the same handle, and a record may serve any number of pairs.  A pair's result is a function of its two records and kc
 *   alone: it depends neither on the rest of the batch nor on the schedule.  Rows are numbered within their record, 0 .. n - 1, in the record's own order
 *   (for a set of ltm_search_fpfh: the target's ORIGINAL order).  1 <= kc <= 16.
 *  DISTANCE of source row s and target row t, in float, no fused multiply-add, bins in order:
 *    acc = 0;  for b = 0 .. 32:  e = s[b] - t[b];  acc = acc + e * e.
 *  ELIGIBLE: a target row with a NaN component is not eligible; a source row with a NaN component has no matches.  (Infinite components are not tested:
 *   their distances are +inf, or NaN where two infinities meet, and a candidate whose distance is NaN is not listed.)
 *  LIST of a source row without NaN: the kk = min(kc, listable target rows) smallest candidates in ascending order of (distance, target row): ties go to
 *   the smaller row.  Output per source row: kc slots of (int32 target row, float distance), slots kk .. kc - 1 holding (-1, +inf).
 *  Output layout: the pairs' source rows one after the other, offsets (n_pairs + 1) saying where each pair's begin; indices and distances are
 *   n_rows x kc, row-major.
 *  Domain: a NULL pointer, a handle that is not a descriptor set of this context (a lane's included), a record number outside its set, or kc outside
 *   1 .. 16 is LTM_E_INVALID before the device is touched, and no handle is returned (*out = NULL).  Empty records and n_pairs = 0 are valid.  All pairs of
 *   a call together: fewer than 2^31 source rows (LTM_E_UNSUPPORTED beyond).
 *  DEPARTURE from PCL: PCL searches a FLANN kd-tree over the 33-D rows (approximate beyond its checks, and in its own tie order); here the search is
 *   exhaustive and therefore exact.
 * The kernel stages LTM_MATCH_TILE_ROWS target rows at a time (ltm_match_tile_rows() returns it).  The call handles ALL pairs in ONE launch and returns ONE
 * handle; it reads nothing back from the device (two small tables go up) and returns with the launch queued on the context's stream.  Memory comes from
 * the context's pool; scratch is back when the call returns, on every error path too; the handle keeps no reference to the descriptor sets (either may be
 * freed first); ltm_destroy releases open handles. */
#define LTM_MATCH_TILE_ROWS 128
#define LTM_MATCH_MAX_KC    16
typedef struct ltm_matches ltm_matches;
uint32_t ltm_match_tile_rows(void);                        /* LTM_MATCH_TILE_ROWS; host only */
int  ltm_fpfh_match(ltm_ctx*, size_t n_pairs, ltm_fpfh* target_set, const uint32_t* target_rec, ltm_fpfh* source_set, const uint32_t* source_rec, int kc,
                    ltm_matches** out /* one handle, one record per pair */);
int  ltm_matches_info(ltm_ctx*, ltm_matches*, size_t* n_pairs, size_t* n_rows /* the pairs' source rows, summed */, int* kc);
/* the set's device arrays, borrowed until ltm_matches_free: pair offsets (uint64, n_pairs + 1: pair i has rows [off[i], off[i + 1])), target rows (int32,
 * n_rows x kc) and distances (float, n_rows x kc).  Any pointer may be NULL */
int  ltm_matches_device(ltm_ctx*, ltm_matches*, const uint64_t** offsets_dev, const int32_t** indices_dev, const float** distances_dev);
/* host copies, any pointer may be NULL: per pair the rows of its source and of its target record; per source row and slot the target row and distance */
int  ltm_matches_download(ltm_ctx*, ltm_matches*, uint32_t* n_source, uint32_t* n_target, int32_t* indices, float* distances);
int  ltm_matches_free(ltm_ctx*, ltm_matches*);

/* ------------------------------------------------------- initial alignment ---- */
/* Sample-consensus initial alignment of loop pairs from their feature matches: pcl::SampleConsensusPrerejective (setMaximumIterations,
 * setNumberOfSamples(3), setCorrespondenceRandomness, setSimilarityThreshold, setMaxCorrespondenceDistance, setInlierFraction, align), the step that gives
 * ltm_icp_align* an init16 inside its basin when the prior is poor.  The reference does not call it and PCL is not available to compare against; this is
 * what this library takes PCL 1.10's computeTransformation to do, with the departures listed below.  tools/sac_numpy.py restates this text in numpy and
 * the tests compare against that, for equality, the transform bit for bit.
 *  A RECORD is one pair: targets[i] and sources[i] are search indices (ltm_search_build or ltm_search_build_scanset; an index may serve many pairs) and
 *   pair i of the match handle holds, for every row of the source, target rows of the target: ROWS are positions of the index's cloud in its ORIGINAL
 *   order (the rows of ltm_search_fpfh), so the source index has as many target points as the match record has source rows, and the target index as
 *   many as the record's target had rows.  A record's result is a function of its two indices, its match record and the parameters alone: it depends
 *   neither on the rest of the batch nor on the schedule, and there are no floating-point atomics.
 *  DRAWS: hypothesis h (0 <= h < max_iterations) uses mix_j = the hash of "planes" with x = seed + 0x9E3779B9 * (6 h + j + 1), j = 0 .. 5.  Source rows
 *   s_j = ((uint64)mix_j * n_rows) >> 32, j = 0, 1, 2, over ALL n_rows rows of the source.  Match of row s_j: m_j = ((uint64)mix_{3+j} * kk_j) >> 32 among
 *   the kk_j filled slots of the row's list, giving the target row t_j.  The hypothesis is INVALID when two source rows coincide, a drawn row's point has
 *   a non-finite coordinate, a drawn row has no match (kk_j = 0), two matched target rows coincide, or a matched target point is non-finite.  There is no
 *   redraw.
 *  PREREJECTION (CorrespondenceRejectorPoly), in double with + - x only: with a_j the source points and b_j the target points as doubles, for the edges
 *   (0,1), (1,2), (2,0): ls = |a_i - a_k|^2 and lt = |b_i - b_k|^2, each (dx dx + dy dy) + dz dz with d the first point less the second; the hypothesis
 *   is invalid (and counted in n_prerejected) unless  min(ls, lt) >= (thr thr) max(ls, lt)  on every edge, thr the double similarity_threshold.
 *  TRANSFORM, in double with + - x / sqrt, each rounded once, no fused multiply-add (the discipline of "fpfh"; cross products as there).  Frame of a
 *   triangle (a0, a1, a2): u = a1 - a0, e1 = u / sqrt(u.u) (three divisions); n = u x (a2 - a0), e3 = n / sqrt(n.n); e2 = e3 x e1.  The hypothesis is
 *   invalid if u.u or n.n, on either side, is 0 or not finite.  With f the source's frame and g the target's:  R_rc = (g1_r f1_c + g2_r f2_c) + g3_r f3_c.
 *   With the centroids c = ((a0 + a1) + a2) / 3.0 per component, cs of the source and ct of the target:  t_r = ct_r - ((R_r0 cs_x + R_r1 cs_y) + R_r2 cs_z).
 *   So the rotation is exact in the first edge and in the triangle's plane, the translation at the centroids.
 *  VOTE: the voting points are the finite source points at positions 0, eval_stride, 2 eval_stride, ... of the source index's own order (its finite points
 *   in the code order of its own frame; among points of equal code the order is the index's own); n_eval = ceil(n_finite / eval_stride).  A voting point
 *   is transformed as in step 1 of "icp" (double, rounded to float; a query that overflows is skipped) and is an INLIER iff some finite target point has
 *   float L2_Simple distance d2 to the query with (double)d2 <= inlier_distance inlier_distance.  The count of an invalid hypothesis is 0.
 *  BEST: the valid hypothesis with the largest count (its CONSENSUS), ties to the smaller h.  found = ((double)consensus >= inlier_fraction (double)n_eval
 *   and consensus >= 3).  The record: found, best (-1: no valid hypothesis), consensus, n_valid, n_prerejected, n_eval and T (16 doubles, row-major, last
 *   row 0 0 0 1; all NaN if best = -1).  hyp_counts and hyp_valid are kept per pair, n_pairs x max_iterations, as in "planes".
 *  Domain: 1 <= max_iterations <= 16384; 0 <= similarity_threshold < 1; inlier_distance finite and > 0; 0 <= inlier_fraction <= 1; eval_stride >= 1.  A
 *   NULL pointer, a handle of another context (a lane included), n_pairs different from the match handle's number of pairs, an index whose number of
 *   target points differs from the rows of its match record, or a parameter outside its range (NaN included) is LTM_E_INVALID before the device is
 *   touched, and no handle is returned (*out = NULL).  Empty indices and n_pairs = 0 are valid.  The distinct indices of a call together: fewer than 2^31
 *   target points (LTM_E_UNSUPPORTED beyond).
 *  DEPARTURES from PCL: PCL estimates the transform by the SVD of the three pairs, here it comes from the two frames; PCL draws with rand() and redraws a
 *   degenerate or prerejected sample, here the draws come from the hash and there is no redraw; PCL ranks by the inliers' mean squared error under the
 *   inlier-fraction gate, here by the count; PCL does not evaluate a hypothesis it has already beaten, here ALL max_iterations hypotheses are
 *   evaluated in full; eval_stride is an addition.  The least-squares fit over the winner's inliers is not here: one ltm_icp_align
 *   iteration started from T with max_corr_dist = inlier_distance is that fit.
 * The vote kernel gives a workgroup LTM_SAC_BLOCK_POINTS voting points of one pair (ltm_sac_block_points() returns it).  ltm_sac_align handles ALL pairs in
 * ONE fixed sequence of launches and returns ONE handle; it reads nothing back from the device (small tables go up) and returns with the launches queued
 * on the context's stream.  Memory comes from the context's pool; scratch is back when the call returns, on every error path too; the handle keeps no
 * reference to its indices or matches; ltm_destroy releases open handles. */
#define LTM_SAC_BLOCK_POINTS 1024
typedef struct ltm_sac ltm_sac;
typedef struct {
    uint32_t max_iterations;        /* 1000   setMaximumIterations: hypotheses per pair, all evaluated; 1 .. 16384 */
    uint32_t seed;                  /* 0      of the draws */
    double   similarity_threshold;  /* 0.9    setSimilarityThreshold, in [0, 1) */
    double   inlier_distance;       /* 0 (must be set)  setMaxCorrespondenceDistance [m] */
    double   inlier_fraction;       /* 0.25   setInlierFraction, in [0, 1] */
    uint32_t eval_stride;           /* 1      every eval_stride-th finite source point, in the source index's own order, votes */
} ltm_sac_params;
void     ltm_sac_default_params(ltm_sac_params*);          /* host only, needs no device; NULL is a no-op */
uint32_t ltm_sac_block_points(void);                       /* LTM_SAC_BLOCK_POINTS; host only */
int  ltm_sac_align(ltm_ctx*, size_t n_pairs, ltm_search* const* targets, ltm_search* const* sources, ltm_matches* matches /* pair i of the handle */,
                   const ltm_sac_params*, ltm_sac** out /* one handle, one record per pair */);
int  ltm_sac_info(ltm_ctx*, ltm_sac*, size_t* n_pairs, uint32_t* max_iterations);
/* the set's device arrays, borrowed until ltm_sac_free: hypothesis inlier counts (uint32, n_pairs x max_iterations, 0 where invalid) and valid bytes */
int  ltm_sac_device(ltm_ctx*, ltm_sac*, const uint32_t** hyp_counts_dev, const uint8_t** hyp_valid_dev);
/* host copies, any pointer may be NULL: per pair found, best, consensus, n_valid, n_prerejected, n_eval, T16 (n_pairs x 16 doubles: what ltm_icp_align*
 * takes as init16); hyp_counts and hyp_valid n_pairs x max_iterations */
int  ltm_sac_download(ltm_ctx*, ltm_sac*, uint8_t* found, int32_t* best, uint32_t* consensus, uint32_t* n_valid, uint32_t* n_prerejected, uint32_t* n_eval,
                      double* T16, uint32_t* hyp_counts, uint8_t* hyp_valid);
int  ltm_sac_free(ltm_ctx*, ltm_sac*);

/* ------------------------------------------------------------------- lanes ---- */
/* The reference runs the stages of Removerter::run() one after the other on one thread; several of them do not depend on each other: the
 * central and the query session's makeGlobalMap + Step-1 chains (Removerter.cpp:213-252, :1580-1587), their HD kNN maps and static reprojections
 * (:1590-1601, :1527-1538), the two directions of the LD kNN diff (:1418-1421), filterStrongND against filterStrongPD (:1395-1411), the grids of
 * :1445-1476 and the six reprojections of :1551-1577.  A LANE is a second context on the parent's device (own stream, own pool, the parent's
 * configuration and create-time self-check) that a second host thread drives; the projection kernels are bound by vector-instruction issue and the
 * grids / kNN stages by launch latency, so the two kinds of work fill each other's gaps.  The library keeps the lanes out of each other's way by
 * itself: the large projection launches of a context and its lanes are chained on the device (one at a time, in the order the hosts submit them),
 * each on its own context's stream -- there is no separate stream and no stream priority --, so that one lane's partition + grids run beside the
 * other lane's projection instead of both lanes projecting together and then idling together.  Results do not depend on the schedule: every kernel
 * sees the same inputs as in the one-lane order.
 *
 *   ltm_lane_create           a context like `parent` (same device, field of view, extrinsic, kernel switches); destroy with ltm_destroy
 *   ltm_cloud_lend / _give    make a cloud of context `from` usable in context `to` WITHOUT copying: `lend` leaves ownership with `from` (the new handle
 *                             is a borrowed view: freeing it releases nothing; `from` must keep its cloud alive and unchanged until the borrower is done
 *                             with it and must order its own later writes / frees after the borrower's reads -- ltm_lane_fence(to, from) or an event);
 *                             `give` moves the memory block into `to`'s pool and invalidates the handle in `from`.  Both make `to`'s stream wait for what
 *                             `from`'s stream has been given so far (the cloud's producer).  Same for scan sets.
 *   ltm_lane_fence(a, b)      everything submitted to b afterwards runs after everything submitted to a so far (device-side; the host does not wait)
 *   ltm_event_record / _wait  the same dependency in two halves, for a consumer on another thread: record on one context, hand the event over by
 *                             whatever means the host language has, wait on the other.  An event may be waited for any number of times.
 * Two contexts are locked in address order by the two-context calls, so they may be issued from either thread. */
typedef struct ltm_event ltm_event;
int  ltm_lane_create(ltm_ctx* parent, ltm_ctx** lane);
int  ltm_lane_fence(ltm_ctx* done_in, ltm_ctx* before_next_of);
int  ltm_event_record(ltm_ctx*, ltm_event** ev);
int  ltm_event_wait(ltm_ctx*, ltm_event* ev);
void ltm_event_destroy(ltm_event* ev);
int  ltm_cloud_lend(ltm_ctx* from, ltm_cloud h, ltm_ctx* to, ltm_cloud* out);
int  ltm_cloud_give(ltm_ctx* from, ltm_cloud h, ltm_ctx* to, ltm_cloud* out);
int  ltm_scanset_lend(ltm_ctx* from, ltm_scanset h, ltm_ctx* to, ltm_scanset* out);
int  ltm_scanset_give(ltm_ctx* from, ltm_scanset h, ltm_ctx* to, ltm_scanset* out);
/* ------------------------------------------------------ parity / debug helpers ---- */
/* one range image of `pts` after optional transforms T1 then T2 (NULL = none); rimg R*C floats,
 * ptidx R*C int32 or NULL.  Host output buffers. */
int ltm_debug_range_image(ltm_ctx*, ltm_cloud pts, const double* T1, const double* T2, float res_alpha,
                          float* rimg, int32_t* ptidx);
/* The four RViz images of one keyframe (Removerter.cpp:580-585 pubRangeImg x4; utility.h:114-127 convertColorMappedImg =
 * 255*(img-min)/(max-min) -> 8 bit -> cv::COLORMAP_JET), computed and colour-mapped on the device so that a ROS host only
 * pays for them when somebody subscribes: scan range image, map range image (both on [range_min, range_max] =
 * rimg_color_min/max), their difference (scan-map for mode 0, map-scan for mode 1, on [diff_min, diff_max] = 0..0.5 in
 * RosParamServer.cpp:12) and the map point-index image (on [0, M]).  Each output is rows*cols*3 bytes BGR8
 * (ltm_rimg_size) in host memory, or NULL to skip it. */
int ltm_debug_viz_images(ltm_ctx*, ltm_cloud map, ltm_scanset scans, ltm_poses poses, size_t kf, float res_alpha, int mode,
                         float range_min, float range_max, float diff_min, float diff_max,
                         uint8_t* scan_bgr, uint8_t* map_bgr, uint8_t* diff_bgr, uint8_t* ptidx_bgr);
/* element-wise device evaluation of the projection arithmetic: out_az_el_r (3n), out_row_col (2n) */
int ltm_debug_project(ltm_ctx*, const float* xyz, size_t n, float res_alpha, float* out_az_el_r, int32_t* out_row_col);
void ltm_rimg_size(float vfov, float hfov, float res_alpha, int* rows, int* cols);   /* utility.cpp:222-236 */
/* result of the create-time exhaustive device self-check of the fast arithmetic forms (rad2deg by multiplication,
 * division by the FOV constants) against plain IEEE division over all 2^32 binary32 inputs:
 * mismatches3 = {rad2deg, /vfov, /hfov}; the fast forms are used only when all three are zero. */
int ltm_debug_selfcheck(ltm_ctx*, uint64_t* mismatches3, int* fast_math_enabled);
/* the elevation polynomial of the bounded-error projection, as fitted when a context with this vertical field of view is created
 * (host arithmetic only, needs no device): atan(t) ~ t (c[0] + u (c[1] + u (c[2] + u c[3]))), u = t^2, on [0, tan(vfov/2 + 2 deg)];
 * *max_err_rad = largest error of its binary32 evaluation.  Returns 1 if the kernels use it for this field of view (vfov/2 + 2 deg
 * <= 45 deg and error <= 1e-6 rad), 0 if they keep the generic polynomial on [0, 1], < 0 on invalid arguments. */
int ltm_debug_elevation_fit(float vfov_deg, float* c4, double* max_err_rad);
/* Host arithmetic only: the point order ltm_voxel_grid_scanset's default (PCL) path gives one keyframe whose points have the leaf indices
 * leaf_idx[0..n) -- the permutation std::sort with pcl::VoxelGrid's leaf-index-only comparator leaves behind (voxel_grid.hpp), computed by
 * lt-mapper_amd/csrc/ltm_pclsort.h (use_std_sort == 0) or by std::sort itself (!= 0); the two must agree (tests/test_abi.py). */
int ltm_debug_pcl_sort_order(const uint32_t* leaf_idx, size_t n, uint32_t* order_out, int use_std_sort, uint32_t* heap_sort_fallbacks /* nullable: how
                             often the restatement went into introsort's heap-sort fallback (0 for std::sort, which does not say) */);
/* the voxel grid's sort key (host arithmetic only, needs no device): for a cloud with bounding box [mn, mx] and leaf size `leaf`, the
 * octree frame (depth, lattice origin) and the mask of the interleaved Morton-code bits (x = bit 3L+2, y = 3L+1, z = 3L of level L)
 * that the radix sort looks at -- the others are functions of more significant bits for every key inside the box and are left out
 * (fewer passes; order and equality of codes are unchanged).  Returns the number of kept bits, or < 0. */
int ltm_debug_voxel_key_bits(const float* mn3, const float* mx3, float leaf, uint64_t* kept_mask, unsigned* depth, double* frame_min3);
/* The launch constants of the projection kernels (k_vote_map_cull, k_map_rimg_blockmin, k_map_rimg_lds, k_map_rimg and the cull check), which the host
 * computes once per launch and passes as a kernel argument, for a context with this field of view and base->lidar extrinsic (4x4 row-major, NULL =
 * identity), the image of `res_alpha`, a map of `map_points` points and `n_keyframes` keyframes in the batch.  Needs no context; host arithmetic unless
 * on_device != 0, which lets one thread of the current device evaluate the same expressions (what every thread did before they moved to the host).
 *   out_f32[16] = half_v, half_h, 1/vfov, 1/hfov, rows, cols, rows - 1, cols - 1, row_scale, col_scale, row_bias, col_bias, 1 - 2 eps, rmin^2, eps, el_tclamp
 *   out_u32[12] = rows, cols, rows * cols, steep_clamps, packable, n_tiles, n_tile_groups, magic, shift, grid size, el_fit, 0
 * and, for the workgroups [first_block, first_block + n_blocks) of that launch, the map tile and the keyframe each one works on (0xffffffff in both
 * for a workgroup with nothing to do): (b >> 6) / n_tile_groups is taken as mulhi(b & ~63, magic) >> shift, exact for every b < 2^32. */
int ltm_debug_proj_launch(float vfov, float hfov, float res_alpha, const double* base2lidar16_or_null, size_t map_points, size_t n_keyframes, int on_device,
                          float* out_f32, uint32_t* out_u32, uint32_t first_block, size_t n_blocks, uint32_t* out_tile, uint32_t* out_kf);
/* The workgroup mapping of the range-culled vote kernel (k_vote_map_cull): one workgroup takes a run of `tile_run` consecutive 4096-point map tiles
 * for one keyframe (context switch LTM_VOTE_TILE_RUN, 1 .. 16, default 4, read by ltm_create; 1 = one tile per workgroup, the mapping
 * ltm_debug_proj_launch reports).  Run r covers tiles [r * run_len, min((r + 1) * run_len, n_tiles)).  For the workgroups [first_block, first_block + n_blocks) of a launch over
 * `map_points` points and `n_keyframes` keyframes: the run and the keyframe each one works on (0xffffffff in both for a workgroup with nothing to do),
 * the run length after clamping and the grid size.  Needs no context and no device; exact for every block index below 2^32.
 * The plain launch of the exact arg-min image kernel (reprojection, mode-1 votes; k_map_rimg_blockmin_run) uses the same mapping with a run length of its own:
 * context switch LTM_MAP_TILE_RUN, 1 .. 16, read by ltm_create (pass it as `tile_run` to see that launch's mapping); when it is not given the run
 * length is 2, halved for a launch that would keep fewer than 16384 workgroups.  Images, labels and reprojected
 * scans are the same bits for every value.  Two A/B switches of that kernel, also read by ltm_create: LTM_MAP_TILE_PERSIST=0 flushes and resets its LDS tables
 * behind every tile of a run, LTM_MAP_TILE_BARRIER=1 puts a barrier between the two halves of its pre-filter; both measured slower.  The list-driven launch
 * behind the occlusion cull keeps one (tile, keyframe) pair per workgroup. */
int ltm_debug_vote_run_launch(size_t map_points, size_t n_keyframes, int tile_run, uint32_t first_block, size_t n_blocks, uint32_t* out_run, uint32_t* out_kf,
                              uint32_t* out_run_len, uint32_t* out_grid);
/* The band plan of k_scan_rimg_lds for a set of image shapes (rows[j] x cols[j], j < n_shapes): one workgroup keeps one band of one keyframe in LDS, a band
 * being rows [out_row0[b * n_shapes + j], out_row0[(b + 1) * n_shapes + j]) of every shape j.  *out_n_bands = 0 (and LTM_OK) for a set the plan cannot serve:
 * more than 8 shapes, a shape without pixels, one row of all shapes together wider than the budget.  out_row0 ((max_bands + 1) * n_shapes entries) and
 * out_bytes (max_bands entries: LDS bytes of each band, at most *out_budget_bytes) are filled for the first min(n_bands, max_bands) bands; all outputs but
 * out_n_bands may be NULL.  Needs no context and no device. */
int ltm_debug_scan_bands(size_t n_shapes, const int32_t* rows, const int32_t* cols, uint32_t* out_n_bands, uint32_t* out_budget_bytes, size_t max_bands,
                         uint32_t* out_row0, uint32_t* out_bytes);
/* The scan range images of keyframes [kf_begin, kf_end) for one resolution as the votes see them, cached or built now: img_out ((kf_end - kf_begin) * rows * cols
 * floats, 10000 = empty), smax_out (one float per keyframe: the largest non-empty range, 0 without one) and, for diff_thres >= 0, qbound_out (the bound image of the
 * range-culled vote for that threshold).  Every output may be NULL. */
int ltm_debug_scan_images(ltm_ctx*, ltm_scanset scans, size_t kf_begin, size_t kf_end, float res_alpha, float diff_thres, float* img_out, float* smax_out,
                          float* qbound_out);
/* The survivor queue word of k_vote_map_cull carries a pixel as a linear index in 18 bits (all ones: pixel not certain); row and column come back from it
 * as row = mulhi(px << 6, magic) >> shift, col = px - row * cols.  For the image shape a fresh context derives from (vfov, hfov, res_alpha):
 *   out_u32[8] = rows, cols, rows * cols, 1 if the shape may take the kernel's fast path (rows * cols <= out_u32[7]), magic, shift, pixel bits (18),
 *                largest rows * cols of the fast path (2^18 - 1)
 * and the row and column the kernel derives from each of px[0 .. n_px) (every px below 2^26, the quotient's domain).  Needs no context and no device. */
int ltm_debug_vote_queue_word(float vfov, float hfov, float res_alpha, uint32_t* out_u32, size_t n_px, const uint32_t* px, uint32_t* out_row, uint32_t* out_col);
/* checks the bounded-error projection that the range-culled vote kernel uses to decide which points need the exact
 * arithmetic: counts points (host xyz, n*3 floats; global frame if inv_pose16 is given, else local) whose exact pixel /
 * range fall outside its candidate set / bounds.  Must be 0. */
int ltm_debug_cull_check(ltm_ctx*, const float* xyz, size_t n, const double* inv_pose16_or_null, float res_alpha, uint64_t* violations);
/* The culled projection kernels (k_vote_map_cull, the pre-filter of k_map_rimg_blockmin: map2RangeImg, utility.cpp:92-142, evaluated exactly only where it can
 * matter) rest on error bounds of a bounded-error projection.  Every range-image shape is validated on the device the first time a context uses it -- 2^20
 * probe points on and beside the pixel-rounding boundaries, in the sensor frame and through one keyframe pose of the call -- and a shape that leaves the
 * bounds is served by the exact kernels from then on (a line on stderr says so).  Counters since ltm_create: shapes checked / shapes that failed. */
int ltm_debug_cull_validation(ltm_ctx*, uint64_t* shapes_checked, uint64_t* shapes_failed);
/* diagnostic counters of the occlusion cull in front of the exact-image kernel on large maps (reprojection, ND votes) since the
 * last reset: (tile, keyframe) pairs seen by culled launches, pairs of the first distance shell, pairs projected in all (the rest was
 * proven hidden and dropped) */
int ltm_debug_occlusion_stats(ltm_ctx*, uint64_t* pairs, uint64_t* first_shell, uint64_t* projected, int reset);
/* voxel grids of clouds since the last reset, and how many of them were recognised as the identity during their bounding-box pass (the
 * input an order-preserving subset of an earlier grid's output, still in octree order and one point per voxel under the frame this
 * call derives: output = copy of the input, bit for bit what the sort + centroid path gives) */
int ltm_debug_voxel_stats(ltm_ctx*, uint64_t* grids, uint64_t* identity_hits, int reset);
/* ltm_reproject_twin since the last reset, stats[8]: calls, calls that projected the shared points once, calls that ran two plain reprojections instead,
 * those plain reprojections, joins whose shared points did not pair up in order (counted among the fallbacks), and the points of map_a, of map_b and of
 * their shared part as the last join saw them */
int ltm_debug_reproject_twin_stats(ltm_ctx*, uint64_t* stats /* 8 */, int reset);
/* ltm_knn_partition's two-phase query (k <= 4, more than 64 target points, LTM_KNN_FAST != 0) since the last reset: scan queries it served,
 * queries its bucket test (phase 1) left undecided for the exact search, calls that took the two-phase path, and calls among them whose
 * cell id + query index did not fit 64 bits so that phase 2 walked its queue in scan order.  All four are counted only in a context created
 * with LTM_KNN_STATS=1 (lanes inherit the switch) and stay 0 otherwise; any pointer may be NULL. */
int ltm_debug_knn_stats(ltm_ctx*, uint64_t* queries, uint64_t* undecided, uint64_t* two_phase_calls, uint64_t* unsorted_queue_calls, int reset);
/* counters of ltm_search_cluster since the last reset, stats[6]: point pairs whose distance was evaluated, pairs found adjacent (edges, each from its higher end;
 * at most one per visited clique leaf), leaves visited by the walks, clique leaves among them (leaves whose box diagonal is below the tolerance by the margin of box_is_clique: united
 * beforehand), walks that left a clique leaf at its first hit, compare-and-swaps of the union-find that failed and were retried.  Always counted; context
 * switch LTM_CLUSTER_CLIQUE=0 (read by ltm_create) turns the clique leaves off -- same results, the counters show which form ran. */
int ltm_debug_cluster_stats(ltm_ctx*, uint64_t* stats /* 6 */, int reset);
/* counters of the plane segmentation since the last reset, stats[4]: point-hypothesis tests (per record its finite points x its valid hypotheses), valid
 * hypotheses, records, records refined.  Counted on the device (the segmentation reads nothing back); this call reads them. */
int ltm_debug_plane_stats(ltm_ctx*, uint64_t* stats /* 4 */, int reset);
/* counters of the outlier filters since the last reset, stats[4]: finite points processed, point pairs whose distance was evaluated, radius walks that
 * refused a node because min_neighbors had been counted, records.  Counted on the device (the filters read nothing back); this call reads them. */
int ltm_debug_outlier_stats(ltm_ctx*, uint64_t* stats /* 4 */, int reset);
/* counters of ltm_search_fpfh since the last reset, stats[4]: finite points processed, point pairs whose distance was evaluated (twice as many where the
 * second pass collects the neighbourhoods again), pairs skipped as degenerate, points that took the LDS list form (k > 16).  Counted on the device; this call reads them. */
int ltm_debug_fpfh_stats(ltm_ctx*, uint64_t* stats /* 4 */, int reset);
/* counters of ltm_sac_align since the last reset, stats[4]: point-hypothesis inlier tests (voting points x valid hypotheses; a target without a finite point has no valid hypothesis and adds none), hypotheses prerejected, walks
 * that ended early at their first hit (the inliers found), records.  Counted on the device; this call reads them. */
int ltm_debug_sac_stats(ltm_ctx*, uint64_t* stats /* 4 */, int reset);
/* which kernel forms a Scan Context shape gets (host arithmetic only, needs no device; the launch wrappers' own expressions): *scatter_in_lds = 1 if
 * ltm_sc_from_scanset pre-reduces a block's points in LDS (up to 4096 bins), 0 if it goes straight to device memory; *pair_in_lds = 1 if the pair
 * distance of ltm_sc_distance / ltm_sc_detect stages both descriptors in LDS (up to 60 KB with the keys and norms), 0 if it reads them from device
 * memory.  Either pointer may be NULL.  LTM_E_INVALID outside 1 <= num_ring <= 64, 1 <= num_sector <= 256. */
int ltm_debug_sc_paths(int num_ring, int num_sector, int* scatter_in_lds, int* pair_in_lds);
/* diagnostic counters of the range-culled vote kernel since the last reset: points tested / points that needed the exact path */
int ltm_debug_cull_stats(ltm_ctx*, uint64_t* survivors, uint64_t* points, int reset);
/* blocks of the context's device pool that are handed out (live) and the bytes they hold: what a caller's handles and open tickets own */
int ltm_debug_pool_live(ltm_ctx*, uint64_t* live_blocks, uint64_t* live_bytes);

/* ----------------------------------------------------------- measurement ---- */
/* Per-kernel-class HIP-event timing on the context's stream.  Classes: "vote_map", "vote_scan",
 * "vote_compare", "reproject_map", "knn_query", "voxel", .... */
int ltm_profile_enable(ltm_ctx*, int on);
int ltm_profile_reset(ltm_ctx*);
/* returns number of classes; fills up to cap entries.  units = class-specific work count
 * (point-projections for vote_map), bytes = algorithmic bytes, ms = sum of event durations */
int ltm_profile_read(ltm_ctx*, const char** names, double* ms, uint64_t* launches, double* units, double* bytes, int cap);
/* same class order as ltm_profile_read: the COMPULSORY bytes of each class's launches as this library issues them -- a projection
 * launch (map2RangeImg for a batch of keyframes, utility.cpp:92-142 under the loops Removerter.cpp:555 / Session.cpp:354) reads its map
 * once for the whole batch, where SURVEY.md 8d's figure counts one map read per keyframe; equal to `bytes` for every other class */
int ltm_profile_read_compulsory(ltm_ctx*, double* bytes_c, int cap);

#ifdef __cplusplus
}
#endif
#endif
