"""ctypes binding of the C ABI in include/ltm.h (libltm_hip.so).

This is plumbing for tests and bench.py: every call goes straight to the HIP library.  There is no
CPU fallback -- if the library is missing or no gfx950 device is usable, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libltm_hip.so")

_lib = None

LTM_OK = 0
ERR_NAMES = {0: "LTM_OK", -1: "LTM_E_INVALID", -2: "LTM_E_DEVICE", -3: "LTM_E_NOMEM", -4: "LTM_E_UNSUPPORTED"}


class LtmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class LtmConfig(C.Structure):
    _fields_ = [("vfov", C.c_float), ("hfov", C.c_float), ("lidar2base", C.c_double * 16),
                ("device", C.c_int), ("max_kf_batch", C.c_int)]


class ScParams(C.Structure):
    """ltm_sc_params (Scancontext.h:84-99)"""
    _fields_ = [("lidar_height", C.c_double), ("num_ring", C.c_int), ("num_sector", C.c_int), ("max_radius", C.c_double),
                ("num_candidates", C.c_int), ("search_ratio", C.c_double), ("dist_thres", C.c_double)]


class ClusterParams(C.Structure):
    """ltm_cluster_params"""
    _fields_ = [("tolerance", C.c_double), ("min_size", C.c_uint32), ("max_size", C.c_uint32)]


class PlaneParams(C.Structure):
    """ltm_plane_params"""
    _fields_ = [("distance_threshold", C.c_double), ("max_iterations", C.c_uint32), ("seed", C.c_uint32), ("axis", C.c_double * 3),
                ("eps_angle", C.c_double), ("refine", C.c_int32)]


class SacParams(C.Structure):
    """ltm_sac_params"""
    _fields_ = [("max_iterations", C.c_uint32), ("seed", C.c_uint32), ("similarity_threshold", C.c_double), ("inlier_distance", C.c_double),
                ("inlier_fraction", C.c_double), ("eval_stride", C.c_uint32)]


class SorParams(C.Structure):
    """ltm_sor_params"""
    _fields_ = [("mean_k", C.c_uint32), ("stddev_mul", C.c_double)]


class RorParams(C.Structure):
    """ltm_ror_params"""
    _fields_ = [("radius", C.c_double), ("min_neighbors", C.c_uint32)]


class IcpParams(C.Structure):
    """ltm_icp_params (LTslam.cpp:207-210)"""
    _fields_ = [("max_corr_dist", C.c_double), ("max_iterations", C.c_int), ("transformation_epsilon", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double)]


# ltm_icp_result as a numpy record (the C layout: 160 bytes)
ICP_RESULT = np.dtype([("T", np.float64, (4, 4)), ("fitness", np.float64), ("last_mse", np.float64), ("converged", np.int32),
                       ("iterations", np.int32), ("state", np.int32), ("n_corr", np.uint32)], align=True)
ICP_STATES = ("too few correspondences", "iterations", "transform", "absolute mse", "relative mse", "degenerate system")
ICP_METHODS = ("point", "plane", "gicp")


class _MethodDefault(int):
    """verify_loops' default for normal_k.  It is the int 10 -- what method="plane" has used since it was added, and what the signature shows -- but its
    identity tells "not given" from an explicit 10, so that method="gicp" can take GICP_NORMAL_K instead"""


GICP_NORMAL_K = 20      # pcl::GeneralizedIterativeClosestPoint's k_correspondences_
_NORMAL_K_OF_METHOD = _MethodDefault(10)


# name -> (restype, argtypes); kept in one table so tests can check it against include/ltm.h
_vp, _sz, _u64, _i, _f = C.c_void_p, C.c_size_t, C.c_uint64, C.c_int, C.c_float
_pu64 = C.POINTER(C.c_uint64)
_psz = C.POINTER(C.c_size_t)
SIGNATURES = {
    "ltm_abi_version": (_i, []),
    "ltm_create": (_i, [C.POINTER(LtmConfig), C.POINTER(_vp)]),
    "ltm_destroy": (None, [_vp]),
    "ltm_last_error": (C.c_char_p, [_vp]),
    "ltm_synchronize": (_i, [_vp]),
    "ltm_clear_caches": (_i, [_vp]),
    "ltm_stream": (_vp, [_vp]),
    "ltm_cloud_upload": (_i, [_vp, _vp, _sz, _sz, _pu64]),
    "ltm_cloud_from_device": (_i, [_vp, _vp, _sz, _pu64]),
    "ltm_cloud_size": (_i, [_vp, _u64, _psz]),
    "ltm_cloud_download": (_i, [_vp, _u64, _vp, _sz, _sz]),
    "ltm_cloud_device_ptr": (_i, [_vp, _u64, C.POINTER(_vp)]),
    "ltm_cloud_clone": (_i, [_vp, _u64, _pu64]),
    "ltm_cloud_concat": (_i, [_vp, _pu64, _sz, _pu64]),
    "ltm_cloud_transform": (_i, [_vp, _u64, _vp, _vp, _pu64]),
    "ltm_cloud_select": (_i, [_vp, _u64, _vp, _sz, _pu64]),
    "ltm_scanset_keyframe": (_i, [_vp, _u64, _sz, _pu64]),
    "ltm_cloud_free": (_i, [_vp, _u64]),
    "ltm_cloud_alloc": (_i, [_vp, _sz, _pu64]),
    "ltm_scanset_alloc": (_i, [_vp, _pu64, _sz, _pu64]),
    "ltm_scanset_upload_begin": (_i, [_vp, _sz, _pu64]),
    "ltm_scanset_upload_chunk": (_i, [_vp, _u64, _vp, _sz, _pu64, _sz]),
    "ltm_scanset_upload_end": (_i, [_vp, _u64, _pu64]),
    "ltm_cloud_fetch_begin": (_i, [_vp, _u64, C.POINTER(_vp)]),
    "ltm_scanset_fetch_begin": (_i, [_vp, _u64, C.POINTER(_vp)]),
    "ltm_fetch_wait": (_i, [_vp, C.POINTER(_vp), _psz, C.POINTER(_pu64), _psz]),
    "ltm_fetch_release": (_i, [_vp, _vp]),
    "ltm_cloud_fetch_chunks_begin": (_i, [_vp, _u64, C.POINTER(_vp)]),
    "ltm_scanset_fetch_chunks_begin": (_i, [_vp, _u64, C.POINTER(_vp)]),
    "ltm_fetch_info": (_i, [_vp, _psz, C.POINTER(_pu64), _psz]),
    "ltm_fetch_next_chunk": (_i, [_vp, C.POINTER(_vp), _psz, _psz, _psz, _psz]),
    "ltm_fetch_chunk_done": (_i, [_vp, _vp]),
    "ltm_buffer_alloc": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "ltm_buffer_free": (_i, [_vp, _vp]),
    "ltm_buffer_fill": (_i, [_vp, _vp, _i, _sz]),
    "ltm_buffer_copy": (_i, [_vp, _vp, _vp, _sz, _i]),
    "ltm_scanset_upload": (_i, [_vp, _vp, _sz, _pu64, _sz, _pu64]),
    "ltm_scanset_from_device": (_i, [_vp, _vp, _pu64, _sz, _pu64]),
    "ltm_scanset_info": (_i, [_vp, _u64, _psz, _psz]),
    "ltm_scanset_offsets": (_i, [_vp, _u64, _pu64]),
    "ltm_scanset_download": (_i, [_vp, _u64, _vp, _sz, _sz]),
    "ltm_scanset_device_ptr": (_i, [_vp, _u64, C.POINTER(_vp)]),
    "ltm_scanset_as_cloud": (_i, [_vp, _u64, _pu64]),
    "ltm_scanset_concat": (_i, [_vp, _pu64, _sz, _pu64]),
    "ltm_scanset_zip_concat": (_i, [_vp, _u64, _u64, _u64, _pu64]),
    "ltm_scanset_free": (_i, [_vp, _u64]),
    "ltm_poses_create": (_i, [_vp, _sz, _vp, _vp, _pu64]),
    "ltm_poses_free": (_i, [_vp, _u64]),
    "ltm_inverse4x4": (_i, [_vp, _vp]),
    "ltm_preclean": (_i, [_vp, _u64, _f, _pu64]),
    "ltm_merge_to_global": (_i, [_vp, _u64, _u64, _pu64]),
    "ltm_voxel_centroid": (_i, [_vp, _u64, _f, _pu64]),
    "ltm_voxel_centroid_shard": (_i, [_vp, _u64, _f, C.c_uint32, C.c_uint32, _pu64]),
    "ltm_voxel_centroid_batch": (_i, [_vp, _sz, _pu64, C.POINTER(_f), _pu64]),
    "ltm_cloud_bbox": (_i, [_vp, _u64, C.POINTER(_f), C.POINTER(_f)]),
    "ltm_voxel_key_histogram": (_i, [_vp, _u64, C.POINTER(_f), C.POINTER(_f), _f, C.POINTER(C.c_uint32)]),
    "ltm_voxel_key_split": (_i, [_vp, _u64, C.POINTER(_f), C.POINTER(_f), _f, C.c_uint32, C.POINTER(C.c_uint32), _pu64]),
    "ltm_voxel_centroid_box": (_i, [_vp, _u64, C.POINTER(_f), C.POINTER(_f), _f, _pu64]),
    "ltm_voxel_centroid_scanset": (_i, [_vp, _u64, _f, _pu64]),
    "ltm_voxel_grid_scanset": (_i, [_vp, _u64, _f, _pu64]),
    "ltm_voxel_grid_scanset_begin": (_i, [_vp, _u64, _f, C.POINTER(_vp)]),
    "ltm_voxel_grid_scanset_end": (_i, [_vp, _vp, _pu64]),
    "ltm_scanset_prepare_range_images": (_i, [_vp, _u64, _sz, _sz, C.POINTER(_f), _sz]),
    "ltm_scanset_prepare_vote_images": (_i, [_vp, _u64, _sz, _sz, C.POINTER(_f), _sz, _f]),
    "ltm_visibility_vote": (_i, [_vp, _u64, _u64, _u64, _sz, _sz, _f, _f, _i, _vp]),
    "ltm_partition_by_labels": (_i, [_vp, _u64, _vp, _pu64, _pu64]),
    "ltm_visibility_partition": (_i, [_vp, _u64, _u64, _u64, _f, _f, _i, _pu64, _pu64, _vp]),
    "ltm_lane_create": (_i, [_vp, C.POINTER(_vp)]),
    "ltm_lane_fence": (_i, [_vp, _vp]),
    "ltm_event_record": (_i, [_vp, C.POINTER(_vp)]),
    "ltm_event_wait": (_i, [_vp, _vp]),
    "ltm_event_destroy": (None, [_vp]),
    "ltm_cloud_lend": (_i, [_vp, _u64, _vp, _pu64]),
    "ltm_cloud_give": (_i, [_vp, _u64, _vp, _pu64]),
    "ltm_scanset_lend": (_i, [_vp, _u64, _vp, _pu64]),
    "ltm_scanset_give": (_i, [_vp, _u64, _vp, _pu64]),
    "ltm_reproject": (_i, [_vp, _u64, _u64, _sz, _sz, _f, _pu64]),
    "ltm_reproject_twin": (_i, [_vp, _u64, _u64, _u64, _sz, _sz, _f, _pu64, _pu64]),
    "ltm_reproject_twin_applicable": (_i, [_vp, _u64, _u64, C.POINTER(_i)]),
    "ltm_debug_reproject_twin_stats": (_i, [_vp, _pu64, _i]),
    "ltm_knn_partition": (_i, [_vp, _u64, _u64, _u64, _sz, _sz, _i, _f, _pu64, _pu64]),
    "ltm_knn_split_cloud": (_i, [_vp, _u64, _u64, _i, _f, _pu64, _pu64]),
    "ltm_search_build": (_i, [_vp, _u64, C.POINTER(_vp)]),
    "ltm_search_free": (_i, [_vp, _vp]),
    "ltm_search_info": (_i, [_vp, _vp, _psz, _psz]),
    "ltm_knn_search": (_i, [_vp, _vp, _u64, _i, _vp, _vp]),
    "ltm_radius_search": (_i, [_vp, _vp, _u64, _f, _i, C.POINTER(_vp)]),
    "ltm_search_result_info": (_i, [_vp, _vp, _psz, _psz, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "ltm_search_result_free": (_i, [_vp, _vp]),
    "ltm_search_estimate_normals": (_i, [_vp, _sz, C.POINTER(_vp), _i, _vp]),
    "ltm_search_normals_info": (_i, [_vp, _vp, C.POINTER(_i), C.POINTER(_vp)]),
    "ltm_search_normals_download": (_i, [_vp, _vp, _vp]),
    "ltm_sc_default_params": (None, [C.POINTER(ScParams)]),
    "ltm_sc_from_scanset": (_i, [_vp, _u64, _sz, _sz, C.POINTER(ScParams), C.POINTER(_vp)]),
    "ltm_sc_from_descriptors": (_i, [_vp, _vp, _sz, C.POINTER(ScParams), C.POINTER(_vp)]),
    "ltm_sc_info": (_i, [_vp, _vp, _psz, C.POINTER(_i), C.POINTER(_i)]),
    "ltm_sc_download": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "ltm_sc_distance": (_i, [_vp, _vp, _vp, _vp, _sz, C.POINTER(ScParams), _vp, _vp]),
    "ltm_sc_detect": (_i, [_vp, _vp, _vp, C.POINTER(ScParams), _vp, _vp, _vp, _vp, _vp]),
    "ltm_sc_free": (_i, [_vp, _vp]),
    "ltm_icp_default_params": (None, [C.POINTER(IcpParams)]),
    "ltm_icp_align": (_i, [_vp, _sz, C.POINTER(_vp), _pu64, _vp, C.POINTER(IcpParams), _vp, _vp]),
    "ltm_icp_align_scanset": (_i, [_vp, _sz, C.POINTER(_vp), _u64, _vp, _vp, C.POINTER(IcpParams), _vp, _vp]),
    "ltm_icp_align_plane": (_i, [_vp, _sz, C.POINTER(_vp), _pu64, _vp, C.POINTER(IcpParams), _vp, _vp]),
    "ltm_icp_align_plane_scanset": (_i, [_vp, _sz, C.POINTER(_vp), _u64, _vp, _vp, C.POINTER(IcpParams), _vp, _vp]),
    "ltm_icp_align_gicp": (_i, [_vp, _sz, C.POINTER(_vp), C.POINTER(_vp), _vp, C.POINTER(IcpParams), C.c_double, _vp, _vp]),
    "ltm_pose6d_to_affine3f": (_i, [_vp, _sz, _vp]),
    "ltm_submaps_assemble": (_i, [_vp, _u64, _vp, _vp, _sz, _i, _f, _i, _pu64]),
    "ltm_search_build_scanset": (_i, [_vp, _u64, _sz, _sz, C.POINTER(_vp)]),
    "ltm_cluster_default_params": (None, [C.POINTER(ClusterParams)]),
    "ltm_search_cluster": (_i, [_vp, _sz, C.POINTER(_vp), C.POINTER(ClusterParams), C.POINTER(_vp)]),
    "ltm_clusters_info": (_i, [_vp, _vp, _psz, _psz, _psz]),
    "ltm_clusters_device": (_i, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "ltm_clusters_download": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ltm_clusters_extract": (_i, [_vp, _vp, _u64, _pu64]),
    "ltm_clusters_free": (_i, [_vp, _vp]),
    "ltm_debug_cluster_stats": (_i, [_vp, _pu64, _i]),
    "ltm_plane_default_params": (None, [C.POINTER(PlaneParams)]),
    "ltm_plane_block_points": (C.c_uint32, []),
    "ltm_scanset_segment_planes": (_i, [_vp, _u64, _sz, _sz, C.POINTER(PlaneParams), C.POINTER(_vp)]),
    "ltm_cloud_segment_plane": (_i, [_vp, _u64, C.POINTER(PlaneParams), C.POINTER(_vp)]),
    "ltm_planes_info": (_i, [_vp, _vp, _psz, _psz, C.POINTER(C.c_uint32)]),
    "ltm_planes_device": (_i, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "ltm_planes_download": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ltm_planes_split_scanset": (_i, [_vp, _vp, _u64, _pu64, _pu64]),
    "ltm_planes_split_cloud": (_i, [_vp, _vp, _u64, _pu64, _pu64]),
    "ltm_planes_free": (_i, [_vp, _vp]),
    "ltm_debug_plane_stats": (_i, [_vp, _pu64, _i]),
    "ltm_sor_default_params": (None, [C.POINTER(SorParams)]),
    "ltm_ror_default_params": (None, [C.POINTER(RorParams)]),
    "ltm_search_filter_statistical": (_i, [_vp, _sz, C.POINTER(_vp), C.POINTER(SorParams), C.POINTER(_vp)]),
    "ltm_search_filter_radius": (_i, [_vp, _sz, C.POINTER(_vp), C.POINTER(RorParams), C.POINTER(_vp)]),
    "ltm_outliers_info": (_i, [_vp, _vp, C.POINTER(_i), _psz, _psz]),
    "ltm_outliers_device": (_i, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "ltm_outliers_download": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ltm_outliers_split_scanset": (_i, [_vp, _vp, _u64, _pu64, _pu64]),
    "ltm_outliers_split_cloud": (_i, [_vp, _vp, _u64, _pu64, _pu64]),
    "ltm_outliers_free": (_i, [_vp, _vp]),
    "ltm_debug_outlier_stats": (_i, [_vp, _pu64, _i]),
    "ltm_search_fpfh": (_i, [_vp, _sz, C.POINTER(_vp), _i, C.POINTER(_vp)]),
    "ltm_fpfh_info": (_i, [_vp, _vp, _psz, _psz, C.POINTER(_i)]),
    "ltm_fpfh_device": (_i, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "ltm_fpfh_download": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "ltm_fpfh_free": (_i, [_vp, _vp]),
    "ltm_debug_fpfh_stats": (_i, [_vp, _pu64, _i]),
    "ltm_fpfh_upload": (_i, [_vp, _sz, _vp, _vp, C.POINTER(_vp)]),
    "ltm_match_tile_rows": (C.c_uint32, []),
    "ltm_fpfh_match": (_i, [_vp, _sz, _vp, _vp, _vp, _vp, _i, C.POINTER(_vp)]),
    "ltm_matches_info": (_i, [_vp, _vp, _psz, _psz, C.POINTER(_i)]),
    "ltm_matches_device": (_i, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "ltm_matches_download": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "ltm_matches_free": (_i, [_vp, _vp]),
    "ltm_sac_default_params": (None, [C.POINTER(SacParams)]),
    "ltm_sac_block_points": (C.c_uint32, []),
    "ltm_sac_align": (_i, [_vp, _sz, C.POINTER(_vp), C.POINTER(_vp), _vp, C.POINTER(SacParams), C.POINTER(_vp)]),
    "ltm_sac_info": (_i, [_vp, _vp, _psz, C.POINTER(C.c_uint32)]),
    "ltm_sac_device": (_i, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "ltm_sac_download": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ltm_sac_free": (_i, [_vp, _vp]),
    "ltm_debug_sac_stats": (_i, [_vp, _pu64, _i]),
    "ltm_debug_pool_live": (_i, [_vp, _pu64, _pu64]),
    "ltm_debug_range_image": (_i, [_vp, _u64, _vp, _vp, _f, _vp, _vp]),
    "ltm_debug_viz_images": (_i, [_vp, _u64, _u64, _u64, _sz, _f, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "ltm_debug_project": (_i, [_vp, _vp, _sz, _f, _vp, _vp]),
    "ltm_debug_elevation_fit": (_i, [_f, C.POINTER(_f), C.POINTER(C.c_double)]),
    "ltm_debug_pcl_sort_order": (_i, [C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32), _i, C.POINTER(C.c_uint32)]),
    "ltm_debug_voxel_key_bits": (_i, [C.POINTER(_f), C.POINTER(_f), _f, _pu64, C.POINTER(C.c_uint), C.POINTER(C.c_double)]),
    "ltm_debug_selfcheck": (_i, [_vp, _pu64, C.POINTER(_i)]),
    "ltm_debug_cull_check": (_i, [_vp, _vp, _sz, _vp, _f, _pu64]),
    "ltm_debug_cull_stats": (_i, [_vp, _pu64, _pu64, _i]),
    "ltm_debug_proj_launch": (_i, [_f, _f, _f, _vp, _sz, _sz, _i, _vp, _vp, C.c_uint32, _sz, _vp, _vp]),
    "ltm_debug_vote_run_launch": (_i, [_sz, _sz, _i, C.c_uint32, _sz, _vp, _vp, _vp, _vp]),
    "ltm_debug_vote_queue_word": (_i, [C.c_float, C.c_float, C.c_float, _vp, _sz, _vp, _vp, _vp]),
    "ltm_debug_scan_bands": (_i, [_sz, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "ltm_debug_scan_images": (_i, [_vp, _u64, _sz, _sz, _f, _f, _vp, _vp, _vp]),
    "ltm_debug_cull_validation": (_i, [_vp, _pu64, _pu64]),
    "ltm_debug_occlusion_stats": (_i, [_vp, _pu64, _pu64, _pu64, _i]),
    "ltm_debug_voxel_stats": (_i, [_vp, _pu64, _pu64, _i]),
    "ltm_debug_knn_stats": (_i, [_vp, _pu64, _pu64, _pu64, _pu64, _i]),
    "ltm_debug_sc_paths": (_i, [_i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "ltm_rimg_size": (None, [_f, _f, _f, C.POINTER(_i), C.POINTER(_i)]),
    "ltm_profile_enable": (_i, [_vp, _i]),
    "ltm_profile_reset": (_i, [_vp]),
    "ltm_profile_read_compulsory": (_i, [_vp, C.POINTER(C.c_double), _i]),
    "ltm_profile_read": (_i, [_vp, C.POINTER(C.c_char_p), C.POINTER(C.c_double), _pu64, C.POINTER(C.c_double),
                              C.POINTER(C.c_double), _i]),
}


def load_library(path=None):
    """Load libltm_hip.so and declare every entry point.  Raises if the library is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    # Load order of the HIP runtime: torch ships its own libamdhip64 and this library links the system one (same soname).  Whichever is
    # mapped first serves both; if OURS comes first and torch is imported later in the same process (build() followed by smoke()),
    # torch initialises against a runtime it was not built with and ltm_create then finds no usable device.  Importing torch first --
    # the order bench.py and the tests always had -- keeps one consistent runtime.  Without torch installed nothing changes.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} not found: build it with `make hip` (or __graft_entry__.build()). There is no CPU fallback.")
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def voxel_key_bits(mn, mx, leaf):
    """ltm_debug_voxel_key_bits: (kept bit count, kept mask, octree depth, lattice origin) of the voxel grid's sort key"""
    a = (_f * 3)(*[float(v) for v in mn]); b = (_f * 3)(*[float(v) for v in mx])
    mask, depth, fmin = _u64(), C.c_uint(), (C.c_double * 3)()
    n = load_library().ltm_debug_voxel_key_bits(a, b, float(leaf), C.byref(mask), C.byref(depth), fmin)
    if n < 0:
        raise ValueError("unsupported box / leaf")
    return n, mask.value, depth.value, np.array(list(fmin))


PROJ_LAUNCH_F32 = ("half_v", "half_h", "inv_v", "inv_h", "frows", "fcols", "row_max", "col_max", "row_scale", "col_scale", "row_bias", "col_bias",
                   "certain_lim", "rmin2", "eps", "el_tclamp")
PROJ_LAUNCH_U32 = ("rows", "cols", "npx", "steep_clamps", "packable", "n_tiles", "n_tg", "tg_magic", "tg_shift", "grid", "el_fit", "fast")


def proj_launch(vfov, hfov, alpha, base2lidar=None, map_points=0, n_keyframes=1, on_device=False, first_block=0, n_blocks=0):
    """ltm_debug_proj_launch: ({name: float32}, {name: int}, tile[n_blocks], keyframe[n_blocks]) -- the launch constants of the projection kernels
    and the (tile, keyframe) of a run of workgroups (0xffffffff: idle).  Needs no context; on_device evaluates the constants with one device thread."""
    f = np.zeros(len(PROJ_LAUNCH_F32), dtype=np.float32)
    u = np.zeros(len(PROJ_LAUNCH_U32), dtype=np.uint32)
    tile = np.zeros(max(n_blocks, 1), dtype=np.uint32)
    kf = np.zeros(max(n_blocks, 1), dtype=np.uint32)
    b2l = None if base2lidar is None else _mat16(base2lidar)
    rc = load_library().ltm_debug_proj_launch(float(vfov), float(hfov), float(alpha), None if b2l is None else b2l.ctypes.data, int(map_points),
                                              int(n_keyframes), int(bool(on_device)), f.ctypes.data, u.ctypes.data, int(first_block), int(n_blocks),
                                              tile.ctypes.data, kf.ctypes.data)
    if rc != 0:
        raise LtmError(rc, "ltm_debug_proj_launch")
    return dict(zip(PROJ_LAUNCH_F32, f)), {k: int(v) for k, v in zip(PROJ_LAUNCH_U32, u)}, tile[:n_blocks], kf[:n_blocks]


def vote_run_launch(map_points, n_keyframes, tile_run, first_block=0, n_blocks=0):
    """ltm_debug_vote_run_launch: (run[n_blocks], keyframe[n_blocks], run length, grid size) -- which run of `tile_run` consecutive map tiles and which
    keyframe each workgroup of a range-culled vote launch works on (0xffffffff: idle).  Needs no context and no device."""
    run = np.zeros(max(n_blocks, 1), dtype=np.uint32)
    kf = np.zeros(max(n_blocks, 1), dtype=np.uint32)
    run_len, grid = C.c_uint32(0), C.c_uint32(0)
    rc = load_library().ltm_debug_vote_run_launch(int(map_points), int(n_keyframes), int(tile_run), int(first_block), int(n_blocks), run.ctypes.data,
                                                  kf.ctypes.data, C.byref(run_len), C.byref(grid))
    if rc != 0:
        raise LtmError(rc, "ltm_debug_vote_run_launch")
    return run[:n_blocks], kf[:n_blocks], run_len.value, grid.value


def scan_bands(rows, cols):
    """ltm_debug_scan_bands: (n_bands, row0[n_bands + 1, n_shapes], bytes[n_bands], budget) -- the band plan of the LDS scan-image kernel for the image
    shapes rows[j] x cols[j]: band b holds rows [row0[b, j], row0[b + 1, j]) of shape j.  n_bands == 0: the set is not served (the older kernels take it).
    Needs no context and no device."""
    r = np.ascontiguousarray(rows, dtype=np.int32)
    c = np.ascontiguousarray(cols, dtype=np.int32)
    assert r.shape == c.shape and r.ndim == 1
    lib = load_library()
    n_bands, budget = C.c_uint32(0), C.c_uint32(0)
    rc = lib.ltm_debug_scan_bands(len(r), r.ctypes.data if len(r) else None, c.ctypes.data if len(r) else None, C.byref(n_bands), C.byref(budget), 0, None, None)
    if rc != 0:
        raise LtmError(rc, "ltm_debug_scan_bands")
    nb = n_bands.value
    row0 = np.zeros((nb + 1, max(len(r), 1)), dtype=np.uint32)
    nbytes = np.zeros(max(nb, 1), dtype=np.uint32)
    if nb:
        rc = lib.ltm_debug_scan_bands(len(r), r.ctypes.data, c.ctypes.data, C.byref(n_bands), C.byref(budget), nb, row0.ctypes.data, nbytes.ctypes.data)
        if rc != 0:
            raise LtmError(rc, "ltm_debug_scan_bands")
    return nb, row0[:, :len(r)], nbytes[:nb], budget.value


VOTE_QUEUE_WORD_U32 = ("rows", "cols", "npx", "fast_path", "px_magic", "px_shift", "px_bits", "npx_limit")


def vote_queue_word(vfov, hfov, alpha, px=None):
    """ltm_debug_vote_queue_word: ({name: int}, row[n], col[n]) -- the pixel field of the range-culled vote kernel's survivor queue word for the image
    shape of (vfov, hfov, alpha), and the row and column the kernel derives from the pixel indices `px`.  Needs no context and no device."""
    u = np.zeros(len(VOTE_QUEUE_WORD_U32), dtype=np.uint32)
    p = np.ascontiguousarray(np.zeros(0) if px is None else px, dtype=np.uint32)
    row = np.zeros(max(len(p), 1), dtype=np.uint32)
    col = np.zeros(max(len(p), 1), dtype=np.uint32)
    rc = load_library().ltm_debug_vote_queue_word(float(vfov), float(hfov), float(alpha), u.ctypes.data, len(p), p.ctypes.data if len(p) else None,
                                                  row.ctypes.data, col.ctypes.data)
    if rc != 0:
        raise LtmError(rc, "ltm_debug_vote_queue_word")
    return {k: int(v) for k, v in zip(VOTE_QUEUE_WORD_U32, u)}, row[:len(p)], col[:len(p)]


def inverse4x4(m):
    """ltm_inverse4x4: the library's Eigen::Matrix4d::inverse() restatement (needs no device)"""
    a = np.ascontiguousarray(m, dtype=np.float64).reshape(16)
    out = np.empty(16, dtype=np.float64)
    if load_library().ltm_inverse4x4(a.ctypes.data, out.ctypes.data) != 0:
        raise ValueError("singular or non-finite matrix")
    return out.reshape(4, 4)


def pose6d_to_affine3f(xyzrpy):
    """ltm_pose6d_to_affine3f: (n, 6) poses x y z roll pitch yaw -> (n, 3, 4) float32 affines, pcl::getTransformation in float (needs no device)"""
    a = np.ascontiguousarray(xyzrpy, dtype=np.float32).reshape(-1, 6)
    out = np.empty((a.shape[0], 3, 4), dtype=np.float32)
    if a.shape[0] and load_library().ltm_pose6d_to_affine3f(a.ctypes.data, a.shape[0], out.ctypes.data) != 0:
        raise ValueError("ltm_pose6d_to_affine3f failed")
    return out


ORDERS = {"input": 0, "pcl": 1}


def _np_pts(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        a = a.reshape(-1, 4)
    return a


def _mat16(m):
    m = np.ascontiguousarray(m, dtype=np.float64).reshape(-1)
    assert m.size == 16
    return m


class Context:
    """One ltm_ctx: one GPU, one HIP stream, all device memory behind handles."""

    def __init__(self, vfov=50.0, hfov=360.0, lidar2base=None, device=0, max_kf_batch=0):
        self.lib = load_library()
        cfg = LtmConfig()
        cfg.vfov, cfg.hfov, cfg.device, cfg.max_kf_batch = vfov, hfov, device, max_kf_batch
        l2b = _mat16(np.eye(4) if lidar2base is None else lidar2base)
        for i in range(16):
            cfg.lidar2base[i] = l2b[i]
        self.vfov, self.hfov, self.device = float(vfov), float(hfov), int(device)
        h = _vp()
        rc = self.lib.ltm_create(C.byref(cfg), C.byref(h))
        if rc != LTM_OK:
            raise LtmError(rc, "ltm_create failed (no usable gfx950 device?)")
        self.h = h

    def lane(self):
        """ltm_lane_create: a second context on this one's device (own stream, own pool, same configuration) for a second host thread; clouds and
        scan sets pass between the two without copies (lend / give)"""
        other = Context.__new__(Context)
        other.lib, other.vfov, other.hfov, other.device = self.lib, self.vfov, self.hfov, self.device
        h = _vp()
        rc = self.lib.ltm_lane_create(self.h, C.byref(h))
        if rc != LTM_OK:
            raise LtmError(rc, "ltm_lane_create failed")
        other.h = h
        return other

    def _pass(self, obj, to, give):
        kind = "cloud" if isinstance(obj, Cloud) else "scanset"
        out = _u64()
        self._ck(getattr(self.lib, f"ltm_{kind}_{'give' if give else 'lend'}")(self.h, obj.h, to.h, C.byref(out)))
        new = (Cloud if kind == "cloud" else ScanSet)(to, out.value)
        if give:
            obj.h = 0
        else:
            new._lender = obj      # keeps the owner's Python handle (and so the memory) alive as long as the view exists
        return new

    def lend(self, obj, to):
        """a borrowed view of `obj` (Cloud or ScanSet of this context) in context `to`, no copy; this context keeps ownership"""
        return self._pass(obj, to, False)

    def give(self, obj, to):
        """moves `obj` into context `to` (no copy); `obj` is invalid afterwards"""
        return self._pass(obj, to, True)

    def fence(self, before_next_of):
        """what is submitted to `before_next_of` from now on runs after everything submitted to this context so far"""
        self._ck(self.lib.ltm_lane_fence(self.h, before_next_of.h))

    def event_record(self):
        ev = _vp()
        self._ck(self.lib.ltm_event_record(self.h, C.byref(ev)))
        return Event(self.lib, ev)

    def event_wait(self, ev):
        self._ck(self.lib.ltm_event_wait(self.h, ev.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.ltm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != LTM_OK:
            raise LtmError(rc, self.lib.ltm_last_error(self.h).decode())

    # ---- clouds
    def upload(self, pts):
        a = _np_pts(pts)
        out = _u64()
        self._ck(self.lib.ltm_cloud_upload(self.h, a.ctypes.data, a.shape[0], 16, C.byref(out)))
        return Cloud(self, out.value)

    def cloud_from_device(self, dev_ptr, n):
        out = _u64()
        self._ck(self.lib.ltm_cloud_from_device(self.h, dev_ptr, n, C.byref(out)))
        return Cloud(self, out.value)

    def transform(self, cloud, T1=None, T2=None):
        """pcl::transformPointCloud once or twice (row-major 4x4 doubles)"""
        t1 = None if T1 is None else np.ascontiguousarray(T1, dtype=np.float64).reshape(16)
        t2 = None if T2 is None else np.ascontiguousarray(T2, dtype=np.float64).reshape(16)
        out = _u64()
        self._ck(self.lib.ltm_cloud_transform(self.h, cloud.h, None if t1 is None else t1.ctypes.data, None if t2 is None else t2.ctypes.data, C.byref(out)))
        return Cloud(self, out.value)

    def select(self, cloud, idx):
        """pcl::ExtractIndices (parsePointcloudSubsetUsingPtIdx, Removerter.cpp:933-946): out[j] = cloud[idx[j]]"""
        a = np.ascontiguousarray(idx, dtype=np.int32)
        out = _u64()
        self._ck(self.lib.ltm_cloud_select(self.h, cloud.h, a.ctypes.data, a.size, C.byref(out)))
        return Cloud(self, out.value)

    def scan_of_keyframe(self, scans, kf):
        out = _u64()
        self._ck(self.lib.ltm_scanset_keyframe(self.h, scans.h, kf, C.byref(out)))
        return Cloud(self, out.value)

    def concat(self, clouds):
        arr = (_u64 * len(clouds))(*[c.h for c in clouds])
        out = _u64()
        self._ck(self.lib.ltm_cloud_concat(self.h, arr, len(clouds), C.byref(out)))
        return Cloud(self, out.value)

    # ---- scan sets
    def upload_scans(self, pts, offsets):
        a = _np_pts(pts)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        out = _u64()
        self._ck(self.lib.ltm_scanset_upload(self.h, a.ctypes.data, 16, off.ctypes.data_as(_pu64), off.size - 1, C.byref(out)))
        return ScanSet(self, out.value)

    def scans_from_device(self, dev_ptr, offsets):
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        out = _u64()
        self._ck(self.lib.ltm_scanset_from_device(self.h, dev_ptr, off.ctypes.data_as(_pu64), off.size - 1, C.byref(out)))
        return ScanSet(self, out.value)

    def concat_scansets(self, sets):
        arr = (_u64 * len(sets))(*[s.h for s in sets])
        out = _u64()
        self._ck(self.lib.ltm_scanset_concat(self.h, arr, len(sets), C.byref(out)))
        return ScanSet(self, out.value)

    def zip_concat(self, a, b, c=None):
        out = _u64()
        self._ck(self.lib.ltm_scanset_zip_concat(self.h, a.h, b.h, c.h if c is not None else 0, C.byref(out)))
        return ScanSet(self, out.value)

    # ---- poses
    def poses(self, poses, inv=None):
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)
        iv = None if inv is None else np.ascontiguousarray(inv, dtype=np.float64).reshape(-1, 16)
        out = _u64()
        self._ck(self.lib.ltm_poses_create(self.h, p.shape[0], p.ctypes.data, None if iv is None else iv.ctypes.data, C.byref(out)))
        if iv is None:      # the host copy holds what the library computed for itself (ltm_inverse4x4)
            iv = np.stack([inverse4x4(m).reshape(16) for m in p]) if p.shape[0] else p.copy()
        return Poses(self, out.value, p.shape[0], p.copy(), iv.copy())

    # ---- stages
    def preclean(self, scans, radius):
        out = _u64()
        self._ck(self.lib.ltm_preclean(self.h, scans.h, radius, C.byref(out)))
        return ScanSet(self, out.value)

    def merge_to_global(self, scans, poses):
        out = _u64()
        self._ck(self.lib.ltm_merge_to_global(self.h, scans.h, poses.h, C.byref(out)))
        return Cloud(self, out.value)

    def voxel_centroid(self, cloud, leaf):
        out = _u64()
        self._ck(self.lib.ltm_voxel_centroid(self.h, cloud.h, leaf, C.byref(out)))
        return Cloud(self, out.value)

    def voxel_centroid_batch(self, clouds, leafs):
        n = len(clouds)
        ins = (_u64 * n)(*[c.h for c in clouds])
        lf = (_f * n)(*[float(x) for x in leafs])
        outs = (_u64 * n)()
        self._ck(self.lib.ltm_voxel_centroid_batch(self.h, n, ins, lf, outs))
        return [Cloud(self, outs[k]) for k in range(n)]

    # ---- key-range exchange (include/ltm.h: ltm_cloud_bbox ... ltm_voxel_centroid_box)
    @staticmethod
    def _f3(v):
        return (_f * 3)(*[float(x) for x in v])

    def bbox(self, cloud):
        mn, mx = (_f * 3)(), (_f * 3)()
        self._ck(self.lib.ltm_cloud_bbox(self.h, cloud.h, mn, mx))
        return np.array(mn[:], np.float32), np.array(mx[:], np.float32)

    def voxel_key_histogram(self, cloud, mn, mx, leaf):
        hist = (C.c_uint32 * 4096)()
        self._ck(self.lib.ltm_voxel_key_histogram(self.h, cloud.h, self._f3(mn), self._f3(mx), leaf, hist))
        return np.frombuffer(hist, dtype=np.uint32).copy()

    def voxel_key_split(self, cloud, mn, mx, leaf, cuts):
        n = len(cuts) - 1
        cb = (C.c_uint32 * (n + 1))(*[int(x) for x in cuts])
        outs = (_u64 * n)()
        self._ck(self.lib.ltm_voxel_key_split(self.h, cloud.h, self._f3(mn), self._f3(mx), leaf, n, cb, outs))
        return [Cloud(self, outs[k]) for k in range(n)]

    def voxel_centroid_box(self, cloud, mn, mx, leaf):
        out = _u64()
        self._ck(self.lib.ltm_voxel_centroid_box(self.h, cloud.h, self._f3(mn), self._f3(mx), leaf, C.byref(out)))
        return Cloud(self, out.value)

    def voxel_centroid_shard(self, cloud, leaf, shard, n_shards):
        out = _u64()
        self._ck(self.lib.ltm_voxel_centroid_shard(self.h, cloud.h, leaf, shard, n_shards, C.byref(out)))
        return Cloud(self, out.value)

    def viz_images(self, cmap, scans, poses, kf, alpha, mode=0, range_axis=(0.0, 10.0), diff_axis=(0.0, 0.5)):
        """the four RViz images of keyframe `kf` (Removerter.cpp:580-585) as (rows, cols, 3) BGR8 arrays"""
        rows, cols = self.rimg_size(alpha)
        out = {k: np.empty((rows, cols, 3), dtype=np.uint8) for k in ("scan", "map", "diff", "ptidx")}
        self._ck(self.lib.ltm_debug_viz_images(self.h, cmap.h, scans.h, poses.h, kf, alpha, mode, range_axis[0], range_axis[1],
                                               diff_axis[0], diff_axis[1], out["scan"].ctypes.data, out["map"].ctypes.data,
                                               out["diff"].ctypes.data, out["ptidx"].ctypes.data))
        return out

    def voxel_centroid_scanset(self, scans, leaf):
        out = _u64()
        self._ck(self.lib.ltm_voxel_centroid_scanset(self.h, scans.h, leaf, C.byref(out)))
        return ScanSet(self, out.value)

    def voxel_grid_scanset(self, scans, leaf):
        out = _u64()
        self._ck(self.lib.ltm_voxel_grid_scanset(self.h, scans.h, leaf, C.byref(out)))
        return ScanSet(self, out.value)

    def voxel_grid_scanset_begin(self, scans, leaf):
        """first half of voxel_grid_scanset: returns a ticket at once (keys on their way to the host threads); `scans` must stay alive until
        voxel_grid_scanset_end(ticket).  Work submitted in between runs beside the transfer and the host sort."""
        t = C.c_void_p()
        self._ck(self.lib.ltm_voxel_grid_scanset_begin(self.h, scans.h, leaf, C.byref(t)))
        return VgsTicket(self, t, scans)

    def voxel_grid_scanset_end(self, ticket):
        return ticket.end()

    def prepare_scan_images(self, scans, alphas, kf_begin=0, kf_end=None):
        """scan range images of all the listed resolutions in one pass over the scans (kept for the votes that follow)"""
        a = (_f * len(alphas))(*[float(x) for x in alphas])
        self._ck(self.lib.ltm_scanset_prepare_range_images(self.h, scans.h, kf_begin, scans.n_kf if kf_end is None else kf_end, a, len(alphas)))

    def prepare_vote_images(self, scans, alphas, thr, kf_begin=0, kf_end=None):
        """prepare_scan_images plus the threshold of the votes that follow: their bound images come out of the same pass (thr < 0: none)"""
        a = (_f * len(alphas))(*[float(x) for x in alphas])
        self._ck(self.lib.ltm_scanset_prepare_vote_images(self.h, scans.h, kf_begin, scans.n_kf if kf_end is None else kf_end, a, len(alphas), float(thr)))

    def debug_scan_images(self, scans, alpha, thr=-1.0, kf_begin=0, kf_end=None, want_qbound=None):
        """ltm_debug_scan_images: (img[n_kf, rows, cols] f32, smax[n_kf] f32, qbound[n_kf, rows, cols] f32 or None) -- the scan range images of one resolution
        as the votes see them (cached or built now); the bound image for thr >= 0."""
        ke = scans.n_kf if kf_end is None else kf_end
        rows, cols = self.rimg_size(alpha)
        n = ke - kf_begin
        img = np.zeros((n, rows, cols), dtype=np.float32)
        smax = np.zeros(n, dtype=np.float32)
        want_q = (thr >= 0) if want_qbound is None else want_qbound
        qb = np.zeros((n, rows, cols), dtype=np.float32) if want_q else None
        self._ck(self.lib.ltm_debug_scan_images(self.h, scans.h, kf_begin, ke, float(alpha), float(thr), img.ctypes.data, smax.ctypes.data,
                                                qb.ctypes.data if want_q else None))
        return img, smax, qb

    def visibility_vote(self, cmap, scans, poses, kf_begin, kf_end, alpha, thr, mode, labels_dev_ptr):
        self._ck(self.lib.ltm_visibility_vote(self.h, cmap.h, scans.h, poses.h, kf_begin, kf_end, alpha, thr, mode, labels_dev_ptr))

    def partition_by_labels(self, cmap, labels_dev_ptr):
        k, f = _u64(), _u64()
        self._ck(self.lib.ltm_partition_by_labels(self.h, cmap.h, labels_dev_ptr, C.byref(k), C.byref(f)))
        return Cloud(self, k.value), Cloud(self, f.value)

    def visibility_partition(self, cmap, scans, poses, alpha, thr=0.1, mode=0, want_labels=False):
        k, f = _u64(), _u64()
        labels = np.zeros(len(cmap), dtype=np.uint8) if want_labels else None
        self._ck(self.lib.ltm_visibility_partition(self.h, cmap.h, scans.h, poses.h, alpha, thr, mode, C.byref(k), C.byref(f),
                                                   labels.ctypes.data if want_labels else None))
        kept, flagged = Cloud(self, k.value), Cloud(self, f.value)
        return (kept, flagged, labels) if want_labels else (kept, flagged)

    def reproject(self, cmap, poses, alpha=3.0, kf_begin=0, kf_end=None):
        out = _u64()
        self._ck(self.lib.ltm_reproject(self.h, cmap.h, poses.h, kf_begin, poses.n if kf_end is None else kf_end, alpha, C.byref(out)))
        return ScanSet(self, out.value)

    def reproject_twin(self, cmap_a, cmap_b, poses, alpha=3.0, kf_begin=0, kf_end=None):
        """ltm_reproject_twin: (reproject(cmap_a), reproject(cmap_b)), the points that two grids of one frame share projected once"""
        a, b = _u64(), _u64()
        self._ck(self.lib.ltm_reproject_twin(self.h, cmap_a.h, cmap_b.h, poses.h, kf_begin, poses.n if kf_end is None else kf_end, alpha,
                                             C.byref(a), C.byref(b)))
        return ScanSet(self, a.value), ScanSet(self, b.value)

    def reproject_twin_applicable(self, cmap_a, cmap_b):
        """ltm_reproject_twin_applicable: True when reproject_twin would look for shared points (two grids of one frame), known without touching the device"""
        yes = _i()
        self._ck(self.lib.ltm_reproject_twin_applicable(self.h, cmap_a.h, cmap_b.h, C.byref(yes)))
        return bool(yes.value)

    def reproject_twin_stats(self, reset=False):
        """ltm_debug_reproject_twin_stats as a dict: calls, hits (shared points projected once), fallbacks (two plain reprojections), plain_passes,
        unordered (joins whose shared points did not pair up in order), and last_a / last_b / last_shared, the sizes the last join saw"""
        v = (_u64 * 8)()
        self._ck(self.lib.ltm_debug_reproject_twin_stats(self.h, v, 1 if reset else 0))
        names = ("calls", "hits", "fallbacks", "plain_passes", "unordered", "last_a", "last_b", "last_shared")
        return {k: int(x) for k, x in zip(names, v)}

    def knn_partition(self, target, scans, poses, k, thr, kf_begin=0, kf_end=None):
        co, di = _u64(), _u64()
        self._ck(self.lib.ltm_knn_partition(self.h, target.h, scans.h, poses.h, kf_begin, poses.n if kf_end is None else kf_end,
                                            k, thr, C.byref(co), C.byref(di)))
        return ScanSet(self, co.value), ScanSet(self, di.value)

    def knn_split_cloud(self, target, query, k, thr):
        near, far = _u64(), _u64()
        self._ck(self.lib.ltm_knn_split_cloud(self.h, target.h, query.h, k, thr, C.byref(near), C.byref(far)))
        return Cloud(self, near.value), Cloud(self, far.value)

    def search_index(self, cloud):
        """ltm_search_build: exact k-NN / radius search index over `cloud` (a Cloud of this context or an (n, 4) / (n, 3) array), the
        counterpart of pcl::KdTreeFLANN::setInputCloud"""
        if not isinstance(cloud, Cloud):
            cloud = self.upload(_xyzi(cloud))
        h = _vp()
        self._ck(self.lib.ltm_search_build(self.h, cloud.h, C.byref(h)))
        return SearchIndex(self, h.value)

    def search_index_batch(self, scanset, kf_begin=0, kf_end=None):
        """ltm_search_build_scanset: one SearchIndex per keyframe [kf_begin, kf_end) of a ScanSet, built together (a fixed number of launches and one
        read-back for the whole batch); each is interchangeable with search_index(scan_of_keyframe(scanset, kf))"""
        ke = scanset.n_kf if kf_end is None else kf_end
        n = max(int(ke) - int(kf_begin), 0)
        hs = (_vp * max(n, 1))()
        self._ck(self.lib.ltm_search_build_scanset(self.h, scanset.h, kf_begin, ke, hs))
        return [SearchIndex(self, hs[i]) for i in range(n)]

    def estimate_normals(self, indices, k=10, viewpoints=None):
        """ltm_search_estimate_normals: pcl::NormalEstimation (setKSearch(k), setViewPoint) over the targets of all `indices` (SearchIndex objects of this
        context, each at most once) in one launch; viewpoints: (n, 3) or None = the origin for all.  The normals stay with the indices
        (SearchIndex.normals downloads them, icp_align(method="plane") uses them)."""
        indices = list(indices)
        k = _normals_k(k)
        for x in indices:
            if not isinstance(x, SearchIndex):
                raise TypeError("estimate_normals takes SearchIndex objects (Context.search_index)")
        if len({id(x) for x in indices}) != len(indices):
            raise ValueError("an index is listed twice")
        n = len(indices)
        vp = None
        if viewpoints is not None:
            vp = np.ascontiguousarray(viewpoints, dtype=np.float32).reshape(-1)
            if vp.size != 3 * n:
                raise ValueError("one viewpoint (x, y, z) per index")
        hs = (_vp * max(n, 1))(*[x.h for x in indices])
        self._ck(self.lib.ltm_search_estimate_normals(self.h, n, hs, k, None if vp is None else vp.ctypes.data))

    def cluster(self, indices, tolerance, min_size=1, max_size=None):
        """ltm_search_cluster: pcl::EuclideanClusterExtraction over the targets of all `indices` (SearchIndex objects of this context; the same one may be
        listed more than once) in one sequence of launches and one read-back.  Returns one Clusters per index.  max_size None: no upper limit."""
        p = cluster_params(tolerance, min_size, max_size)
        indices, hs = self._index_handles(indices, "cluster")
        n = len(indices)
        out = (_vp * max(n, 1))()
        self._ck(self.lib.ltm_search_cluster(self.h, n, hs, C.byref(p), out))
        return [Clusters(self, out[i]) for i in range(n)]

    def cluster_stats(self, reset=False):
        """ltm_debug_cluster_stats: dict of the six counters since the last reset"""
        return self._stats("ltm_debug_cluster_stats", CLUSTER_STATS, reset)

    def segment_planes(self, scans, distance_threshold, max_iterations=128, axis=None, eps_angle=0.0, seed=0, refine=True, kf_begin=0, kf_end=None):
        """ltm_scanset_segment_planes: pcl::SACSegmentation (SACMODEL_PLANE, or SACMODEL_PERPENDICULAR_PLANE with `axis` and `eps_angle` [rad]; SAC_RANSAC)
        of every keyframe [kf_begin, kf_end) of a ScanSet in one sequence of launches; nothing is read back.  Returns one Planes for the range."""
        p = plane_params(distance_threshold, max_iterations, axis, eps_angle, seed, refine)
        if not isinstance(scans, ScanSet):
            raise TypeError("segment_planes takes a ScanSet (Context.upload_scans); segment_plane takes a cloud")
        kb = int(kf_begin)
        ke = scans.n_kf if kf_end is None else int(kf_end)
        if kb < 0 or ke < kb:
            raise ValueError("need 0 <= kf_begin <= kf_end")
        h = _vp()
        self._ck(self.lib.ltm_scanset_segment_planes(self.h, scans.h, kb, ke, C.byref(p), C.byref(h)))
        return Planes(self, h.value)

    def segment_plane(self, cloud, distance_threshold, max_iterations=128, axis=None, eps_angle=0.0, seed=0, refine=True):
        """ltm_cloud_segment_plane: the same for one Cloud of this context, or an (n, 4) / (n, 3) array; one record"""
        p = plane_params(distance_threshold, max_iterations, axis, eps_angle, seed, refine)
        if isinstance(cloud, ScanSet) or cloud is None:
            raise TypeError("segment_plane takes a Cloud or an array of points")
        if not isinstance(cloud, Cloud):
            cloud = self.upload(_xyzi(cloud))
        h = _vp()
        self._ck(self.lib.ltm_cloud_segment_plane(self.h, cloud.h, C.byref(p), C.byref(h)))
        return Planes(self, h.value)

    def plane_stats(self, reset=False):
        """ltm_debug_plane_stats: dict of the four counters since the last reset"""
        return self._stats("ltm_debug_plane_stats", PLANE_STATS, reset)

    def _stats(self, fn_name, names, reset):
        a = (C.c_uint64 * len(names))()
        self._ck(getattr(self.lib, fn_name)(self.h, a, int(reset)))
        return dict(zip(names, [int(v) for v in a]))

    def _index_handles(self, indices, what):
        """(the indices as a list, their handles as the array a batched entry point takes)"""
        indices = list(indices)
        for x in indices:
            if not isinstance(x, SearchIndex):
                raise TypeError(f"{what} takes SearchIndex objects (Context.search_index)")
        return indices, (_vp * max(len(indices), 1))(*[x.h for x in indices])

    def statistical_outliers(self, indices, mean_k, stddev_mul):
        """ltm_search_filter_statistical: pcl::StatisticalOutlierRemoval (setMeanK, setStddevMulThresh) over the targets of all `indices` (SearchIndex objects
        of this context; the same one may be listed more than once) in one sequence of launches; nothing is read back.  Returns one Outliers with one
        record per index."""
        p = sor_params(mean_k, stddev_mul)
        indices, hs = self._index_handles(indices, "statistical_outliers")
        h = _vp()
        self._ck(self.lib.ltm_search_filter_statistical(self.h, len(indices), hs, C.byref(p), C.byref(h)))
        return Outliers(self, h.value)

    def radius_outliers(self, indices, radius, min_neighbors=1):
        """ltm_search_filter_radius: pcl::RadiusOutlierRemoval (setRadiusSearch, setMinNeighborsInRadius) likewise"""
        p = ror_params(radius, min_neighbors)
        indices, hs = self._index_handles(indices, "radius_outliers")
        h = _vp()
        self._ck(self.lib.ltm_search_filter_radius(self.h, len(indices), hs, C.byref(p), C.byref(h)))
        return Outliers(self, h.value)

    def outlier_stats(self, reset=False):
        """ltm_debug_outlier_stats: dict of the four counters since the last reset"""
        return self._stats("ltm_debug_outlier_stats", OUTLIER_STATS, reset)

    def fpfh(self, indices, k):
        """ltm_search_fpfh: pcl::FPFHEstimation (setKSearch(k)) over the targets of all `indices` (SearchIndex objects of this context with normals, each at
        most once) in one sequence of launches; nothing is read back.  Returns one Fpfh with one record per index."""
        indices, hs = self._index_handles(indices, "fpfh")
        h = _vp()
        self._ck(self.lib.ltm_search_fpfh(self.h, len(indices), hs, int(k), C.byref(h)))
        return Fpfh(self, h.value)

    def fpfh_from_rows(self, rows, offsets=None):
        """ltm_fpfh_upload: an Fpfh from the caller's own rows, (n, 33) float32; offsets (n_records + 1, from 0) cut them into records, None = one record.
        Its k reads 0; for matching any 33-float descriptor"""
        d = np.ascontiguousarray(rows, dtype=np.float32)
        if d.ndim != 2 or d.shape[1] != FPFH_SIZE:
            raise ValueError("rows must be (n, 33)")
        off = np.array([0, len(d)], np.uint64) if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if len(off) < 1 or int(off[0]) != 0 or int(off[-1]) != len(d) or (off[1:] < off[:-1]).any():
            raise ValueError("offsets must run from 0 to the number of rows without decreasing")
        h = _vp()
        self._ck(self.lib.ltm_fpfh_upload(self.h, len(off) - 1, off.ctypes.data, d.ctypes.data, C.byref(h)))
        return Fpfh(self, h.value)

    def fpfh_match(self, target_set, source_set, pairs, kc):
        """ltm_fpfh_match: for every pair (target record, source record) of `pairs` (an (n, 2) integer array) the kc nearest rows of the target record, in
        descriptor space, of every row of the source record: exhaustive and exact, all pairs in one launch; nothing is read back.  The two sets may be
        the same Fpfh.  Returns one Matches with one record per pair."""
        if not isinstance(target_set, Fpfh) or not isinstance(source_set, Fpfh):
            raise TypeError("fpfh_match takes Fpfh objects (Context.fpfh, Context.fpfh_from_rows)")
        p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if (p < 0).any() or (p >= 2 ** 32).any():
            raise ValueError("record numbers must be in [0, 2^32)")
        k = int(kc)
        if k != kc or not 1 <= k <= MATCH_MAX_KC:
            raise ValueError("need 1 <= kc <= 16")
        t, s = np.ascontiguousarray(p[:, 0], dtype=np.uint32), np.ascontiguousarray(p[:, 1], dtype=np.uint32)
        h = _vp()
        self._ck(self.lib.ltm_fpfh_match(self.h, len(p), target_set.h, t.ctypes.data if len(p) else None, source_set.h, s.ctypes.data if len(p) else None,
                                         k, C.byref(h)))
        return Matches(self, h.value)

    def sac_align(self, pairs, matches, **params):
        """ltm_sac_align: pcl::SampleConsensusPrerejective over the matches of every pair in one sequence of launches; nothing is read back.  pairs: a
        sequence of (target SearchIndex, source SearchIndex), pair i belonging to record i of `matches` (Context.fpfh_match with pairs in the same order);
        params: the fields of ltm_sac_params (inlier_distance must be given).  Returns one SacAlignments; its T is what icp_align takes as init."""
        p = sac_params(**params)
        if not isinstance(matches, Matches):
            raise TypeError("sac_align takes the Matches of Context.fpfh_match")
        pairs = list(pairs)
        targets, ht = self._index_handles([t for t, _ in pairs], "sac_align")
        sources, hs = self._index_handles([s for _, s in pairs], "sac_align")
        h = _vp()
        self._ck(self.lib.ltm_sac_align(self.h, len(pairs), ht, hs, matches.h, C.byref(p), C.byref(h)))
        return SacAlignments(self, h.value)

    def sac_stats(self, reset=False):
        """ltm_debug_sac_stats: dict of the four counters since the last reset"""
        return self._stats("ltm_debug_sac_stats", SAC_STATS, reset)

    def fpfh_stats(self, reset=False):
        """ltm_debug_fpfh_stats: dict of the four counters since the last reset"""
        return self._stats("ltm_debug_fpfh_stats", FPFH_STATS, reset)

    # ---- loop submaps
    def loop_submaps(self, scans, keys, search_num, leaf=0.3, affines=None, order="pcl"):
        """ltm_submaps_assemble: Session::loopFindNearKeyframesLocalCoord (affines=None) / CentralCoord (affines: (n_kf, 3, 4) float32, see
        pose6d_to_affine3f) for every key at once.  Returns a ScanSet with one keyframe per key: keyframes key - search_num ... key + search_num of
        `scans`, each moved by its affine in float, concatenated and gridded by pcl::VoxelGrid at `leaf` (0: no grid); order: "pcl" sums a voxel in
        PCL's std::sort order (host threads), "input" in input order on the device alone."""
        k = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1)
        a = None
        if affines is not None:
            a = np.ascontiguousarray(affines, dtype=np.float32).reshape(-1, 12)
            if a.shape[0] != scans.n_kf:
                raise ValueError("one affine per keyframe of the scan set")
        out = _u64()
        self._ck(self.lib.ltm_submaps_assemble(self.h, scans.h, None if a is None else a.ctypes.data, k.ctypes.data, k.size, int(search_num), float(leaf),
                                               ORDERS[order], C.byref(out)))
        return ScanSet(self, out.value)

    def verify_loops(self, target_scans, source_scans, pairs, target_affines=None, source_affines=None, search_num=25, leaf=0.3,
                     fitness_threshold=0.5, order="pcl", max_batch_points=1 << 26, method="point", normal_k=_NORMAL_K_OF_METHOD, coarse=None, fpfh_k=16,
                     match_k=4, sac=None, **icp):
        """The body of LTslam::addSCloops' loop (LTslam.cpp:370-416) for all `pairs` = (target key, source key): the target submap (+-search_num
        keyframes) and its search index are made ONCE per distinct target key, the source submap is the source keyframe alone (searchNum = 0), every
        source is aligned to its target by icp_align, and a pair is accepted iff converged and fitness <= fitness_threshold (loopFitnessScoreThreshold,
        0.5 by default: ltslam/src/RosParamServer.cpp:23).  The work is cut into batches of consecutive pairs whose submaps hold at most max_batch_points
        points before the grid (estimated from the scan sets' offsets).  method="plane" verifies with point-to-plane ICP: the normals of each batch of
        target indices are estimated in one call (normal_k neighbours), the viewpoint at the key keyframe's translation (the origin without affines).
        method="gicp" verifies with generalized ICP (gicp_epsilon among **icp): the source keyframes'
        indices are built with search_index_batch as well, and the normals of the batch's source and target indices are estimated in ONE call (targets
        first; the viewpoint of a source at its keyframe's translation).
        normal_k, when not given, is the method's own: 10 for "plane", 20 for "gicp" (PCL's k_correspondences_, DeviceICP's default too).
        coarse="fpfh" gives every pair a start from its descriptors before the ICP: source indices are built as for "gicp", normals (10 neighbours, no
        viewpoint) and FPFH descriptors (fpfh_k) of the batch's targets and sources are made in one call each, the pairs are matched (match_k lists) and
        aligned by sac_align (sac: a dict of its parameters, inlier_distance among them), and the chosen ICP method starts from that T; a pair without
        `found` starts from its given start (init= among **icp, one per pair; identity without one).  coarse=None, the default, is the path without any of this.
        Returns (ICP_RESULT records, accept mask), one entry per pair."""
        if coarse not in (None, "fpfh"):
            raise ValueError('coarse must be None or "fpfh"')
        if coarse and (sac is None or "inlier_distance" not in sac):
            raise ValueError('coarse="fpfh" needs sac=dict(inlier_distance=...)')
        method = _icp_method(method)
        if method != "point":
            normal_k = normals_k_of(method, normal_k)
        pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        res = np.zeros(len(pairs), dtype=ICP_RESULT)
        given = None      # coarse: the caller's own starts (init=, one per pair), kept for the pairs the coarse step does not find
        if coarse and icp.get("init") is not None:
            given = np.ascontiguousarray(icp["init"], dtype=np.float64).reshape(len(pairs), 4, 4)
        t_off = target_scans.offsets().astype(np.int64)
        s_off = source_scans.offsets().astype(np.int64)

        def window_points(off, key, sn):
            lo, hi = max(key - sn, 0), min(key + sn, len(off) - 2)
            return int(off[hi + 1] - off[lo]) if hi >= lo else 0

        batches, cur, seen, pts = [], [], set(), 0
        for i, (tk, sk) in enumerate(pairs):
            add = window_points(s_off, int(sk), 0) + (0 if int(tk) in seen else window_points(t_off, int(tk), search_num))
            if cur and pts + add > max_batch_points:
                batches.append(cur)
                cur, seen, pts = [], set(), 0
                add = window_points(s_off, int(sk), 0) + window_points(t_off, int(tk), search_num)
            cur.append(i)
            seen.add(int(tk))
            pts += add
        if cur:
            batches.append(cur)
        for b in batches:
            tkeys = sorted({int(pairs[i, 0]) for i in b})
            slot = {k: j for j, k in enumerate(tkeys)}
            tsub = self.loop_submaps(target_scans, tkeys, search_num, leaf, target_affines, order)
            ssub = self.loop_submaps(source_scans, [int(pairs[i, 1]) for i in b], 0, leaf, source_affines, order)
            idx = self.search_index_batch(tsub)
            sidx = []
            try:
                if coarse:
                    sidx = self.search_index_batch(ssub)
                    starts = self._coarse_starts(idx, sidx, [slot[int(pairs[i, 0])] for i in b], fpfh_k, match_k, sac, None if given is None else given[b])
                if method == "gicp":
                    sidx = sidx or self.search_index_batch(ssub)
                    vp = None
                    if target_affines is not None or source_affines is not None:
                        zero = np.zeros(3, np.float32)
                        ta = None if target_affines is None else np.asarray(target_affines, dtype=np.float32).reshape(-1, 3, 4)
                        sa = None if source_affines is None else np.asarray(source_affines, dtype=np.float32).reshape(-1, 3, 4)
                        vp = np.stack([zero if ta is None else ta[k, :, 3] for k in tkeys] + [zero if sa is None else sa[int(pairs[i, 1]), :, 3] for i in b])
                    self.estimate_normals(idx + sidx, normal_k, vp)
                    res[b] = self.icp_align([(idx[slot[int(pairs[i, 0])]], sidx[j]) for j, i in enumerate(b)], method=method, **(dict(icp, init=starts) if coarse else icp))
                    continue
                if method == "plane":
                    vp = None
                    if target_affines is not None:
                        vp = np.asarray(target_affines, dtype=np.float32).reshape(-1, 3, 4)[tkeys, :, 3]
                    self.estimate_normals(idx, normal_k, vp)
                res[b] = self.icp_align([(idx[slot[int(pairs[i, 0])]], (ssub, j)) for j, i in enumerate(b)], method=method, **(dict(icp, init=starts) if coarse else icp))
            finally:
                for x in idx + sidx:
                    x.close()
                tsub.free()
                ssub.free()
        return res, (res["converged"] != 0) & (res["fitness"] <= fitness_threshold)

    def _coarse_starts(self, idx, sidx, target_of, fpfh_k, match_k, sac, given):
        """verify_loops(coarse="fpfh"): (n, 4, 4) starts of the pairs (idx[target_of[j]], sidx[j]): sac_align's T where found, elsewhere the pair's
        given start (`given`, (n, 4, 4), None = identity)"""
        self.estimate_normals(idx + sidx, 10)
        with self.fpfh(idx + sidx, fpfh_k) as f, self.fpfh_match(f, f, [(t, len(idx) + j) for j, t in enumerate(target_of)], match_k) as m, \
                self.sac_align([(idx[t], sidx[j]) for j, t in enumerate(target_of)], m, **sac) as a:
            found, T = a.found.astype(bool), a.T
        return np.where(found[:, None, None], T, np.eye(4)[None] if given is None else given)

    # ---- scan context
    def scan_contexts(self, scans, kf_begin=0, kf_end=None, **params):
        """ltm_sc_from_scanset: Scan Context descriptors and keys of keyframes [kf_begin, kf_end) of a ScanSet (makeAndSaveScancontextAndKeys per
        keyframe); params: the fields of ltm_sc_params, the reference's values by default"""
        p = sc_params(**params)
        h = _vp()
        ke = scans.n_kf if kf_end is None else kf_end
        self._ck(self.lib.ltm_sc_from_scanset(self.h, scans.h, kf_begin, ke, C.byref(p), C.byref(h)))
        return ScanContexts(self, h.value, p)

    def scan_contexts_from(self, desc, **params):
        """ltm_sc_from_descriptors: a descriptor set from (n, num_ring, num_sector) float64 descriptors made elsewhere (saveScancontextAndKeys)"""
        p = sc_params(**params)
        d = np.ascontiguousarray(desc, dtype=np.float64).reshape(-1, p.num_ring, p.num_sector)
        h = _vp()
        self._ck(self.lib.ltm_sc_from_descriptors(self.h, d.ctypes.data, d.shape[0], C.byref(p), C.byref(h)))
        return ScanContexts(self, h.value, p)

    # ---- icp
    def icp_align(self, pairs, init=None, trace=False, method="point", gicp_epsilon=1e-3, **params):
        """ltm_icp_align (method="point", the default) / ltm_icp_align_plane (method="plane": every target must carry normals, see estimate_normals;
        state 5 = degenerate system): ICP of every (target, source) of `pairs` in one batch -- target a SearchIndex of this context (one index
        may serve many pairs), source a Cloud of this context, an (n, 3) / (n, 4) array or (ScanSet, keyframe) -- when every source is a keyframe of one
        ScanSet they are read in place (ltm_icp_align_scanset).  init: (n, 4, 4) source->target start transforms
        (None: identity); params: the fields of ltm_icp_params, the reference's values by default.  Returns a record array of dtype ICP_RESULT
        (T, fitness, last_mse, converged, iterations, state, n_corr), one record per pair; with trace=True also the (n, max_iterations, 2)
        array of (n_corr, mse) per iteration, NaN where no iteration ran.
        method="gicp" is ltm_icp_align_gicp, generalized (plane-to-plane) ICP: the source of every pair is a SearchIndex too (anything else raises
        TypeError, an empty batch ValueError: there is nothing to say which kind of source it would have had), both sides must carry normals, and
        gicp_epsilon in (0, 1] (PCL's 0.001 by default) regularises the covariances the normals imply; the sources are read in place."""
        if _icp_method(method) == "gicp":
            return self._icp_align_gicp(list(pairs), init, trace, gicp_epsilon, params)
        plane = method == "plane"
        align_clouds = self.lib.ltm_icp_align_plane if plane else self.lib.ltm_icp_align
        align_scanset = self.lib.ltm_icp_align_plane_scanset if plane else self.lib.ltm_icp_align_scanset
        p = icp_params(**params)
        pairs = list(pairs)
        n = len(pairs)
        res = np.zeros(n, dtype=ICP_RESULT)
        assert ICP_RESULT.itemsize == 160
        tr = np.full((n, max(p.max_iterations, 0), 2), np.nan) if trace else None
        if n:
            for t, _ in pairs:
                if not isinstance(t, SearchIndex):
                    raise TypeError("the target of a pair must be a SearchIndex (Context.search_index)")
            made = []
            try:
                th = (_vp * n)(*[t.h for t, _ in pairs])
                i16 = None
                if init is not None:
                    i16 = np.ascontiguousarray(init, dtype=np.float64).reshape(n, 16)
                in_set = [isinstance(s_, tuple) and len(s_) == 2 and isinstance(s_[0], ScanSet) for _, s_ in pairs]
                if all(in_set) and all(s_[0] is pairs[0][1][0] for _, s_ in pairs):
                    # every source a keyframe of ONE scan set (the submaps of loop_submaps): read in place
                    kf = np.ascontiguousarray([s_[1] for _, s_ in pairs], dtype=np.uint32)
                    self._ck(align_scanset(self.h, n, th, pairs[0][1][0].h, kf.ctypes.data, None if i16 is None else i16.ctypes.data,
                                                            C.byref(p), res.ctypes.data, tr.ctypes.data if trace and tr.size else None))
                    return (res, tr) if trace else res
                src = []
                for (_, s_), sset in zip(pairs, in_set):
                    if sset:
                        s_ = self.scan_of_keyframe(s_[0], int(s_[1]))
                        made.append(s_)
                    elif not isinstance(s_, Cloud):
                        s_ = self.upload(_xyzi(s_))
                        made.append(s_)
                    src.append(s_)
                sh = (C.c_uint64 * n)(*[s_.h for s_ in src])
                self._ck(align_clouds(self.h, n, th, sh, None if i16 is None else i16.ctypes.data, C.byref(p), res.ctypes.data,
                                                tr.ctypes.data if trace and tr.size else None))
            finally:
                for s_ in made:
                    s_.free()
        return (res, tr) if trace else res

    def _icp_align_gicp(self, pairs, init, trace, gicp_epsilon, params):
        n = len(pairs)
        if not n:
            raise ValueError("method='gicp' needs at least one (target SearchIndex, source SearchIndex) pair")
        eps = float(gicp_epsilon)
        if not (np.isfinite(eps) and 0.0 < eps <= 1.0):
            raise ValueError("gicp_epsilon must be in (0, 1]")
        for t, s_ in pairs:
            if not isinstance(t, SearchIndex) or not isinstance(s_, SearchIndex):
                raise TypeError("method='gicp' takes (SearchIndex, SearchIndex) pairs: the source needs an index and normals of its own")
        p = icp_params(**params)
        res = np.zeros(n, dtype=ICP_RESULT)
        tr = np.full((n, max(p.max_iterations, 0), 2), np.nan) if trace else None
        th = (_vp * n)(*[t.h for t, _ in pairs])
        sh = (_vp * n)(*[s_.h for _, s_ in pairs])
        i16 = None if init is None else np.ascontiguousarray(init, dtype=np.float64).reshape(n, 16)
        self._ck(self.lib.ltm_icp_align_gicp(self.h, n, th, sh, None if i16 is None else i16.ctypes.data, C.byref(p), eps, res.ctypes.data,
                                             tr.ctypes.data if trace and tr.size else None))
        return (res, tr) if trace else res

    # ---- debug / parity
    def pool_live(self):
        """ltm_debug_pool_live: (blocks, bytes) of the device pool that are handed out"""
        b, n = _u64(), _u64()
        self._ck(self.lib.ltm_debug_pool_live(self.h, C.byref(b), C.byref(n)))
        return b.value, n.value

    def rimg_size(self, alpha):
        r, c = _i(), _i()
        self.lib.ltm_rimg_size(self.vfov, self.hfov, alpha, C.byref(r), C.byref(c))
        return r.value, c.value

    def debug_range_image(self, cloud, alpha, T1=None, T2=None, want_idx=True):
        R, Cc = self.rimg_size(alpha)
        rimg = np.empty((R, Cc), dtype=np.float32)
        idx = np.empty((R, Cc), dtype=np.int32) if want_idx else None
        t1 = None if T1 is None else _mat16(T1)
        t2 = None if T2 is None else _mat16(T2)
        self._ck(self.lib.ltm_debug_range_image(self.h, cloud.h, None if t1 is None else t1.ctypes.data,
                                                None if t2 is None else t2.ctypes.data, alpha, rimg.ctypes.data,
                                                idx.ctypes.data if want_idx else None))
        return rimg, idx

    def debug_project(self, xyz, alpha):
        a = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        sph = np.empty((a.shape[0], 3), dtype=np.float32)
        rc = np.empty((a.shape[0], 2), dtype=np.int32)
        self._ck(self.lib.ltm_debug_project(self.h, a.ctypes.data, a.shape[0], alpha, sph.ctypes.data, rc.ctypes.data))
        return sph, rc

    def cull_check(self, xyz, alpha, inv_pose=None):
        a = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        t = None if inv_pose is None else _mat16(inv_pose)
        v = _u64()
        self._ck(self.lib.ltm_debug_cull_check(self.h, a.ctypes.data, a.shape[0], None if t is None else t.ctypes.data, alpha, C.byref(v)))
        return int(v.value)

    def occlusion_stats(self, reset=False):
        a, b, d = _u64(), _u64(), _u64()
        self._ck(self.lib.ltm_debug_occlusion_stats(self.h, C.byref(a), C.byref(b), C.byref(d), 1 if reset else 0))
        return a.value, b.value, d.value

    def voxel_stats(self, reset=False):
        a, b = _u64(), _u64()
        self._ck(self.lib.ltm_debug_voxel_stats(self.h, C.byref(a), C.byref(b), 1 if reset else 0))
        return int(a.value), int(b.value)

    def knn_stats(self, reset=False):
        """(scan queries of two-phase ltm_knn_partition calls, queries phase 1 left undecided, two-phase calls, calls whose phase-2 queue stayed in
        scan order); counted only in a context created with LTM_KNN_STATS=1"""
        q, u, t, s = _u64(), _u64(), _u64(), _u64()
        self._ck(self.lib.ltm_debug_knn_stats(self.h, C.byref(q), C.byref(u), C.byref(t), C.byref(s), 1 if reset else 0))
        return int(q.value), int(u.value), int(t.value), int(s.value)

    def cull_validation(self):
        """(image shapes whose bounded-error projection was validated on first use, shapes that failed and fell back to the exact kernels)"""
        a, b = _u64(), _u64()
        self._ck(self.lib.ltm_debug_cull_validation(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def cull_stats(self, reset=True):
        a, b = _u64(), _u64()
        self._ck(self.lib.ltm_debug_cull_stats(self.h, C.byref(a), C.byref(b), 1 if reset else 0))
        return int(a.value), int(b.value)

    def selfcheck(self):
        m = (C.c_uint64 * 3)()
        on = _i()
        self._ck(self.lib.ltm_debug_selfcheck(self.h, m, C.byref(on)))
        return [int(x) for x in m], bool(on.value)

    # ---- measurement
    def synchronize(self):
        self._ck(self.lib.ltm_synchronize(self.h))

    def clear_caches(self):
        self._ck(self.lib.ltm_clear_caches(self.h))

    def stream(self):
        return self.lib.ltm_stream(self.h)

    def profile_enable(self, on=True):
        self._ck(self.lib.ltm_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        self._ck(self.lib.ltm_profile_reset(self.h))

    def profile_read(self):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        launches = (C.c_uint64 * cap)()
        units = (C.c_double * cap)()
        nbytes = (C.c_double * cap)()
        n = self.lib.ltm_profile_read(self.h, names, ms, launches, units, nbytes, cap)
        if n < 0:
            self._ck(n)
        nb_c = (C.c_double * cap)()
        self._ck(min(self.lib.ltm_profile_read_compulsory(self.h, nb_c, cap), 0))
        return {names[i].decode(): dict(ms=ms[i], launches=int(launches[i]), units=units[i], bytes=nbytes[i], bytes_c=nb_c[i]) for i in range(min(n, cap))}


def _xyzi(a):
    """(n, 3) or (n, 4) points -> packed float32 XYZI"""
    a = np.asarray(a, dtype=np.float32)
    if a.ndim == 2 and a.shape[1] == 3:
        a = np.concatenate([a, np.zeros((a.shape[0], 1), np.float32)], axis=1)
    return _np_pts(a)


class _PtrHandle:
    """a pointer handle of the library owned by a Context: close() (or leaving a `with` block, or the object going) frees it with the subclass's _free"""
    _free = None
    _host = None      # the per-record arrays of a set, once downloaded

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if self.h and self.ctx.h:
            getattr(self.ctx.lib, self._free)(self.ctx.h, self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _out(self, dev, n, dtype, as_torch):
        """n elements of a library device array -> numpy array or torch CUDA tensor (a copy either way)"""
        if as_torch:
            import torch
            t = torch.empty(n, dtype={np.int32: torch.int32, np.float32: torch.float32, np.uint64: torch.int64, np.uint8: torch.uint8}[dtype],
                            device=f"cuda:{self.ctx.device}")
            if n:
                torch.cuda.synchronize(t.device)
                self.ctx._ck(self.ctx.lib.ltm_buffer_copy(self.ctx.h, t.data_ptr(), dev, n * t.element_size(), 2))
            return t
        a = np.empty(n, dtype=dtype)
        if n:
            self.ctx._ck(self.ctx.lib.ltm_buffer_copy(self.ctx.h, a.ctypes.data, dev, a.nbytes, 1))
        return a


class SearchIndex(_PtrHandle):
    """ltm_search: device-resident exact k-NN / radius search over one cloud (pcl::KdTreeFLANN's queries, semantics in include/ltm.h).
    Queries are Clouds of the same context or (n, 3) / (n, 4) arrays.  Results are numpy arrays, or with as_torch=True CUDA tensors that
    torch allocated and owns (the library's buffers are copied into them device to device)."""

    _free = "ltm_search_free"

    def _query(self, query):
        return query if isinstance(query, Cloud) else self.ctx.upload(_xyzi(query))

    def info(self):
        """(target points, finite target points)"""
        a, b = C.c_size_t(), C.c_size_t()
        self.ctx._ck(self.ctx.lib.ltm_search_info(self.ctx.h, self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def knn(self, query, k, as_torch=False):
        """nearestKSearch for every query point: (idx int32 [n, k], d2 float32 [n, k]); padding -1 / +inf"""
        q = self._query(query)
        n = len(q)
        nb = max(n * int(k), 1) * 4
        pi, pd = _vp(), _vp()
        self.ctx._ck(self.ctx.lib.ltm_buffer_alloc(self.ctx.h, nb, C.byref(pi)))
        try:
            self.ctx._ck(self.ctx.lib.ltm_buffer_alloc(self.ctx.h, nb, C.byref(pd)))
            try:
                self.ctx._ck(self.ctx.lib.ltm_knn_search(self.ctx.h, self.h, q.h, int(k), pi, pd))
                idx = self._out(pi.value, n * int(k), np.int32, as_torch)
                d2 = self._out(pd.value, n * int(k), np.float32, as_torch)
            finally:
                self.ctx.lib.ltm_buffer_free(self.ctx.h, pd)
        finally:
            self.ctx.lib.ltm_buffer_free(self.ctx.h, pi)
        return idx.reshape(n, int(k)), d2.reshape(n, int(k))

    def radius(self, query, r, max_nn=0, as_torch=False):
        """radiusSearch for every query point, CSR: (offsets uint64 [n+1] (int64 as torch), idx int32 [total], d2 float32 [total])"""
        q = self._query(query)
        res = _vp()
        self.ctx._ck(self.ctx.lib.ltm_radius_search(self.ctx.h, self.h, q.h, float(r), int(max_nn), C.byref(res)))
        try:
            nq, tot = C.c_size_t(), C.c_size_t()
            po, pi, pd = _vp(), _vp(), _vp()
            self.ctx._ck(self.ctx.lib.ltm_search_result_info(self.ctx.h, res, C.byref(nq), C.byref(tot), C.byref(po), C.byref(pi), C.byref(pd)))
            off = self._out(po.value, nq.value + 1, np.uint64, as_torch)
            idx = self._out(pi.value, tot.value, np.int32, as_torch)
            d2 = self._out(pd.value, tot.value, np.float32, as_torch)
        finally:
            self.ctx.lib.ltm_search_result_free(self.ctx.h, res)
        return off, idx, d2

    def estimate_normals(self, k=10, viewpoint=None):
        """ltm_search_estimate_normals for this index alone: setKSearch(k), setViewPoint(*viewpoint) (None: the origin), compute"""
        self.ctx.estimate_normals([self], k, None if viewpoint is None else np.asarray(viewpoint, dtype=np.float32).reshape(1, 3))

    def normals_k(self):
        """k of the normals the index carries, 0 if none"""
        k, p = _i(), _vp()
        self.ctx._ck(self.ctx.lib.ltm_search_normals_info(self.ctx.h, self.h, C.byref(k), C.byref(p)))
        return k.value

    def normals(self):
        """ltm_search_normals_download: (n_target, 4) float32 (nx, ny, nz, curvature) in the target's original order; NaN rows for non-finite points"""
        out = np.empty((self.info()[0], 4), np.float32)
        self.ctx._ck(self.ctx.lib.ltm_search_normals_download(self.ctx.h, self.h, out.ctypes.data))
        return out

    def cluster(self, tolerance, min_size=1, max_size=None):
        """ltm_search_cluster for this index alone: setClusterTolerance(tolerance), setMinClusterSize, setMaxClusterSize (None: no limit), extract"""
        return self.ctx.cluster([self], tolerance, min_size, max_size)[0]

    def statistical_outliers(self, mean_k, stddev_mul):
        """ltm_search_filter_statistical for this index alone: setMeanK(mean_k), setStddevMulThresh(stddev_mul), filter; an Outliers of one record"""
        return self.ctx.statistical_outliers([self], mean_k, stddev_mul)

    def fpfh(self, k):
        """ltm_search_fpfh for this index alone: setKSearch(k), compute; an Fpfh of one record (the index needs normals: estimate_normals)"""
        return self.ctx.fpfh([self], k)

    def radius_outliers(self, radius, min_neighbors=1):
        """ltm_search_filter_radius for this index alone: setRadiusSearch(radius), setMinNeighborsInRadius(min_neighbors), filter"""
        return self.ctx.radius_outliers([self], radius, min_neighbors)



CLUSTER_STATS = ("pairs_tested", "edges_found", "leaves_visited", "clique_leaves", "clique_early_exits", "hook_retries")


def cluster_params(tolerance, min_size=1, max_size=None):
    """ltm_cluster_params, checked: tolerance finite and > 0, 1 <= min_size <= max_size (None or 0: no upper limit)"""
    tolerance = float(tolerance)
    if not (np.isfinite(tolerance) and tolerance > 0.0):
        raise ValueError("tolerance must be finite and > 0")
    lo, hi = int(min_size), 0 if max_size is None else int(max_size)
    if lo < 1 or hi < 0 or lo >= 2 ** 32 or hi >= 2 ** 32 or (hi != 0 and hi < lo):
        raise ValueError("need 1 <= min_size <= max_size (max_size None: no limit)")
    return ClusterParams(tolerance, lo, hi)


class Clusters(_PtrHandle):
    """ltm_clusters: the Euclidean clusters of one search index's target (semantics in include/ltm.h, "clusters").  Labels and point indices refer to the
    target's ORIGINAL order; clusters are numbered by size descending, ties by the lowest original index."""

    _free = "ltm_clusters_free"

    def info(self):
        """(target points, clusters, clustered points)"""
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.ctx._ck(self.ctx.lib.ltm_clusters_info(self.ctx.h, self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def __len__(self):
        return self.info()[1]

    def _device(self):
        pl, po, pi = _vp(), _vp(), _vp()
        self.ctx._ck(self.ctx.lib.ltm_clusters_device(self.ctx.h, self.h, C.byref(pl), C.byref(po), C.byref(pi)))
        return pl.value, po.value, pi.value

    def labels(self, as_torch=False):
        """int32 [n_target]: the cluster of every target point, -1 = none"""
        return self._out(self._device()[0], self.info()[0], np.int32, as_torch)

    def indices(self, as_torch=False):
        """CSR: (offsets uint64 [n_clusters + 1] (int64 as torch), idx int32 [clustered points]); row c = cluster c in ascending original index"""
        _, nc, npts = self.info()
        _, po, pi = self._device()
        return self._out(po, nc + 1, np.uint64, as_torch), self._out(pi, npts, np.int32, as_torch)

    def _download(self):
        if self._host is None:
            nc = self.info()[1]
            sizes, first = np.empty(nc, np.uint32), np.empty(nc, np.int32)
            box, cen = np.empty((nc, 6), np.float32), np.empty((nc, 3), np.float64)
            self.ctx._ck(self.ctx.lib.ltm_clusters_download(self.ctx.h, self.h, None, sizes.ctypes.data, first.ctypes.data, box.ctypes.data, cen.ctypes.data))
            self._host = (sizes, first, box, cen)
        return self._host

    sizes = property(lambda self: self._download()[0], doc="uint32 [n_clusters]")
    first_index = property(lambda self: self._download()[1], doc="int32 [n_clusters]: lowest original index")
    boxes = property(lambda self: self._download()[2], doc="float32 [n_clusters, 6]: min xyz, max xyz")
    centroids = property(lambda self: self._download()[3], doc="float64 [n_clusters, 3]")

    def extract(self, cloud):
        """ltm_clusters_extract: the clustered points of `cloud` (the Cloud the index was built over, or its array) as a ScanSet, keyframe c = cluster c"""
        if not isinstance(cloud, Cloud):
            cloud = self.ctx.upload(_xyzi(cloud))
        out = _u64()
        self.ctx._ck(self.ctx.lib.ltm_clusters_extract(self.ctx.h, self.h, cloud.h, C.byref(out)))
        return ScanSet(self.ctx, out.value)



def _icp_method(method):
    if method not in ICP_METHODS:
        raise ValueError(f"method must be one of {ICP_METHODS}, not {method!r}")
    return method


def normals_k_of(method, normal_k=_NORMAL_K_OF_METHOD):
    """the neighbours verify_loops estimates normals with: normal_k where the caller gave one, else the method's own (10 for "plane", 20 for "gicp")"""
    return _normals_k(GICP_NORMAL_K if normal_k is _NORMAL_K_OF_METHOD and _icp_method(method) == "gicp" else normal_k)


def _normals_k(k):
    k = int(k)
    if not 3 <= k <= 64:
        raise ValueError("k must be in [3, 64]")
    return k


def icp_params(**over):
    """ltm_icp_params: ltm_icp_default_params with the given fields replaced"""
    p = IcpParams()
    load_library().ltm_icp_default_params(C.byref(p))
    for k, v in over.items():
        if k not in dict(IcpParams._fields_):
            raise TypeError(f"ltm_icp_params has no field {k!r}")
        setattr(p, k, v)
    return p


def sc_params(**over):
    """ltm_sc_params: ltm_sc_default_params with the given fields replaced"""
    p = ScParams()
    load_library().ltm_sc_default_params(C.byref(p))
    for k, v in over.items():
        if k not in dict(ScParams._fields_):
            raise TypeError(f"ltm_sc_params has no field {k!r}")
        setattr(p, k, v)
    return p


def sc_paths(num_ring, num_sector):
    """ltm_debug_sc_paths: (the descriptor scatter pre-reduces in LDS, the pair distance stages both descriptors in LDS) for this shape; host only"""
    a, b = _i(), _i()
    rc = load_library().ltm_debug_sc_paths(num_ring, num_sector, C.byref(a), C.byref(b))
    if rc != 0:
        raise LtmError(rc, "ltm_debug_sc_paths")
    return bool(a.value), bool(b.value)


PLANE_STATS = ("point_hypothesis_tests", "valid_hypotheses", "records", "records_refined")
PLANE_MAX_ITERATIONS = 4096


def plane_block_points():
    """ltm_plane_block_points: the points of one record that a workgroup of the count kernel takes (needs no device)"""
    return int(load_library().ltm_plane_block_points())


def plane_params(distance_threshold, max_iterations=128, axis=None, eps_angle=0.0, seed=0, refine=True):
    """ltm_plane_params, checked: distance_threshold finite and > 0, 1 <= max_iterations <= 4096, axis None or three finite numbers, with a non-zero axis
    eps_angle finite and >= 0, 0 <= seed < 2^32"""
    thr = float(distance_threshold)
    if not (np.isfinite(thr) and thr > 0.0):
        raise ValueError("distance_threshold must be finite and > 0")
    it = int(max_iterations)
    if it != max_iterations or not 1 <= it <= PLANE_MAX_ITERATIONS:
        raise ValueError("need 1 <= max_iterations <= 4096")
    sd = int(seed)
    if sd != seed or not 0 <= sd < 2 ** 32:
        raise ValueError("need 0 <= seed < 2^32")
    ax = np.zeros(3) if axis is None else np.asarray(axis, dtype=np.float64).reshape(-1)
    if ax.shape != (3,) or not np.isfinite(ax).all():
        raise ValueError("axis must be three finite numbers")
    eps = float(eps_angle)
    if ax.any() and not (np.isfinite(eps) and eps >= 0.0):
        raise ValueError("eps_angle must be finite and >= 0")
    if not ax.any():
        eps = eps if np.isfinite(eps) else 0.0
    return PlaneParams(thr, it, sd, (C.c_double * 3)(*ax.tolist()), eps, 1 if refine else 0)


class Planes(_PtrHandle):
    """ltm_planes: the RANSAC plane of every record (keyframe of a scan-set range, or one cloud); semantics in include/ltm.h, "planes".  Labels are in the order
    of the range's points."""

    _free = "ltm_planes_free"

    def info(self):
        """(records, points, max_iterations)"""
        a, b, m = C.c_size_t(), C.c_size_t(), C.c_uint32()
        self.ctx._ck(self.ctx.lib.ltm_planes_info(self.ctx.h, self.h, C.byref(a), C.byref(b), C.byref(m)))
        return a.value, b.value, m.value

    def __len__(self):
        return self.info()[0]

    def _device(self):
        pl, pc, pv = _vp(), _vp(), _vp()
        self.ctx._ck(self.ctx.lib.ltm_planes_device(self.ctx.h, self.h, C.byref(pl), C.byref(pc), C.byref(pv)))
        return pl.value, pc.value, pv.value

    def _download(self):
        if self._host is None:
            nr = self.info()[0]
            found, best, cons, nval = np.empty(nr, np.uint8), np.empty(nr, np.int32), np.empty(nr, np.uint32), np.empty(nr, np.uint32)
            nin, ref, coeff, point = np.empty(nr, np.uint32), np.empty(nr, np.uint8), np.empty((nr, 4), np.float64), np.empty((nr, 3), np.float64)
            self.ctx._ck(self.ctx.lib.ltm_planes_download(self.ctx.h, self.h, found.ctypes.data, best.ctypes.data, cons.ctypes.data, nval.ctypes.data,
                                                          nin.ctypes.data, ref.ctypes.data, coeff.ctypes.data, point.ctypes.data, None, None, None))
            self._host = (found, best, cons, nval, nin, ref, coeff, point)
        return self._host

    found = property(lambda self: self._download()[0], doc="uint8 [n_records]: 1 = the record has a plane")
    best = property(lambda self: self._download()[1], doc="int32 [n_records]: the best hypothesis, -1 = none")
    consensus = property(lambda self: self._download()[2], doc="uint32 [n_records]: its inlier count")
    n_valid = property(lambda self: self._download()[3], doc="uint32 [n_records]: valid hypotheses")
    n_inliers = property(lambda self: self._download()[4], doc="uint32 [n_records]: labels set by the final plane")
    refined = property(lambda self: self._download()[5], doc="uint8 [n_records]: 1 = the coefficients are the refined ones")
    coefficients = property(lambda self: self._download()[6], doc="float64 [n_records, 4]: a, b, c, d")
    points = property(lambda self: self._download()[7], doc="float64 [n_records, 3]: the plane point the labels were taken about")

    def labels(self, as_torch=False):
        """uint8 [n_points]: 1 = inlier of its record's final plane"""
        return self._out(self._device()[0], self.info()[1], np.uint8, as_torch)

    def hypothesis_counts(self):
        """uint32 [n_records, max_iterations]: the inlier count of every hypothesis, 0 where invalid"""
        nr, _, m = self.info()
        return self._out(self._device()[1], nr * m, np.uint32, False).reshape(nr, m)

    def hypothesis_valid(self):
        """uint8 [n_records, max_iterations]"""
        nr, _, m = self.info()
        return self._out(self._device()[2], nr * m, np.uint8, False).reshape(nr, m)

    def split(self, scans_or_cloud):
        """ltm_planes_split_scanset / _cloud: (inliers, rest) of the ScanSet or Cloud the set was made from, input order kept"""
        a, b = _u64(), _u64()
        if isinstance(scans_or_cloud, ScanSet):
            self.ctx._ck(self.ctx.lib.ltm_planes_split_scanset(self.ctx.h, self.h, scans_or_cloud.h, C.byref(a), C.byref(b)))
            return ScanSet(self.ctx, a.value), ScanSet(self.ctx, b.value)
        cloud = scans_or_cloud if isinstance(scans_or_cloud, Cloud) else self.ctx.upload(_xyzi(scans_or_cloud))
        self.ctx._ck(self.ctx.lib.ltm_planes_split_cloud(self.ctx.h, self.h, cloud.h, C.byref(a), C.byref(b)))
        return Cloud(self.ctx, a.value), Cloud(self.ctx, b.value)



OUTLIER_STATS = ("finite_points", "distance_evaluations", "radius_early_stops", "records")
OUTLIERS_STATISTICAL, OUTLIERS_RADIUS = 0, 1
SOR_MAX_MEAN_K = 63      # mean_k + 1 neighbours: the limit of ltm_knn_search


def sor_params(mean_k, stddev_mul):
    """ltm_sor_params, checked: 1 <= mean_k <= 63, stddev_mul finite"""
    k = int(mean_k)
    if k != mean_k or not 1 <= k <= SOR_MAX_MEAN_K:
        raise ValueError("need 1 <= mean_k <= 63")
    mul = float(stddev_mul)
    if not np.isfinite(mul):
        raise ValueError("stddev_mul must be finite")
    return SorParams(k, mul)


def ror_params(radius, min_neighbors=1):
    """ltm_ror_params, checked: radius finite and > 0, 1 <= min_neighbors < 2^32"""
    r = float(radius)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError("radius must be finite and > 0")
    m = int(min_neighbors)
    if m != min_neighbors or not 1 <= m < 2 ** 32:
        raise ValueError("need 1 <= min_neighbors < 2^32")
    return RorParams(r, m)


class _DeviceBlock:
    """a library device array as __cuda_array_interface__ (version 2): what torch.as_tensor takes without a copy (torch takes no read-only flag); keeps its owner alive"""

    def __init__(self, owner, ptr, shape, typestr):
        self.owner = owner
        self.__cuda_array_interface__ = dict(shape=tuple(int(v) for v in shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)


FPFH_STATS = ("finite_points", "distance_evaluations", "pairs_skipped", "lds_points")
FPFH_SIZE, FPFH_MIN_K, FPFH_MAX_K = 33, 2, 64


class Fpfh(_PtrHandle):
    """ltm_fpfh: the FPFH descriptors of ltm_search_fpfh, one record per listed search index (semantics in include/ltm.h, "fpfh").  The rows hold the
    records one after the other, each in its target's ORIGINAL order; offsets() says where each begins."""

    _free = "ltm_fpfh_free"

    def info(self):
        """(records, rows, k)"""
        a, b, k = C.c_size_t(), C.c_size_t(), _i()
        self.ctx._ck(self.ctx.lib.ltm_fpfh_info(self.ctx.h, self.h, C.byref(a), C.byref(b), C.byref(k)))
        return a.value, b.value, k.value

    def __len__(self):
        return self.info()[0]

    k = property(lambda self: self.info()[2], doc="the k of the call")

    def _device(self):
        po, pd, ps = _vp(), _vp(), _vp()
        self.ctx._ck(self.ctx.lib.ltm_fpfh_device(self.ctx.h, self.h, C.byref(po), C.byref(pd), C.byref(ps)))
        return po.value, pd.value, ps.value

    def _download(self):
        if self._host is None:
            nr = self.info()[0]
            nt, nf = np.empty(nr, np.uint32), np.empty(nr, np.uint32)
            self.ctx._ck(self.ctx.lib.ltm_fpfh_download(self.ctx.h, self.h, nt.ctypes.data, nf.ctypes.data, None, None))
            self._host = (nt, nf)
        return self._host

    n_target = property(lambda self: self._download()[0], doc="uint32 [n_records]: target points of the record's index")
    n_finite = property(lambda self: self._download()[1], doc="uint32 [n_records]: finite ones among them")

    def offsets(self):
        """uint64 [n_records + 1]: record r owns rows [offsets[r], offsets[r + 1])"""
        return self._out(self._device()[0], self.info()[0] + 1, np.uint64, False)

    def descriptors(self, as_torch=False):
        """float32 [n_points, 33] (a copy): alpha, phi and theta histograms, each summing to 100; NaN rows for non-finite points and points without a normal"""
        n = self.info()[1]
        return self._out(self._device()[1], n * FPFH_SIZE, np.float32, as_torch).reshape(n, FPFH_SIZE)

    def device_view(self):
        """the descriptor block itself as a torch tensor [n_points, 33] on the context's device, WITHOUT a copy (torch.cdist and the like work on it): valid
        until close(); the work queued on the context's stream is waited for first"""
        import torch
        n = self.info()[1]
        if not n:
            return torch.empty((0, FPFH_SIZE), dtype=torch.float32, device=f"cuda:{self.ctx.device}")
        self.ctx.synchronize()
        return torch.as_tensor(_DeviceBlock(self, self._device()[1], (n, FPFH_SIZE), "<f4"), device=f"cuda:{self.ctx.device}")

    def spfh_counts(self):
        """uint8 [n_points, 33]: the SPFH counts of every point, unpacked (ltm_fpfh_download)"""
        n = self.info()[1]
        out = np.zeros((n, FPFH_SIZE), np.uint8)
        self.ctx._ck(self.ctx.lib.ltm_fpfh_download(self.ctx.h, self.h, None, None, None, out.ctypes.data))
        return out


MATCH_MAX_KC = 16


def match_tile_rows():
    """ltm_match_tile_rows: the target rows the match kernel stages at a time (needs no device)"""
    return int(load_library().ltm_match_tile_rows())


class Matches(_PtrHandle):
    """ltm_matches: the feature-space correspondences of ltm_fpfh_match, one record per pair (semantics in include/ltm.h, "fpfh matches").  The rows hold
    the pairs' source rows one after the other; offsets() says where each pair's begin."""

    _free = "ltm_matches_free"

    def info(self):
        """(pairs, source rows, kc)"""
        a, b, k = C.c_size_t(), C.c_size_t(), _i()
        self.ctx._ck(self.ctx.lib.ltm_matches_info(self.ctx.h, self.h, C.byref(a), C.byref(b), C.byref(k)))
        return a.value, b.value, k.value

    def __len__(self):
        return self.info()[0]

    kc = property(lambda self: self.info()[2], doc="the kc of the call")

    def _device(self):
        po, pi, pd = _vp(), _vp(), _vp()
        self.ctx._ck(self.ctx.lib.ltm_matches_device(self.ctx.h, self.h, C.byref(po), C.byref(pi), C.byref(pd)))
        return po.value, pi.value, pd.value

    def _download(self):
        if self._host is None:
            nr = self.info()[0]
            ns, nt = np.empty(nr, np.uint32), np.empty(nr, np.uint32)
            self.ctx._ck(self.ctx.lib.ltm_matches_download(self.ctx.h, self.h, ns.ctypes.data, nt.ctypes.data, None, None))
            self._host = (ns, nt)
        return self._host

    n_source = property(lambda self: self._download()[0], doc="uint32 [n_pairs]: rows of the pair's source record")
    n_target = property(lambda self: self._download()[1], doc="uint32 [n_pairs]: rows of the pair's target record")

    def offsets(self):
        """uint64 [n_pairs + 1]: pair i owns rows [offsets[i], offsets[i + 1])"""
        return self._out(self._device()[0], self.info()[0] + 1, np.uint64, False)

    def indices(self, as_torch=False):
        """int32 [n_rows, kc] (a copy): target rows within the pair's target record, ascending by (distance, row); -1 in unused slots"""
        _, n, k = self.info()
        return self._out(self._device()[1], n * k, np.int32, as_torch).reshape(n, k)

    def distances(self, as_torch=False):
        """float32 [n_rows, kc] (a copy): squared descriptor distances; +inf in unused slots"""
        _, n, k = self.info()
        return self._out(self._device()[2], n * k, np.float32, as_torch).reshape(n, k)


SAC_STATS = ("inlier_tests", "prerejected", "early_hits", "records")
SAC_MAX_ITERATIONS = 16384


def sac_block_points():
    """ltm_sac_block_points: the voting points a workgroup of the vote kernel takes (needs no device)"""
    return int(load_library().ltm_sac_block_points())


def sac_params(inlier_distance=None, max_iterations=None, seed=None, similarity_threshold=None, inlier_fraction=None, eval_stride=None):
    """ltm_sac_params from the library's defaults, checked: inlier_distance finite and > 0 (it has no usable default), 1 <= max_iterations <= 16384,
    0 <= seed < 2^32, similarity_threshold in [0, 1), inlier_fraction in [0, 1], 1 <= eval_stride < 2^32"""
    p = SacParams()
    load_library().ltm_sac_default_params(C.byref(p))
    if inlier_distance is None:
        raise ValueError("inlier_distance must be given")
    p.inlier_distance = float(inlier_distance)
    if not (np.isfinite(p.inlier_distance) and p.inlier_distance > 0.0):
        raise ValueError("inlier_distance must be finite and > 0")
    for name, value, lo, hi in (("max_iterations", max_iterations, 1, SAC_MAX_ITERATIONS), ("seed", seed, 0, 2 ** 32 - 1),
                                ("eval_stride", eval_stride, 1, 2 ** 32 - 1)):
        if value is not None:
            if int(value) != value or not lo <= int(value) <= hi:
                raise ValueError(f"need {lo} <= {name} <= {hi}")
            setattr(p, name, int(value))
    if similarity_threshold is not None:
        p.similarity_threshold = float(similarity_threshold)
    if inlier_fraction is not None:
        p.inlier_fraction = float(inlier_fraction)
    if not 0.0 <= p.similarity_threshold < 1.0:
        raise ValueError("similarity_threshold must be in [0, 1)")
    if not 0.0 <= p.inlier_fraction <= 1.0:
        raise ValueError("inlier_fraction must be in [0, 1]")
    return p


class SacAlignments(_PtrHandle):
    """ltm_sac: the initial alignments of ltm_sac_align, one record per pair (semantics in include/ltm.h, "initial alignment")"""

    _free = "ltm_sac_free"

    def info(self):
        """(pairs, max_iterations)"""
        a, m = C.c_size_t(), C.c_uint32()
        self.ctx._ck(self.ctx.lib.ltm_sac_info(self.ctx.h, self.h, C.byref(a), C.byref(m)))
        return a.value, m.value

    def __len__(self):
        return self.info()[0]

    def _device(self):
        pc, pv = _vp(), _vp()
        self.ctx._ck(self.ctx.lib.ltm_sac_device(self.ctx.h, self.h, C.byref(pc), C.byref(pv)))
        return pc.value, pv.value

    def _download(self):
        if self._host is None:
            nr = self.info()[0]
            found, best = np.empty(nr, np.uint8), np.empty(nr, np.int32)
            cons, nv, npre, ne = (np.empty(nr, np.uint32) for _ in range(4))
            T = np.empty((nr, 4, 4), np.float64)
            self.ctx._ck(self.ctx.lib.ltm_sac_download(self.ctx.h, self.h, found.ctypes.data, best.ctypes.data, cons.ctypes.data, nv.ctypes.data, npre.ctypes.data,
                                                       ne.ctypes.data, T.ctypes.data, None, None))
            self._host = (found, best, cons, nv, npre, ne, T)
        return self._host

    found = property(lambda self: self._download()[0], doc="uint8 [n_pairs]: 1 = the consensus passes the inlier-fraction gate")
    best = property(lambda self: self._download()[1], doc="int32 [n_pairs]: the best hypothesis, -1 = no valid one")
    consensus = property(lambda self: self._download()[2], doc="uint32 [n_pairs]: inliers of the best hypothesis")
    n_valid = property(lambda self: self._download()[3], doc="uint32 [n_pairs]: valid hypotheses")
    n_prerejected = property(lambda self: self._download()[4], doc="uint32 [n_pairs]: hypotheses the polygon test rejected")
    n_eval = property(lambda self: self._download()[5], doc="uint32 [n_pairs]: voting points")
    T = property(lambda self: self._download()[6], doc="float64 [n_pairs, 4, 4]: source -> target of the best hypothesis (NaN: none): the init of icp_align")

    def hypothesis_counts(self):
        """uint32 [n_pairs, max_iterations]: the inlier count of every hypothesis, 0 where invalid"""
        nr, m = self.info()
        return self._out(self._device()[0], nr * m, np.uint32, False).reshape(nr, m)

    def hypothesis_valid(self):
        """uint8 [n_pairs, max_iterations]"""
        nr, m = self.info()
        return self._out(self._device()[1], nr * m, np.uint8, False).reshape(nr, m)



class Outliers(_PtrHandle):
    """ltm_outliers: the labels of a statistical or radius outlier filter, one record per listed search index (semantics in include/ltm.h, "outlier
    filters").  The per-position arrays hold the records one after the other, each in its target's ORIGINAL order; offsets() says where each begins."""

    _free = "ltm_outliers_free"

    def info(self):
        """(kind, records, positions)"""
        k, a, b = _i(), C.c_size_t(), C.c_size_t()
        self.ctx._ck(self.ctx.lib.ltm_outliers_info(self.ctx.h, self.h, C.byref(k), C.byref(a), C.byref(b)))
        return k.value, a.value, b.value

    def __len__(self):
        return self.info()[1]

    kind = property(lambda self: ("statistical", "radius")[self.info()[0]])

    def _device(self):
        po, pl, pd, pc = _vp(), _vp(), _vp(), _vp()
        self.ctx._ck(self.ctx.lib.ltm_outliers_device(self.ctx.h, self.h, C.byref(po), C.byref(pl), C.byref(pd), C.byref(pc)))
        return po.value, pl.value, pd.value, pc.value

    def _download(self):
        if self._host is None:
            kind, nr, _ = self.info()
            nt, nf, nk = np.empty(nr, np.uint32), np.empty(nr, np.uint32), np.empty(nr, np.uint32)
            mean, sd, thr = np.zeros(nr, np.float64), np.zeros(nr, np.float64), np.zeros(nr, np.float64)
            stats = (mean.ctypes.data, sd.ctypes.data, thr.ctypes.data) if kind == OUTLIERS_STATISTICAL else (None, None, None)
            self.ctx._ck(self.ctx.lib.ltm_outliers_download(self.ctx.h, self.h, nt.ctypes.data, nf.ctypes.data, nk.ctypes.data, *stats, None, None, None))
            self._host = (nt, nf, nk, mean, sd, thr)
        return self._host

    n_target = property(lambda self: self._download()[0], doc="uint32 [n_records]: target points of the record's index")
    n_finite = property(lambda self: self._download()[1], doc="uint32 [n_records]: finite ones among them")
    n_kept = property(lambda self: self._download()[2], doc="uint32 [n_records]: labels set")
    mean = property(lambda self: self._download()[3], doc="float64 [n_records]: mean of the distances (statistical; zeros for a radius set)")
    stddev = property(lambda self: self._download()[4], doc="float64 [n_records]")
    threshold = property(lambda self: self._download()[5], doc="float64 [n_records]: mean + stddev_mul * stddev")

    def offsets(self):
        """uint64 [n_records + 1]: record r owns positions [offsets[r], offsets[r + 1]) of labels / distances / counts"""
        return self._out(self._device()[0], self.info()[1] + 1, np.uint64, False)

    def labels(self, as_torch=False):
        """uint8 [n_points]: 1 = kept"""
        return self._out(self._device()[1], self.info()[2], np.uint8, as_torch)

    def distances(self, as_torch=False):
        """float32 [n_points]: the mean neighbour distance of every position, 0 for a non-finite point (statistical sets only)"""
        if self.info()[0] != OUTLIERS_STATISTICAL:
            raise ValueError("a radius outlier set has no distances")
        return self._out(self._device()[2], self.info()[2], np.float32, as_torch)

    def counts(self):
        """uint32 [n_points]: neighbours within the radius, the point included, saturated at min_neighbors (radius sets only)"""
        if self.info()[0] != OUTLIERS_RADIUS:
            raise ValueError("a statistical outlier set has no counts")
        return self._out(self._device()[3], self.info()[2], np.uint32, False)

    def split(self, scans_or_cloud):
        """ltm_outliers_split_scanset / _cloud: (kept, removed) of a ScanSet with one keyframe per record, or of the Cloud (or array) of a one-record
        set; input order kept on both sides"""
        a, b = _u64(), _u64()
        if isinstance(scans_or_cloud, ScanSet):
            self.ctx._ck(self.ctx.lib.ltm_outliers_split_scanset(self.ctx.h, self.h, scans_or_cloud.h, C.byref(a), C.byref(b)))
            return ScanSet(self.ctx, a.value), ScanSet(self.ctx, b.value)
        cloud = scans_or_cloud if isinstance(scans_or_cloud, Cloud) else self.ctx.upload(_xyzi(scans_or_cloud))
        self.ctx._ck(self.ctx.lib.ltm_outliers_split_cloud(self.ctx.h, self.h, cloud.h, C.byref(a), C.byref(b)))
        return Cloud(self.ctx, a.value), Cloud(self.ctx, b.value)



class ScanContexts(_PtrHandle):
    """ltm_sc: N device-resident Scan Context descriptors with their ring and sector keys (semantics in include/ltm.h, "scan context").  The
    parameters it was made with are the defaults of distance() / detect(); keyword arguments replace single fields for one call."""

    _free = "ltm_sc_free"

    def __init__(self, ctx, h, params):
        self.ctx, self.h, self.params = ctx, h, params

    def _params(self, over):
        p = ScParams.from_buffer_copy(self.params)
        for k, v in over.items():
            if k not in dict(ScParams._fields_):
                raise TypeError(f"ltm_sc_params has no field {k!r}")
            setattr(p, k, v)
        return p

    def info(self):
        """(descriptors, num_ring, num_sector)"""
        n, r, s = C.c_size_t(), _i(), _i()
        self.ctx._ck(self.ctx.lib.ltm_sc_info(self.ctx.h, self.h, C.byref(n), C.byref(r), C.byref(s)))
        return n.value, r.value, s.value

    def __len__(self):
        return self.info()[0]

    def download(self):
        """(descriptors float64 [n, ring, sector], ring keys float32 [n, ring], sector keys float64 [n, sector])"""
        n, r, s = self.info()
        desc, rk, sk = np.empty((n, r, s), np.float64), np.empty((n, r), np.float32), np.empty((n, s), np.float64)
        self.ctx._ck(self.ctx.lib.ltm_sc_download(self.ctx.h, self.h, desc.ctypes.data, rk.ctypes.data, sk.ctypes.data))
        return desc, rk, sk

    def distance(self, other, pairs, **params):
        """distanceBtnScanContext(self[i], other[j]) for every row (i, j) of `pairs`: (dist float64 [n], shift int32 [n])"""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        p = self._params(params)
        dist, shift = np.empty(len(pr), np.float64), np.empty(len(pr), np.int32)
        self.ctx._ck(self.ctx.lib.ltm_sc_distance(self.ctx.h, self.h, other.h, pr.ctypes.data, len(pr), C.byref(p), dist.ctypes.data, shift.ctypes.data))
        return dist, shift

    def detect(self, queries, **params):
        """detectLoopClosureIDBetweenSession of every descriptor of `queries` against this set (the database): dict of arrays with one entry per
        query -- loop_id, nn_idx, nn_align (int32), min_dist (float64), yaw_diff_rad (float32)"""
        p = self._params(params)
        n = len(queries)
        out = {"loop_id": np.empty(n, np.int32), "nn_idx": np.empty(n, np.int32), "min_dist": np.empty(n, np.float64),
               "nn_align": np.empty(n, np.int32), "yaw_diff_rad": np.empty(n, np.float32)}
        self.ctx._ck(self.ctx.lib.ltm_sc_detect(self.ctx.h, self.h, queries.h, C.byref(p), *[out[k].ctypes.data for k in
                                                                                             ("loop_id", "nn_idx", "min_dist", "nn_align", "yaw_diff_rad")]))
        return out



class VgsTicket:
    """an open ltm_voxel_grid_scanset_begin: end() finishes the grid; a ticket dropped without it (an exception between the halves) is ended and its result
    freed when the object goes (and ltm_destroy joins whatever is still open), so the coordinator thread never outlives its buffers"""

    def __init__(self, ctx, t, scans):
        self.ctx, self.t, self.scans = ctx, t, scans

    def end(self):
        t, self.t = self.t, None
        if t is None:
            raise LtmError(-1, "the ticket was ended already")
        out = _u64()
        self.ctx._ck(self.ctx.lib.ltm_voxel_grid_scanset_end(self.ctx.h, t, C.byref(out)))
        self.scans = None
        return ScanSet(self.ctx, out.value)

    def __del__(self):
        try:
            if self.t is not None and self.ctx.h:
                self.end().free()
        except Exception:
            pass


class Event:
    """ltm_event: a point of one context's stream that other contexts can wait for (any number of times)"""

    def __init__(self, lib, h):
        self.lib, self.h = lib, h

    def __del__(self):
        try:
            if self.h:
                self.lib.ltm_event_destroy(self.h)
                self.h = None
        except Exception:
            pass


class _Handle:
    _free = None

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def free(self):
        if self.h and self.ctx.h:
            getattr(self.ctx.lib, self._free)(self.ctx.h, self.h)
        self.h = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Cloud(_Handle):
    _free = "ltm_cloud_free"

    def __len__(self):
        n = C.c_size_t()
        self.ctx._ck(self.ctx.lib.ltm_cloud_size(self.ctx.h, self.h, C.byref(n)))
        return n.value

    def download(self):
        n = len(self)
        out = np.empty((n, 4), dtype=np.float32)
        self.ctx._ck(self.ctx.lib.ltm_cloud_download(self.ctx.h, self.h, out.ctypes.data, n, 16))
        return out

    def clone(self):
        out = _u64()
        self.ctx._ck(self.ctx.lib.ltm_cloud_clone(self.ctx.h, self.h, C.byref(out)))
        return Cloud(self.ctx, out.value)

    def device_ptr(self):
        p = _vp()
        self.ctx._ck(self.ctx.lib.ltm_cloud_device_ptr(self.ctx.h, self.h, C.byref(p)))
        return p.value


class ScanSet(_Handle):
    _free = "ltm_scanset_free"

    def info(self):
        a, b = C.c_size_t(), C.c_size_t()
        self.ctx._ck(self.ctx.lib.ltm_scanset_info(self.ctx.h, self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @property
    def n_kf(self):
        return self.info()[0]

    def offsets(self):
        nk, _ = self.info()
        off = np.empty(nk + 1, dtype=np.uint64)
        self.ctx._ck(self.ctx.lib.ltm_scanset_offsets(self.ctx.h, self.h, off.ctypes.data_as(_pu64)))
        return off

    def download(self):
        _, n = self.info()
        out = np.empty((n, 4), dtype=np.float32)
        self.ctx._ck(self.ctx.lib.ltm_scanset_download(self.ctx.h, self.h, out.ctypes.data, n, 16))
        return out, self.offsets()

    def as_cloud(self):
        out = _u64()
        self.ctx._ck(self.ctx.lib.ltm_scanset_as_cloud(self.ctx.h, self.h, C.byref(out)))
        return Cloud(self.ctx, out.value)

    def device_ptr(self):
        p = _vp()
        self.ctx._ck(self.ctx.lib.ltm_scanset_device_ptr(self.ctx.h, self.h, C.byref(p)))
        return p.value


class Poses(_Handle):
    _free = "ltm_poses_free"

    def __init__(self, ctx, h, n, host_poses=None, host_inv=None):
        super().__init__(ctx, h)
        self.n = n
        self.host_poses, self.host_inv = host_poses, host_inv     # kept so that keyframe shards can be sliced off
