"""orb_slam3_fast_amd — MI355X-native ORB front-end (extract + match) behind the reference's API surface.

Host-side mirror (Python, over the C ABI of include/orbx.h) of the reference's
`ORB_SLAM3::ORBextractor` (include/ORBextractor.h:49-118, src/ORBextractor.cc) and the matching routines
of `ORB_SLAM3::ORBmatcher` / `Frame` that are on the hot path (src/ORBmatcher.cc:618-764,1920-1973,
src/Frame.cc:921-1084,1273-1304).  Same names, argument meaning and error behaviour; all compute runs in
the hand-written HIP kernels of liborbx.so.  There is NO CPU fallback: importing works anywhere, but every
compute call raises if the library or a GPU is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("ORBX_LIB_NAME", "liborbx.so"))   # ORBX_LIB_NAME: A/B runs of experiment builds (tools)

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28  # cv::KeyPoint

OK, E_EMPTY, E_BADARG, E_CAPACITY, E_HIP, E_NODEVICE, E_UNSUPPORTED, E_TIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30  # src/ORBmatcher.cc:35-37
NUM_STAGES = 8
MP_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("track_depth", "<f4"),
                     ("predicted_level", "<i4"), ("in_view", "u1"), ("bad", "u1"), ("has_observations", "u1"),
                     ("pad_", "u1"), ("desc", "u1", (32,))])   # orbx_map_point_view
assert MP_DTYPE.itemsize == 60
PP_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("radius", "<f4"), ("angle", "<f4"), ("min_level", "<i4"),
                     ("max_level", "<i4"), ("valid", "u1"), ("has_observations", "u1"), ("pad_", "u1", (2,)),
                     ("desc", "u1", (32,))])   # orbx_projected_point
assert PP_DTYPE.itemsize == 64
FP_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("radius", "<f4"), ("predicted_level", "<i4"), ("valid", "u1"),
                     ("pad_", "u1", (3,)), ("desc", "u1", (32,))])   # orbx_fuse_point
assert FP_DTYPE.itemsize == 56
TRI_RIG_DTYPE = np.dtype([("cam", "<f4", (4, 8)), ("precision", "<f4"), ("R", "<f4", (4, 9)), ("t", "<f4", (4, 3))])   # orbx_tri_rig
assert TRI_RIG_DTYPE.itemsize == 324
MPR_DTYPE = np.dtype([("proj_yr", "<f4"), ("view_cos_r", "<f4"), ("predicted_level_r", "<i4"), ("in_view_r", "u1"),
                      ("pad_", "u1", (3,))])   # orbx_map_point_right
assert MPR_DTYPE.itemsize == 16
POSE_DTYPE = np.dtype([("q", "<f4", 4), ("t", "<f4", 3), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                       ("bf", "<f4")])   # orbx_pose_opt_frame
assert POSE_DTYPE.itemsize == 48
POSE_KB8_DTYPE = np.dtype([("q", "<f4", 4), ("t", "<f4", 3), ("kb8_left", "<f4", 8), ("kb8_right", "<f4", 8), ("trl_q", "<f4", 4),
                           ("trl_t", "<f4", 3)])   # orbx_pose_opt_frame_kb8
assert POSE_KB8_DTYPE.itemsize == 120


class OrbxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("orbx error %d: %s" % (code, msg))
        self.code = code


class _Params(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


class _PreprocParams(C.Structure):
    _fields_ = [("src_w", C.c_int32), ("src_h", C.c_int32), ("channels", C.c_int32), ("rgb_order", C.c_int32),
                ("out_w", C.c_int32), ("out_h", C.c_int32), ("map_x", C.c_void_p), ("map_y", C.c_void_p),
                ("map_stride", C.c_ssize_t), ("n_maps", C.c_int32), ("clahe_clip_limit", C.c_double),
                ("clahe_tiles_x", C.c_int32), ("clahe_tiles_y", C.c_int32)]


_lib = None


def lib():
    """Load liborbx.so (built by __graft_entry__.build() / csrc/Makefile).  Fails loudly when absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("liborbx.so not built (%s): run `python -c 'import __graft_entry__ as g; "
                              "g.build()'` — there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.orbx_last_error.restype = C.c_char_p
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.orbx_extractor_create.argtypes = [C.POINTER(_Params), i, i, i, i, C.POINTER(vp)]
        L.orbx_extractor_destroy.argtypes = [vp]
        L.orbx_get_tables.argtypes = [vp] + [vp] * 6
        L.orbx_extract.argtypes = [vp, vp, i, i, C.c_ssize_t, i, i, vp, vp, i, C.POINTER(i)]
        L.orbx_extract_batch_device.argtypes = [vp, vp, i, i, i, C.c_ssize_t, C.c_ssize_t, vp]
        L.orbx_sync.argtypes = [vp]
        L.orbx_stream_handle.argtypes = [vp, C.POINTER(vp)]
        L.orbx_extract_batch.argtypes = [vp, vp, i, i, i, C.c_ssize_t, C.c_ssize_t, vp]
        L.orbx_batch_download_async.argtypes = [vp, vp, vp, vp, vp, vp, vp, i]
        L.orbx_extract_stereo.argtypes = [vp, vp, vp, i, i, C.c_ssize_t, C.c_ssize_t, vp, vp, vp, vp, i, vp, vp, vp, vp, i, vp, vp, f, f, vp, vp]
        L.orbx_batch_results_device.argtypes = [vp] + [C.POINTER(vp)] * 4 + [C.POINTER(i)]
        L.orbx_batch_download.argtypes = [vp, i, vp, vp, i, C.POINTER(i)]
        L.orbx_pyramid_level.argtypes = [vp, i, i, i, vp, C.c_ssize_t, C.POINTER(i), C.POINTER(i)]
        L.orbx_pyramid_download.argtypes = [vp, i, i, vp, vp]
        L.orbx_host_results.argtypes = [vp, i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i), C.POINTER(i), C.POINTER(vp), C.POINTER(vp)]
        L.orbx_set_host_pyramid.argtypes = [vp, i]
        L.orbx_host_pyramid_level.argtypes = [vp, i, i, C.POINTER(vp), C.POINTER(i), C.POINTER(i), C.POINTER(C.c_ssize_t)]
        L.orbx_debug_candidates.argtypes = [vp, i, i, vp, i]
        L.orbx_hamming256.argtypes = [vp, vp]
        L.orbx_stereo_match_batch.argtypes = [vp, i, vp, i, i, f, f]
        L.orbx_stereo_results_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.orbx_stereo_download.argtypes = [vp, i, vp, vp, i]
        L.orbx_rgbd_depth_batch.argtypes = [vp, i, i, vp, i, C.c_ssize_t, C.c_ssize_t, f, f, vp, vp, i, vp]
        L.orbx_pose_optimization.argtypes = [i, vp, vp, vp, vp, i, vp, i, vp, vp]
        L.orbx_merge_bundle_adjustment.argtypes = [i, vp, vp, vp]
        L.orbx_merge_bundle_adjustment_rig.argtypes = [i, vp, vp, vp]
        L.orbx_merge_ba_stop_after_first.argtypes = [i]
        L.orbx_pose_optimization_batch.argtypes = [vp, i, i, i, vp, vp, vp, vp, vp, vp]
        L.orbx_pose_optimization_kb8.argtypes = [i, vp, i, i, vp, vp, vp, i, vp, vp]
        L.orbx_pose_optimization_fisheye_batch.argtypes = [vp, i, i, i, vp, vp, vp, vp, vp, vp]
        L.orbx_reconstruct_two_views.argtypes = [i, vp, i, vp, i, vp, vp, vp, vp, vp, vp, vp]
        L.orbx_reconstruct_two_views_batch.argtypes = [vp, i, i, vp, vp, i, vp, vp, vp, vp, vp, vp, vp]
        L.orbx_mlpnp_ransac_parameters.argtypes = [i, C.c_double, i, i, i, f, vp, vp, vp]
        L.orbx_mlpnp_iterate.argtypes = [i, vp, i, i, vp, vp, vp, i, vp, vp, i, vp, vp, vp, vp, vp]
        L.orbx_mlpnp_iterate_batch.argtypes = [vp, i, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp]
        L.orbx_sim3_ransac_parameters.argtypes = [i, C.c_double, i, i, vp]
        L.orbx_sim3_iterate.argtypes = [i, i, vp, vp, vp, vp, vp, vp, vp, vp, i, vp, i, vp, vp, i, vp, vp, vp, vp, vp]
        L.orbx_sim3_iterate_batch.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp, i, vp, vp, i, vp, vp, vp, vp, vp]
        L.orbx_optimize_sim3.argtypes = [i, i, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, i, vp, i, vp, vp, vp]
        L.orbx_optimize_sim3_batch.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, vp, i, vp, vp, vp]
        L.orbx_local_bundle_adjustment.argtypes = [i, vp, vp, vp]
        L.orbx_triangulate_matches.argtypes = [i, vp, vp, vp, vp, vp, vp, vp]
        L.orbx_create_new_map_points.argtypes = [i, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orbx_extract_rgbd.argtypes = [vp, vp, i, i, C.c_ssize_t, vp, i, C.c_ssize_t, f, f, vp, vp, i, vp, vp, i, C.POINTER(i),
                                        C.POINTER(i), vp, vp, vp]
        L.orbx_bf_knn2.argtypes = [i, vp, i, vp, i, vp, vp, vp]
        L.orbx_fisheye_stereo_match.argtypes = [i, vp, vp, i, i, vp, vp, i, i, vp, vp, i, vp, vp, vp, vp, vp]
        L.orbx_fisheye_stereo_match_batch.argtypes = [vp, i, vp, i, i, vp]
        L.orbx_undistort_keypoints.argtypes = [i, vp, i, vp, vp, i, vp]
        L.orbx_cvt_gray.argtypes = [i, vp, i, i, C.c_ssize_t, i, i, vp, C.c_ssize_t]
        L.orbx_resize_linear.argtypes = [i, vp, i, i, C.c_ssize_t, i, vp, i, i, C.c_ssize_t]
        L.orbx_remap_linear.argtypes = [i, vp, i, i, C.c_ssize_t, i, vp, vp, C.c_ssize_t, vp, i, i, C.c_ssize_t]
        L.orbx_clahe.argtypes = [i, vp, i, i, C.c_ssize_t, C.c_double, i, i, vp, C.c_ssize_t]
        L.orbx_preproc_create.argtypes = [C.POINTER(_PreprocParams), i, i, C.POINTER(vp)]
        L.orbx_preproc_destroy.argtypes = [vp]
        L.orbx_preproc_destroy.restype = None
        L.orbx_preproc_output_size.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
        L.orbx_preproc_run.argtypes = [vp, vp, C.c_ssize_t, i, vp, C.c_ssize_t]
        L.orbx_preproc_run_device.argtypes = [vp, vp, i, C.c_ssize_t, C.c_ssize_t, C.POINTER(vp), C.POINTER(i), C.POINTER(i),
                                              C.POINTER(C.c_ssize_t), C.POINTER(C.c_ssize_t)]
        L.orbx_extract_batch_raw_device.argtypes = [vp, vp, vp, i, C.c_ssize_t, C.c_ssize_t, vp]
        L.orbx_vocabulary_create.argtypes = [i, i, i, i, i, i, vp, vp, vp, vp, C.POINTER(vp)]
        L.orbx_vocabulary_load_text.argtypes = [i, C.c_char_p, C.POINTER(vp)]
        L.orbx_vocabulary_destroy.argtypes = [vp]
        L.orbx_vocabulary_destroy.restype = None
        L.orbx_vocabulary_info.argtypes = [vp, vp]
        L.orbx_bow_transform.argtypes = [vp, vp, i, i, vp, vp, C.POINTER(i), vp, vp, vp, C.POINTER(i)]
        L.orbx_bow_transform_batch.argtypes = [vp, vp, i]
        L.orbx_bow_results_device.argtypes = [vp] + [C.POINTER(vp)] * 6 + [C.POINTER(i)]
        L.orbx_bow_download.argtypes = [vp, i, vp, vp, C.POINTER(i), vp, vp, vp, C.POINTER(i), i]
        L.orbx_kfdb_create.argtypes = [vp, i, i, C.POINTER(vp)]
        L.orbx_kfdb_create_sized.argtypes = [i, i, i, i, i, C.POINTER(vp)]
        L.orbx_kfdb_destroy.argtypes = [vp]
        L.orbx_kfdb_destroy.restype = None
        L.orbx_kfdb_size.argtypes = [vp]
        L.orbx_kfdb_profile.argtypes = [vp, i, C.POINTER(f)]
        L.orbx_kfdb_add.argtypes = [vp, i, i, vp, vp, i]
        L.orbx_kfdb_add_from_batch.argtypes = [vp, vp, i, i, i]
        L.orbx_kfdb_erase.argtypes = [vp, i]
        L.orbx_kfdb_clear.argtypes = [vp]
        L.orbx_kfdb_clear_map.argtypes = [vp, i]
        L.orbx_kfdb_set_covisibles.argtypes = [vp, i, vp, vp]
        L.orbx_kfdb_detect_relocalization_candidates.argtypes = [vp, vp, vp, i, i, vp, i, C.POINTER(i), vp]
        L.orbx_kfdb_detect_relocalization_candidates_batch.argtypes = [vp, vp, i, i, vp, vp, i, vp, vp]
        L.orbx_kfdb_detect_n_best_candidates.argtypes = [vp, vp, vp, i, i, vp, i, vp, i, i, vp, C.POINTER(i), vp, C.POINTER(i), vp]
        L.orbx_search_by_bow.argtypes = [i, vp, vp, vp, i, vp, vp, vp, i, vp, vp, vp, i, vp, vp, i, i, f, i, vp]
        L.orbx_search_by_projection_fisheye_batch.argtypes = [vp, i, i, i, f, f, f, f, vp, vp, vp, i, f, i, f, f, vp, vp, vp, vp, vp, vp]
        L.orbx_search_by_projection_frame_fisheye_batch.argtypes = [vp, i, i, i, f, f, f, f, vp, vp, vp, i, i, vp, vp, vp, vp]
        L.orbx_search_by_bow_batch.argtypes = [vp, i, i, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, f, i, vp, vp]
        L.orbx_search_by_projection_fisheye.argtypes = [i, vp, vp, i, i, f, f, f, f, vp, i, vp, vp, i, f, i, f, f, vp, vp, vp, vp]
        L.orbx_search_by_projection_frame_fisheye.argtypes = [i, vp, vp, i, i, f, f, f, f, vp, vp, i, i, vp, vp]
        L.orbx_compute_image_bounds.argtypes = [i, i, i, vp, vp, i, vp]
        L.orbx_fisheye_results_device.argtypes = [vp, vp, vp, vp, vp, vp]
        L.orbx_fisheye_download.argtypes = [vp, i, vp, vp, vp, vp, i, i, vp]
        L.orbx_search_for_initialization.argtypes = [i, vp, vp, i, vp, vp, i, f, f, f, f, vp, vp, i, f, i]
        L.orbx_search_for_initialization_batch.argtypes = [vp, i, i, vp, vp, vp, i, f, f, f, f, vp, vp, i, f, i, vp]
        L.orbx_search_by_projection.argtypes = [i, vp, vp, vp, i, f, f, f, f, vp, i, vp, i, f, i, f, f, vp, vp]
        L.orbx_search_by_projection_frame.argtypes = [i, vp, vp, vp, i, f, f, f, f, vp, i, i, vp, vp]
        L.orbx_search_by_projection_frame_batch.argtypes = [vp, i, i, f, f, f, f, vp, vp, i, i, i, vp, vp, vp, vp]
        L.orbx_search_by_projection_batch.argtypes = [vp, i, i, f, f, f, f, vp, vp, i, f, i, f, f, i, vp, vp, vp, vp]
        L.orbx_search_by_projection_keyframe.argtypes = [i, vp, vp, i, f, f, f, f, vp, i, i, i, vp, vp]
        L.orbx_map_upload.argtypes = [vp, i, vp, vp, vp, vp, vp, vp]
        L.orbx_project_map_points_batch.argtypes = [vp, i, vp, f, f, f, f, f, vp, vp]
        L.orbx_last_frames_upload.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp]
        L.orbx_project_map_points_fisheye_batch.argtypes = [vp, i, vp, vp, f, f, f, f, f, vp, vp, vp]
        L.orbx_project_last_frames_batch.argtypes = [vp, i, vp, f, f, f, f, f, vp]
        L.orbx_search_for_triangulation.argtypes = [i, vp, vp, vp, i, vp, vp, vp, vp, i, vp, vp, vp, i, vp, vp, vp, vp, i, vp, vp, i,
                                                    vp, vp, i, i, i, vp]
        L.orbx_search_for_triangulation_rig.argtypes = [i, vp, vp, vp, i, vp, vp, vp, i, i, vp, vp, vp, i, vp, vp, vp, i, i, vp, vp, i, vp,
                                                        i, i, i, vp]
        L.orbx_search_by_bow_keyframes.argtypes = [i, vp, vp, vp, i, vp, vp, vp, i, vp, vp, vp, i, vp, vp, vp, i, f, i, vp]
        L.orbx_fuse_search.argtypes = [i, vp, vp, vp, i, f, f, f, f, vp, i, vp, i, i, vp, vp]
        L.orbx_features_in_area.argtypes = [i, vp, i, f, f, f, f, vp, i, vp, vp, i, vp, vp]
        L.orbx_comm_unique_id.argtypes = [vp]
        L.orbx_comm_create.argtypes = [vp, i, i, i, C.POINTER(vp)]
        L.orbx_comm_adopt.argtypes = [vp, i, C.POINTER(vp)]
        L.orbx_comm_destroy.argtypes = [vp]
        L.orbx_comm_destroy.restype = None
        L.orbx_comm_size.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
        L.orbx_allgather_descriptors.argtypes = [vp, vp, i, vp, vp]
        L.orbx_comm_wait.argtypes = [vp, i, C.POINTER(C.c_ulonglong)]
        L.orbx_clock_probe_start.argtypes = [i, i, C.POINTER(vp)]
        L.orbx_clock_probe_finish.argtypes = [vp, C.POINTER(C.c_double)]
        L.orbx_copy_probe.argtypes = [i, C.c_size_t, i, C.POINTER(C.c_double)]
        L.orbx_profile_enable.argtypes = [vp, i]
        L.orbx_profile_collect.argtypes = [vp, vp, vp]
        L.orbx_stage_name.restype = C.c_char_p
        L.orbx_stage_name.argtypes = [i]
        L.orbx_level_stats.argtypes = [vp, i, vp, vp, vp, vp]
        L.orbx_debug_introsort.argtypes = [vp, i]
        L.orbx_debug_introsort.restype = None
        L.orbx_debug_introsort_device.argtypes = [i, vp, i]
        if hasattr(L, "orbx_debug_octree"):   # (ORBX_LIB_NAME may name an older build in A/B runs)
            L.orbx_debug_introsort_device_nt.argtypes = [i, vp, i, i]
            L.orbx_debug_octree.argtypes = [vp, i, i, i, vp, vp, vp, vp, i]
            L.orbx_debug_octree_check.argtypes = [vp, i, i, i, vp, vp]
        L.orbx_debug_linalg.argtypes = [i, i, i, vp, vp]
        L.orbx_debug_geometry.argtypes = [i, i, i, vp, vp]
        L.orbx_pose_inertial_optimization_last_keyframe.argtypes = [i, vp, vp, vp, vp, vp, i, vp, i, vp, vp, vp, i, vp, vp]
        L.orbx_pose_inertial_optimization_last_frame.argtypes = [i, vp, vp, vp, vp, vp, i, vp, i, vp, vp, vp, vp, vp, i, vp, vp]
        L.orbx_pose_inertial_optimization_last_keyframe_batch.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp]
        L.orbx_pose_inertial_optimization_last_frame_batch.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp,
                                                                       vp, vp]
        L.orbx_debug_inertial_linalg.argtypes = [i, i, i, vp, vp]
        L.orbx_debug_set_detect_list_cap.argtypes = [i]
        L.orbx_debug_set_detect_list_cap.restype = None
        L.orbx_debug_set_octree_global.argtypes = [i]
        L.orbx_debug_set_octree_global.restype = None
        if hasattr(L, "orbx_debug_set_octree_class"):   # (ORBX_LIB_NAME may name an older build in A/B runs)
            L.orbx_debug_set_octree_class.argtypes = [i]
            L.orbx_debug_set_octree_class.restype = None
            L.orbx_debug_octree_plan.argtypes = [vp, i, i, vp, vp]
        L.orbx_debug_set_stereo_direct.argtypes = [i]
        L.orbx_debug_set_stereo_direct.restype = None
        if hasattr(L, "orbx_debug_stereo_sort"):   # (ORBX_LIB_NAME may name an older build in A/B runs)
            L.orbx_debug_stereo_sort.argtypes = [vp, i, vp, vp, vp, i]
        L.orbx_debug_set_clahe_cell_kernel.argtypes = [i]
        L.orbx_debug_set_clahe_cell_kernel.restype = None
        L.orbx_debug_upload_results.argtypes = [vp, i, vp, vp, i, i]
        L.orbx_debug_set_remap_lds.argtypes = [i]
        L.orbx_debug_set_remap_lds.restype = None
        L.orbx_debug_remap_footprints.argtypes = [vp, vp, C.c_ssize_t, i, i, i, i, i, vp, i, C.POINTER(i), C.POINTER(i)]
        L.orbx_debug_preproc_plan.argtypes = [vp, vp]
        if hasattr(L, "orbx_debug_front_tables"):   # (ORBX_LIB_NAME may name an older build in A/B runs)
            L.orbx_debug_front_tables.argtypes = [vp, i, i, vp, i, vp, i, vp]
        if hasattr(L, "orbx_debug_resize_stream"):   # (ORBX_LIB_NAME may name an older build in A/B runs)
            L.orbx_debug_resize_stream_tables.argtypes = [vp, i, i, i, vp, i, vp]
            L.orbx_debug_resize_stream.argtypes = [vp, vp, i, i, i, C.c_ssize_t, C.c_ssize_t, i, i, i]
        L.orbx_debug_set_resize_tail.argtypes = [i, i, i]
        L.orbx_debug_set_resize_tail.restype = None
        L.orbx_debug_resize_plan.argtypes = [vp, vp, vp, vp, i]
        L.orbx_debug_sincos.argtypes = [i, vp, i, i, vp, vp]
        if hasattr(L, "orbx_debug_fast_atan2"):   # (ORBX_LIB_NAME may name an older build in A/B runs)
            L.orbx_debug_fast_atan2.argtypes = [i, vp, vp, i, vp]
            L.orbx_debug_describe_plan.argtypes = [vp, i, i, i, vp]
        L.orbx_debug_score_map.argtypes = [vp, i]
        L.orbx_set_opencv_compat.argtypes = [vp, i]
        L.orbx_debug_score_level.argtypes = [vp, i, i, vp, C.c_ssize_t]
        L.orbx_debug_scratch_pool.argtypes = [i, i, i, vp]
        L.orbx_debug_fill_work_buffers.argtypes = [vp, i]
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise OrbxError(rc, lib().orbx_last_error().decode())
    return rc


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def device_count():
    return lib().orbx_device_count()


class ORBextractor:
    """Mirror of ORB_SLAM3::ORBextractor (include/ORBextractor.h:49-118).

    `ex(image, lap)` is operator() (src/ORBextractor.cc:1015-1106): returns (monoIndex, keypoints,
    descriptors) with keypoints as a structured array laid out like cv::KeyPoint.  An empty image returns
    (-1, [], []) like the reference.  The batched entry points (`extract_batch_device`) are the
    many-camera mode: independent images of one size through every kernel in one launch each.
    """

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, max_width=1280, max_height=720,
                 max_batch=1, device=0):
        self.nfeatures, self.nlevels = int(nfeatures), int(nlevels)
        self.max_batch = max_batch
        p = _Params(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
        h = C.c_void_p()
        _check(lib().orbx_extractor_create(C.byref(p), max_width, max_height, max_batch, device, C.byref(h)))
        self._h = h
        self.device = device
        L = self.nlevels
        t = [np.zeros(L, np.float32) for _ in range(4)]
        self._nfeat = np.zeros(L, np.int32)
        self._umax = np.zeros(16, np.int32)
        _check(lib().orbx_get_tables(h, _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), _p(self._nfeat), _p(self._umax)))
        self._scale, self._inv_scale, self._sigma2, self._inv_sigma2 = t
        cap = C.c_int()
        _check(lib().orbx_batch_results_device(h, None, None, None, None, C.byref(cap)))
        self.capacity = cap.value

    def close(self):
        if getattr(self, "_h", None):
            lib().orbx_extractor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- getters, include/ORBextractor.h:65-83
    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return float(self._scale[1]) if self.nlevels > 1 else 1.0

    def GetScaleFactors(self):
        return self._scale.copy()

    def GetInverseScaleFactors(self):
        return self._inv_scale.copy()

    def GetScaleSigmaSquares(self):
        return self._sigma2.copy()

    def GetInverseScaleSigmaSquares(self):
        return self._inv_sigma2.copy()

    def features_per_level(self):
        return self._nfeat.copy()

    def umax(self):
        return self._umax.copy()

    # ---- operator()
    def _host_bufs(self):
        """Views of the handle's page-locked result block (orbx_host_results): the single-frame entries are called with NULL
        output arrays and the valid prefix is copied ONCE, byte-wise (numpy copies structured records field by field; with the
        per-call np.zeros of six arrays the wrapper's share of a 1280x720 stereo frame was 80 us)."""
        b = getattr(self, "_hb", None)
        if b is None:
            b = {"n": [C.c_int() for _ in range(4)], "lap": np.zeros(4, np.int32), "views": None}
            b["nref"] = [C.byref(x) for x in b["n"]]
            b["lapp"] = (b["lap"].ctypes.data, b["lap"].ctypes.data + 8)
            self._hb = b
        return b

    def _result_views(self, hb, nimg, stereo):
        """numpy views over the result block (its address is fixed for the life of the handle: a section is mapped the first
        time a call has filled it)."""
        v = hb["views"]
        if v is None:
            v = hb["views"] = {}
        cap = self.capacity
        for img in range(nimg):
            need_st = stereo and img == 0 and "ur" not in v
            if img in v and not need_st:
                continue
            pk, pd, pu, pz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            _check(lib().orbx_host_results(self._h, img, C.byref(pk), C.byref(pd), None, None, C.byref(pu), C.byref(pz)))
            if img not in v:
                kb = np.frombuffer((C.c_uint8 * (cap * 28)).from_address(pk.value), np.uint8).reshape(cap, 28)
                db = np.frombuffer((C.c_uint8 * (cap * 32)).from_address(pd.value), np.uint8).reshape(cap, 32)
                v[img] = (kb, db)
            if need_st:
                v["ur"] = np.frombuffer((C.c_float * cap).from_address(pu.value), np.float32)
                v["dp"] = np.frombuffer((C.c_float * cap).from_address(pz.value), np.float32)
        return v

    @staticmethod
    def _take(view, n):
        return view[0][:n].copy().view(KP_DTYPE).reshape(n), view[1][:n].copy()

    def __call__(self, image, vLappingArea=(0, 0)):
        if image is None or image.size == 0:
            return -1, np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        assert image.dtype == np.uint8 and image.ndim == 2, "CV_8UC1 image expected"
        if image.strides[1] != 1:
            image = np.ascontiguousarray(image)
        h, w = image.shape
        b = self._host_bufs()
        mono = _check(lib().orbx_extract(self._h, image.ctypes.data, w, h, image.strides[0], int(vLappingArea[0]),
                                         int(vLappingArea[1]), None, None, self.capacity, b["nref"][0]))
        return (mono,) + self._take(self._result_views(b, 1, False)[0], b["n"][0].value)

    # ---- batched many-camera mode
    def extract_stereo(self, left, right, lap_left=(0, 0), lap_right=(0, 0), bf=0.0, b=0.0):
        """Both eyes of one stereo frame in one batched pipeline (orbx_extract_stereo; the handle needs max_batch >= 2).
        Returns ((monoL, kpsL, descL), (monoR, kpsR, descR)) and, when bf > 0, also (mvuRight, mvDepth) of the left eye."""
        L, R = np.asarray(left), np.asarray(right)
        if L.ndim != 2 or L.shape != R.shape:
            raise ValueError("two gray images of the same size")
        if L.dtype != np.uint8 or L.strides[-1] != 1:
            L = np.ascontiguousarray(L, np.uint8)
        if R.dtype != np.uint8 or R.strides[-1] != 1:
            R = np.ascontiguousarray(R, np.uint8)
        h, w = L.shape
        hb = self._host_bufs()
        lap = hb["lap"]
        lap[0], lap[1], lap[2], lap[3] = lap_left[0], lap_left[1], lap_right[0], lap_right[1]
        nl, nr, ml, mr = hb["n"]
        rl, rr, rml, rmr = hb["nref"]
        cap = self.capacity
        _check(lib().orbx_extract_stereo(self._h, L.ctypes.data, R.ctypes.data, w, h, L.strides[0], R.strides[0], hb["lapp"][0],
                                         hb["lapp"][1], None, None, cap, rl, rml, None, None, cap, rr, rmr,
                                         float(bf), float(b), None, None))
        v = self._result_views(hb, 2, bf > 0)
        out = ((ml.value,) + self._take(v[0], nl.value), (mr.value,) + self._take(v[1], nr.value))
        return out + ((v["ur"][:nl.value].copy(), v["dp"][:nl.value].copy()),) if bf > 0 else out

    def extract_rgbd(self, gray, depth, K, dist, bf, depth_scale):
        """One RGB-D frame (orbx_extract_rgbd): ExtractORB + UndistortKeyPoints + ComputeStereoFromRGBD of the RGB-D Frame
        constructor (src/Frame.cc:281-348) with GrabImageRGBD's depth conversion folded in.  depth = uint16 (CV_16U) or float32
        (CV_32F) image of the gray image's size; depth_scale = Tracking::mDepthMapFactor (depth_scale_from_settings).  Returns
        (mono, kps, desc, kpsUn, uRight, depth)."""
        g = np.asarray(gray)
        if g.ndim != 2 or g.dtype != np.uint8:
            raise ValueError("CV_8UC1 image expected")
        if g.strides[1] != 1:
            g = np.ascontiguousarray(g)
        D = np.asarray(depth)
        if D.shape != g.shape:
            raise ValueError("depth image must have the gray image's size")
        dtype = _DEPTH_TYPES.get(D.dtype.type)
        if dtype is None:
            raise ValueError("depth image must be uint16 (CV_16U) or float32 (CV_32F)")
        if D.strides[1] != D.itemsize or D.strides[0] % D.itemsize:
            D = np.ascontiguousarray(D)
        h, w = g.shape
        K = np.ascontiguousarray(K, np.float32) if K is not None else None
        d = np.ascontiguousarray(dist if dist is not None else [], np.float32).ravel()
        hb = self._host_bufs()
        cap = self.capacity
        kun = np.zeros(cap, KP_DTYPE)
        mono = _check(lib().orbx_extract_rgbd(self._h, g.ctypes.data, w, h, g.strides[0], D.ctypes.data, dtype, D.strides[0],
                                              float(depth_scale), float(bf), None if K is None else _p(K),
                                              _p(d) if len(d) else None, len(d), None, None, cap, hb["nref"][0], hb["nref"][1],
                                              _p(kun), None, None))
        n = hb["n"][0].value
        v = self._result_views(hb, 1, True)
        return (mono,) + self._take(v[0], n) + (kun[:n].copy(), v["ur"][:n].copy(), v["dp"][:n].copy())

    def map_upload(self, world_pos, normal, min_distance, max_distance, desc, flags):
        """The local map as structure-of-arrays, resident on the device (orbx_map_upload): GetWorldPos / GetNormal [n][3],
        mfMinDistance / mfMaxDistance [n], GetDescriptor [n][32], flags bit 0 isBad, bit 1 Observations() > 0."""
        a = [np.ascontiguousarray(world_pos, np.float32), np.ascontiguousarray(normal, np.float32),
             np.ascontiguousarray(min_distance, np.float32), np.ascontiguousarray(max_distance, np.float32),
             np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(flags, np.uint8)]
        n = len(a[2])
        _check(lib().orbx_map_upload(self._h, n, *[_p(x) for x in a]))
        self._map_n = n

    def project_map_points(self, poses, bounds, viewing_cos_limit=0.5, skip=None, want_views=False):
        """Frame::isInFrustum of every uploaded map point for every pose ([n_frames][20] floats: Rcw row-major, tcw, Ow, fx fy cx cy,
        bf) on the device (orbx_project_map_points_batch).  Returns the views (MP_DTYPE [n_frames][n]) when want_views."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 20)
        F = len(poses)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(F, self._map_n)
        views = np.zeros((F, self._map_n), MP_DTYPE) if want_views else None
        _check(lib().orbx_project_map_points_batch(self._h, F, _p(poses), bounds[0], bounds[1], bounds[2], bounds[3],
                                                   float(viewing_cos_limit), None if sk is None else _p(sk),
                                                   None if views is None else _p(views)))
        return views

    def project_map_points_fisheye(self, left_poses, right_poses, bounds, viewing_cos_limit=0.5, skip=None, want_views=False):
        """Frame::isInFrustum for stereo-fisheye frames on the device (orbx_project_map_points_fisheye_batch): one pose per camera
        and frame, 23 floats each (R row-major, t, twc, 8 KB8 parameters) -- the right camera's as the reference derives it
        (src/Frame.cc:1342-1351).  Returns (MP_DTYPE [F][n], MPR_DTYPE [F][n]) when want_views."""
        pl = np.ascontiguousarray(left_poses, np.float32).reshape(-1, 23)
        pr = np.ascontiguousarray(right_poses, np.float32).reshape(-1, 23)
        F = len(pl)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(F, self._map_n)
        vl = np.zeros((F, self._map_n), MP_DTYPE) if want_views else None
        vr = np.zeros((F, self._map_n), MPR_DTYPE) if want_views else None
        _check(lib().orbx_project_map_points_fisheye_batch(self._h, F, _p(pl), _p(pr), bounds[0], bounds[1], bounds[2], bounds[3],
                                                           float(viewing_cos_limit), None if sk is None else _p(sk),
                                                           None if vl is None else _p(vl), None if vr is None else _p(vr)))
        return (vl, vr) if want_views else None

    def last_frames_upload(self, n_points, world_pos, octave, angle, desc, flags):
        """The LastFrames of the batch's cameras as structure-of-arrays on the device (orbx_last_frames_upload): n_points [F];
        world_pos [F][stride][3], octave / angle / flags [F][stride], desc [F][stride][32]; flags bit 0 = map point present and no
        outlier, bit 1 = Observations() > 0."""
        npts = np.ascontiguousarray(n_points, np.int32)
        F = len(npts)
        pos = np.ascontiguousarray(world_pos, np.float32).reshape(F, -1, 3)
        stride = pos.shape[1]
        a = [pos, np.ascontiguousarray(octave, np.int32).reshape(F, stride), np.ascontiguousarray(angle, np.float32).reshape(F, stride),
             np.ascontiguousarray(desc, np.uint8).reshape(F, stride, 32), np.ascontiguousarray(flags, np.uint8).reshape(F, stride)]
        _check(lib().orbx_last_frames_upload(self._h, F, stride, _p(npts), *[_p(x) for x in a]))
        self._lf_n, self._lf_stride = npts.copy(), stride

    def project_last_frames(self, poses, directions, bounds, th, want_views=False):
        """The projection block of SearchByProjection(CurrentFrame, LastFrame) (src/ORBmatcher.cc:1606-1669) for every uploaded
        LastFrame point on the device (orbx_project_last_frames_batch): poses [F][12] floats (Sophus quaternion x y z w, translation,
        fx fy cx cy, bf), directions [F] (0 neither, 1 bForward, 2 bBackward).  Returns the views (PP_DTYPE [F][stride]) if asked."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
        F = len(poses)
        rec = np.zeros(F, np.dtype([("p", "<f4", (12,)), ("direction", "<i4")]))
        rec["p"], rec["direction"] = poses, np.ascontiguousarray(directions, np.int32)
        views = np.zeros((F, self._lf_stride), PP_DTYPE) if want_views else None
        _check(lib().orbx_project_last_frames_batch(self._h, F, _p(rec), bounds[0], bounds[1], bounds[2], bounds[3], float(th),
                                                    None if views is None else _p(views)))
        return views

    def extract_batch_device(self, d_images_ptr, n_images, w, h, row_pitch, image_pitch, lap=None):
        """Enqueue extraction of device-resident images (raw device pointer).  Asynchronous."""
        lap_arr = None if lap is None else np.ascontiguousarray(lap, np.int32).reshape(n_images, 2)
        _check(lib().orbx_extract_batch_device(self._h, C.c_void_p(d_images_ptr), n_images, w, h, row_pitch,
                                               image_pitch, None if lap_arr is None else _p(lap_arr)))

    def stream_handle(self):
        """Address of the handle's hipStream_t (orbx_stream_handle), e.g. for torch.cuda.ExternalStream."""
        st = C.c_void_p()
        _check(lib().orbx_stream_handle(self._h, C.byref(st)))
        return st.value or 0

    def allgather_descriptors(self, comm, n_images, d_all_desc_ptr, d_all_counts_ptr):
        """orbx_allgather_descriptors: one grouped RCCL all-gather of the last batch's descriptor blocks (desc rows + counts)
        of every rank into the caller's DEVICE arrays, enqueued on this handle's stream.  Asynchronous."""
        _check(lib().orbx_allgather_descriptors(self._h, comm._h, n_images, C.c_void_p(d_all_desc_ptr),
                                                C.c_void_p(d_all_counts_ptr)))

    def extract_batch_host(self, images_ptr, n_images, w, h, row_pitch, image_pitch, lap=None):
        """orbx_extract_batch: frames in HOST memory (page-locked for real overlap); asynchronous."""
        lp = None if lap is None else _p(np.ascontiguousarray(lap, np.int32))
        _check(lib().orbx_extract_batch(self._h, C.c_void_p(images_ptr), n_images, w, h, row_pitch, image_pitch, lp))

    def download_async(self, counts_ptr, mono_ptr, kps_ptr, desc_ptr, uright_ptr=None, depth_ptr=None, n_pairs=0):
        """orbx_batch_download_async into host arrays given by address (page-locked for real asynchrony)."""
        _check(lib().orbx_batch_download_async(self._h, counts_ptr, mono_ptr, kps_ptr, desc_ptr, uright_ptr, depth_ptr, n_pairs))

    def extract_batch_raw_device(self, preproc, d_frames_ptr, n_frames, row_pitch, image_pitch, lap=None):
        """Pre-processing chain + extraction of device-resident RAW frames on this handle's stream.  Asynchronous."""
        lap_arr = None if lap is None else np.ascontiguousarray(lap, np.int32).reshape(n_frames, 2)
        _check(lib().orbx_extract_batch_raw_device(self._h, preproc._h, C.c_void_p(d_frames_ptr), n_frames, row_pitch,
                                                   image_pitch, None if lap_arr is None else _p(lap_arr)))

    def sync(self):
        _check(lib().orbx_sync(self._h))

    def download(self, image):
        kps = np.zeros(self.capacity, KP_DTYPE)
        desc = np.zeros((self.capacity, 32), np.uint8)
        n = C.c_int()
        mono = _check(lib().orbx_batch_download(self._h, image, _p(kps), _p(desc), self.capacity, C.byref(n)))
        return mono, kps[:n.value].copy(), desc[:n.value].copy()

    def results_device(self):
        """(d_kps, d_desc, d_counts, d_mono, cap) raw device pointers of the last extraction."""
        a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        cap = C.c_int()
        _check(lib().orbx_batch_results_device(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d),
                                               C.byref(cap)))
        return a.value, b.value, c.value, d.value, cap.value

    # ---- measurement
    def profile_enable(self, on=True, stage=None):
        """on=True: bracket every kernel launch with HIP events; stage="k_detect" etc.: only that kernel."""
        mode = int(bool(on))
        if on and stage is not None:
            names = [lib().orbx_stage_name(s).decode() for s in range(NUM_STAGES)]
            mode = 2 + names.index(stage)
        _check(lib().orbx_profile_enable(self._h, mode))

    def profile_collect(self):
        """{stage name: (total ms, launches)} since the last collect (HIP events on the launch stream)."""
        ms = np.zeros(NUM_STAGES, np.float64)
        cnt = np.zeros(NUM_STAGES, np.int32)
        _check(lib().orbx_profile_collect(self._h, _p(ms), _p(cnt)))
        return {lib().orbx_stage_name(s).decode(): (float(ms[s]), int(cnt[s])) for s in range(NUM_STAGES)}

    def level_stats(self, image=0):
        L = self.nlevels
        w, h, nc, ns = (np.zeros(L, np.int32) for _ in range(4))
        _check(lib().orbx_level_stats(self._h, image, _p(w), _p(h), _p(nc), _p(ns)))
        return w, h, nc, ns

    # ---- mvImagePyramid (include/ORBextractor.h:86)
    def set_opencv_compat(self, opencv_version):
        """Gaussian taps of the reference build's OpenCV (include/orbx.h: orbx_set_opencv_compat): 440 = OpenCV 4.0 .. 4.5.0
        (README.md:101 "tested with 4.4.0") through the scalar fixed-point path, 44016 / 44032 = the same taps with the flooring 16- /
        32-lane vector body of those releases' vertical pass, 451 = OpenCV >= 4.5.1 (the default)."""
        _check(lib().orbx_set_opencv_compat(self._h, int(opencv_version)))

    def image_pyramid(self, level, image=0, blurred=False):
        w, h = C.c_int(), C.c_int()
        _check(lib().orbx_pyramid_level(self._h, image, level, int(blurred), None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _check(lib().orbx_pyramid_level(self._h, image, level, int(blurred), _p(out), out.strides[0],
                                        C.byref(w), C.byref(h)))
        return out

    def pyramid_download(self, image=0, out=None):
        """orbx_pyramid_download: every level of one image of the last extraction with ONE synchronisation (what the C++
        mirror's mvImagePyramid refresh does).  `out` = list of preallocated [h_l, w_l] uint8 arrays to reuse."""
        nl = self.GetLevels()
        if out is None:
            out = []
            w, h = C.c_int(), C.c_int()
            for l in range(nl):
                _check(lib().orbx_pyramid_level(self._h, image, l, 0, None, 0, C.byref(w), C.byref(h)))
                out.append(np.empty((h.value, w.value), np.uint8))
        ptrs = (C.c_void_p * nl)(*[a.ctypes.data for a in out])
        strides = (C.c_ssize_t * nl)(*[a.strides[0] for a in out])
        _check(lib().orbx_pyramid_download(self._h, image, nl, ptrs, strides))
        return out

    def set_host_pyramid(self, enable=True):
        """orbx_set_host_pyramid: the single-frame entries (`ex(image)`, `extract_stereo`) keep a host copy of the pyramid --
        the reference's public mvImagePyramid (include/ORBextractor.h:86) -- current, copied beside the frame's kernels."""
        _check(lib().orbx_set_host_pyramid(self._h, 1 if enable else 0))
        self._hpv = {}

    def host_pyramid(self, image=0):
        """orbx_host_pyramid_level for every level: numpy VIEWS of the handle's page-locked copy (no copy, no synchronisation;
        valid until the next extraction on this handle, like mvImagePyramid)."""
        key = None
        views = getattr(self, "_hpv", None)
        if views is None:
            views = self._hpv = {}
        p, w, h, st = C.c_void_p(), C.c_int(), C.c_int(), C.c_ssize_t()
        _check(lib().orbx_host_pyramid_level(self._h, image, 0, C.byref(p), C.byref(w), C.byref(h), C.byref(st)))
        key = (image, p.value, w.value, h.value, st.value)
        if key in views:   # the block and the geometry are unchanged: the views of the previous frame are this frame's
            return views[key]
        out = []
        for l in range(self.GetLevels()):
            _check(lib().orbx_host_pyramid_level(self._h, image, l, C.byref(p), C.byref(w), C.byref(h), C.byref(st)))
            buf = (C.c_uint8 * (st.value * (h.value - 1) + w.value)).from_address(p.value)
            a = np.frombuffer(buf, np.uint8)
            out.append(np.lib.stride_tricks.as_strided(a, (h.value, w.value), (st.value, 1), writeable=False))
        views[key] = out
        return out

    def debug_score_map(self, enable=True):
        """Test tap: following extractions also keep k_detect's pre-NMS FAST scores at iniThFAST (orbx_debug_score_map)."""
        _check(lib().orbx_debug_score_map(self._h, 1 if enable else 0))

    def debug_score_level(self, level, image=0):
        w, h = C.c_int(), C.c_int()
        _check(lib().orbx_pyramid_level(self._h, image, level, 0, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _check(lib().orbx_debug_score_level(self._h, image, level, _p(out), w.value))
        return out

    def debug_resize_plan(self):
        """Fused small-level resize launches of the handle's current image size: [(first_level, n_levels, n_bands), ...]."""
        a, b, c = (np.zeros(16, np.int32) for _ in range(3))
        n = _check(lib().orbx_debug_resize_plan(self._h, _p(a), _p(b), _p(c), 16))
        return [(int(a[i]), int(b[i]), int(c[i])) for i in range(n)]

    def debug_candidates(self, level, image=0):
        cap = 1 << 20
        out = np.zeros((cap, 3), np.int32)
        n = _check(lib().orbx_debug_candidates(self._h, image, level, _p(out), cap))
        return out[:n].copy()

    def debug_octree(self, width, height, candidates):
        """k_octree alone on the caller's candidates (orbx_debug_octree): candidates[image][level] = (n, 3) integers (x, y,
        response), x, y relative to the (16,16) window origin, in any order.  Returns selected[image][level] = (m, 3) int32 (x, y,
        response) in list order, level coordinates.  The launch is the one an extraction of len(candidates) images makes."""
        counts, flat = _octree_candidates(candidates, self.nlevels)
        n = len(candidates)
        cap = int(self._nfeat.max()) + 64
        nsel = np.zeros(n * self.nlevels, np.int32)
        sel = np.zeros((n, self.nlevels, cap, 3), np.int32)
        _check(lib().orbx_debug_octree(self._h, int(width), int(height), n, _p(counts), _p(flat), _p(nsel), _p(sel), cap))
        return [[sel[i, l, :nsel[i * self.nlevels + l]].copy() for l in range(self.nlevels)] for i in range(n)]

    def debug_resize_stream(self, d_images_ptr, n_images, w, h, row_pitch, image_pitch, kernel=1, quads=0, band=0):
        """Test hook (orbx_debug_resize_stream): levels 1.. of n_images device frames into the handle's pyramid with one kernel
        for every level -- kernel 1 = k_resize_stream (strips of `quads` quads, bands of `band` rows; 0 = the batched path's),
        kernel 0 = the tiled k_resize -- whatever the batch size; synchronises.  pyramid_download(i) returns the levels."""
        _check(lib().orbx_debug_resize_stream(self._h, C.c_void_p(d_images_ptr), int(n_images), int(w), int(h), int(row_pitch),
                                              int(image_pitch), int(kernel), int(quads), int(band)))

    def debug_fill_work_buffers(self, byte):
        """Test hook: every device buffer of the handle that a call produces before it reads it set to `byte`
        (orbx_debug_fill_work_buffers); tables, uploads and protocol state stay."""
        _check(lib().orbx_debug_fill_work_buffers(self._h, int(byte)))


SCRATCH_STATS, SCRATCH_FILL, SCRATCH_TRIM = 0, 1, 2


def scratch_pool_stats(device=0):
    """The one-shot entries' scratch pool on `device` (orbx_debug_scratch_pool): (cached blocks, cached bytes, blocks taken so
    far, those served from the cache)."""
    out = np.zeros(4, np.uint64)
    _check(lib().orbx_debug_scratch_pool(int(device), SCRATCH_STATS, 0, _p(out)))
    return tuple(int(v) for v in out)


def scratch_pool_fill(byte, device=0):
    """Sets every cached block of the pool and the calling thread's upload staging buffer to `byte`; returns the device bytes
    filled."""
    out = np.zeros(4, np.uint64)
    _check(lib().orbx_debug_scratch_pool(int(device), SCRATCH_FILL, int(byte), _p(out)))
    return int(out[0])


def scratch_pool_trim(device=0):
    """Frees every cached block of the pool."""
    _check(lib().orbx_debug_scratch_pool(int(device), SCRATCH_TRIM, 0, None))


def clock_probe_start(device=0, spin_us=2000):
    """orbx_clock_probe_start: one wave spins for spin_us on a private stream; finish() returns the shader clock in GHz."""
    h = C.c_void_p()
    _check(lib().orbx_clock_probe_start(device, int(spin_us), C.byref(h)))
    return h


def clock_probe_finish(probe):
    g = C.c_double()
    _check(lib().orbx_clock_probe_finish(probe, C.byref(g)))
    return g.value


COMM_ID_BYTES = 128


def comm_unique_id():
    """orbx_comm_unique_id: the 128-byte RCCL id rank 0 creates and ships to the other ranks."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(lib().orbx_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """RCCL communicator behind the C ABI (orbx_comm_create: collective over all ranks; one rank per GPU)."""

    def __init__(self, unique_id, n_ranks, rank, device=0):
        assert len(unique_id) == COMM_ID_BYTES
        self._h = C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(lib().orbx_comm_create(buf, n_ranks, rank, device, C.byref(self._h)))
        self.n_ranks, self.rank = n_ranks, rank

    def wait(self, timeout_ms=60000):
        """Block until the communicator's most recent collective has completed (OrbxError E_TIMEOUT after timeout_ms: a rank
        is missing or out of order).  Returns the number of collectives enqueued so far."""
        n = C.c_ulonglong(0)
        _check(lib().orbx_comm_wait(self._h, int(timeout_ms), C.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().orbx_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ComputeStereoMatches(left, right, bf, b, first_left=0, first_right=0, n_pairs=1):
    """Frame::ComputeStereoMatches (src/Frame.cc:921-1084) on the last extractions of two extractors
    (or one extractor holding both eyes).  Returns (mvuRight, mvDepth) arrays [n_pairs][capacity]."""
    _check(lib().orbx_stereo_match_batch(left._h, first_left, right._h, first_right, n_pairs, bf, b))
    out_u = np.zeros((n_pairs, left.capacity), np.float32)
    out_d = np.zeros((n_pairs, left.capacity), np.float32)
    for p in range(n_pairs):
        _check(lib().orbx_stereo_download(left._h, p, _p(out_u[p]), _p(out_d[p]), left.capacity))
    return out_u, out_d


def stereo_match_async(left, right, bf, b, first_left=0, first_right=0, n_pairs=1):
    _check(lib().orbx_stereo_match_batch(left._h, first_left, right._h, first_right, n_pairs, bf, b))


_DEPTH_TYPES = {np.uint16: 2, np.float32: 5}   # ORBX_DEPTH_U16 (CV_16U), ORBX_DEPTH_F32 (CV_32F)
DEPTH_U16, DEPTH_F32 = 2, 5


def depth_scale_from_settings(DepthMapFactor):
    """Tracking::mDepthMapFactor from the settings' RGBD.DepthMapFactor (src/Tracking.cc:610-614): 1 when |factor| < 1e-5,
    else 1.0f / factor -- as np.float32."""
    f = np.float32(DepthMapFactor)
    if abs(float(f)) < 1e-5:
        return np.float32(1.0)
    return np.float32(np.float32(1.0) / f)


def _rgbd_enqueue(ex, d_depth_ptr, depth_type, row_pitch, image_pitch, bf, depth_scale, K, dist, first_image, n_frames,
                  d_kps_un_ptr):
    K = None if K is None else np.ascontiguousarray(K, np.float32)
    d = np.ascontiguousarray(dist if dist is not None else [], np.float32).ravel()
    _check(lib().orbx_rgbd_depth_batch(ex._h, first_image, n_frames, C.c_void_p(d_depth_ptr), int(depth_type), row_pitch,
                                       image_pitch, float(depth_scale), float(bf), None if K is None else _p(K),
                                       _p(d) if len(d) else None, len(d),
                                       None if d_kps_un_ptr is None else C.c_void_p(d_kps_un_ptr)))


def ComputeStereoFromRGBD(ex, d_depth_ptr, depth_type, row_pitch, image_pitch, bf, depth_scale, K=None, dist=None, first_image=0,
                          n_frames=1, d_kps_un_ptr=None):
    """Frame::ComputeStereoFromRGBD (src/Frame.cc:1086-1104) for images [first_image, first_image + n_frames) of ex's last
    extraction, from device-resident depth images (orbx_rgbd_depth_batch; depth_type DEPTH_U16 / DEPTH_F32, frame f at
    d_depth_ptr + f * image_pitch).  The results land in the handle's stereo result arrays (pair f = frame f: a matcher's
    stereo_pair0 reads them).  Returns (mvuRight, mvDepth) arrays [n_frames][capacity]."""
    _rgbd_enqueue(ex, d_depth_ptr, depth_type, row_pitch, image_pitch, bf, depth_scale, K, dist, first_image, n_frames,
                  d_kps_un_ptr)
    out_u = np.zeros((n_frames, ex.capacity), np.float32)
    out_d = np.zeros((n_frames, ex.capacity), np.float32)
    for p in range(n_frames):
        _check(lib().orbx_stereo_download(ex._h, p, _p(out_u[p]), _p(out_d[p]), ex.capacity))
    return out_u, out_d


def rgbd_depth_async(ex, d_depth_ptr, depth_type, row_pitch, image_pitch, bf, depth_scale, K=None, dist=None, first_image=0,
                     n_frames=1, d_kps_un_ptr=None):
    _rgbd_enqueue(ex, d_depth_ptr, depth_type, row_pitch, image_pitch, bf, depth_scale, K, dist, first_image, n_frames,
                  d_kps_un_ptr)


def _pose_frames(q, t, cam, n_frames):
    fr = np.zeros(n_frames, POSE_DTYPE)
    fr["q"] = np.asarray(q, np.float32).reshape(n_frames, 4)
    fr["t"] = np.asarray(t, np.float32).reshape(n_frames, 3)
    cam = np.asarray(cam, np.float32).reshape(-1, 5)
    for j, name in enumerate(("fx", "fy", "cx", "cy", "bf")):
        fr[name] = cam[:, j]
    return fr


def PoseOptimization(kpsUn, uRight, worldPos, hasPoint, invLevelSigma2, q, t, cam, outlier=None, device=0):
    """Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:781-1107) for a pinhole / rectified frame on the GPU
    (orbx_pose_optimization).  kpsUn = mvKeysUn (KP_DTYPE), uRight = mvuRight (None: every edge mono), worldPos [n][3] and
    hasPoint [n] = the frame's map points, invLevelSigma2 = mvInvLevelSigma2, (q, t) = Tcw as Sophus stores it (x y z w),
    cam = (fx, fy, cx, cy, mbf), outlier = mvbOutlier (entries without a point keep their value; default all False).
    Returns (nGood, q, t, outlier)."""
    k = np.ascontiguousarray(kpsUn, KP_DTYPE)
    n = len(k)
    ur = None if uRight is None else np.ascontiguousarray(uRight, np.float32).reshape(n)
    wp = np.ascontiguousarray(worldPos, np.float32).reshape(n, 3)
    hp = np.ascontiguousarray(hasPoint, np.uint8).reshape(n)
    sig = np.ascontiguousarray(invLevelSigma2, np.float32)
    fr = _pose_frames(q, t, cam, 1)
    out = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, np.uint8).reshape(n)
    ng = _check(lib().orbx_pose_optimization(int(device), _p(k), None if ur is None else _p(ur), _p(wp), _p(hp), n, _p(sig),
                                             len(sig), _p(fr), _p(out)))
    return ng, fr["q"][0].copy(), fr["t"][0].copy(), out.astype(bool)


def PoseOptimizationBatch(ex, first_image, n_frames, worldPos, hasPoint, q, t, cam, stereo_pair0=-1, outlier=None,
                          want_trials=False):
    """PoseOptimization of the frames of ex's last extraction batch in ONE kernel launch (orbx_pose_optimization_batch):
    frame f = image first_image + f, keypoints = mvKeysUn, mvInvLevelSigma2 = the handle's, mvuRight from stereo pair
    stereo_pair0 + f (-1: monocular).  worldPos [n_frames][cap][3], hasPoint / outlier [n_frames][cap], q [n_frames][4],
    t [n_frames][3], cam [n_frames][5] (or one row for all).  Returns (nGood, q, t, outlier[, trials])."""
    cap = ex.capacity
    wp = np.ascontiguousarray(worldPos, np.float32).reshape(n_frames, cap, 3)
    hp = np.ascontiguousarray(hasPoint, np.uint8).reshape(n_frames, cap)
    cam = np.broadcast_to(np.asarray(cam, np.float32).reshape(-1, 5), (n_frames, 5))
    fr = _pose_frames(q, t, cam, n_frames)
    out = np.zeros((n_frames, cap), np.uint8) if outlier is None else np.array(outlier, np.uint8).reshape(n_frames, cap)
    ng = np.zeros(n_frames, np.int32)
    tr = np.zeros(n_frames, np.int32)
    _check(lib().orbx_pose_optimization_batch(ex._h, int(first_image), int(n_frames), int(stereo_pair0), _p(wp), _p(hp), _p(fr),
                                              _p(out), _p(ng), _p(tr)))
    res = (ng, fr["q"].copy(), fr["t"].copy(), out.astype(bool))
    return res + (tr,) if want_trials else res


TWO_VIEW_PARAMS_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("sigma", "<f4"),
                                  ("rh_threshold", "<f4"), ("iterations", "<i4")])
TWO_VIEW_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("model", "<i4"), ("best_h", "<i4"), ("best_f", "<i4"), ("score_h", "<f4"),
                                  ("score_f", "<f4"), ("n_matches", "<i4"), ("n_inliers", "<i4"), ("n_good", "<i4"),
                                  ("parallax", "<f4"), ("q", "<f4", (4,)), ("t", "<f4", (3,))])
assert TWO_VIEW_PARAMS_DTYPE.itemsize == 28 and TWO_VIEW_RESULT_DTYPE.itemsize == 68  # orbx_two_view_params / _result

_libc = None


def ransac_sets(n_matches, iterations=200, seed_once=True):
    """The 8-point index sets of TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc:69-96) drawn the reference's
    way from the host's libc: DUtils::Random::SeedRandOnce(0) (srand(0) on the first call of the process only; seed_once=False
    skips it), RandomInt(0, d - 1) = int(((double)rand() / ((double)RAND_MAX + 1.0)) * d), swap-with-back removal.
    Returns [iterations][8] int32 indices into the match list; n_matches < 8 returns zeros (the library does not read them)."""
    global _libc
    if _libc is None:
        _libc = C.CDLL(None)
        _libc.rand.restype = C.c_int
        _libc.srand.argtypes = [C.c_uint]
        if seed_once:
            _libc.srand(0)
    sets = np.zeros((iterations, 8), np.int32)
    if n_matches < 8:
        return sets
    rand_max = 2147483647  # glibc RAND_MAX
    for it in range(iterations):
        avail = list(range(n_matches))
        for j in range(8):
            d = len(avail)
            randi = int((float(_libc.rand()) / (float(rand_max) + 1.0)) * d)
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


def _two_view_params(K, sigma, iterations, rh_threshold):
    prm = np.zeros(1, TWO_VIEW_PARAMS_DTYPE)
    K = np.asarray(K, np.float32)
    prm["fx"], prm["fy"], prm["cx"], prm["cy"] = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.ndim == 2 else K[:4]
    prm["sigma"], prm["rh_threshold"], prm["iterations"] = sigma, rh_threshold, iterations
    return prm


def ReconstructWithTwoViews(vKeys1, vKeys2, vMatches12, K, sets=None, sigma=1.0, iterations=200, rh_threshold=0.5,
                            want_scores=False, device=0):
    """Pinhole::ReconstructWithTwoViews = TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc) on the GPU
    (orbx_reconstruct_two_views).  vKeys1 / vKeys2 = mvKeysUn of the initial and the current frame (KP_DTYPE), vMatches12 [n1]
    (-1: unmatched), K = 3 x 3 pinhole matrix or (fx, fy, cx, cy), sets = [iterations][8] indices into the match list
    (None: ransac_sets).  Returns (ok, q, t, vP3D [n1][3], vbTriangulated [n1], result record[, hyp_scores [2][iterations]])."""
    k1, k2 = np.ascontiguousarray(vKeys1, KP_DTYPE), np.ascontiguousarray(vKeys2, KP_DTYPE)
    m = np.ascontiguousarray(vMatches12, np.int32).reshape(len(k1))
    if sets is None:
        sets = ransac_sets(int((m >= 0).sum()), iterations)
    st = np.ascontiguousarray(sets, np.int32).reshape(iterations, 8)
    prm = _two_view_params(K, sigma, iterations, rh_threshold)
    res = np.zeros(1, TWO_VIEW_RESULT_DTYPE)
    p3d = np.zeros((len(k1), 3), np.float32)
    tri = np.zeros(len(k1), np.uint8)
    sc = np.zeros((2, iterations), np.float32)
    _check(lib().orbx_reconstruct_two_views(int(device), _p(k1), len(k1), _p(k2), len(k2), _p(m), _p(st), _p(prm), _p(res), _p(p3d),
                                            _p(tri), _p(sc) if want_scores else None))
    r = res[0]
    out = (bool(r["ok"]), r["q"].copy(), r["t"].copy(), p3d, tri.astype(bool), r)
    return out + (sc,) if want_scores else out


def ReconstructWithTwoViewsBatch(ex, first_image, vKeys1, vMatches12, K, sets=None, sigma=1.0, iterations=200, rh_threshold=0.5,
                                 want_scores=False):
    """ReconstructWithTwoViews for the frames of ex's last extraction batch in one call (orbx_reconstruct_two_views_batch), in
    the layout of ORBmatcher.SearchForInitializationBatch: pair f = (vKeys1[f], image first_image + f), vMatches12[f] as that
    call returned it, sets[f] [iterations][8] (None: ransac_sets per pair, in pair order).  Returns (results
    [F] TWO_VIEW_RESULT_DTYPE, list of vP3D, list of vbTriangulated[, hyp_scores [F][2][iterations]])."""
    F = len(vKeys1)
    n1 = np.array([len(k) for k in vKeys1], np.int32)
    stride = max(int(n1.max()) if F else 0, 1)
    Kp = np.zeros((F, stride), KP_DTYPE)
    M = np.full((F, stride), -1, np.int32)
    for f in range(F):
        Kp[f, :n1[f]] = vKeys1[f]
        M[f, :n1[f]] = np.asarray(vMatches12[f], np.int32)
    if sets is None:
        sets = [ransac_sets(int((M[f] >= 0).sum()), iterations) for f in range(F)]
    st = np.ascontiguousarray(np.asarray(sets, np.int32).reshape(F, iterations, 8))
    prm = _two_view_params(K, sigma, iterations, rh_threshold)
    res = np.zeros(F, TWO_VIEW_RESULT_DTYPE)
    p3d = np.zeros((F, stride, 3), np.float32)
    tri = np.zeros((F, stride), np.uint8)
    sc = np.zeros((F, 2, iterations), np.float32)
    _check(lib().orbx_reconstruct_two_views_batch(ex._h, int(first_image), F, _p(Kp), _p(n1), stride, _p(M), _p(st), _p(prm),
                                                  _p(res), _p(p3d), _p(tri), _p(sc) if want_scores else None))
    out = (res, [p3d[f, :n1[f]].copy() for f in range(F)], [tri[f, :n1[f]].astype(bool) for f in range(F)])
    return out + (sc,) if want_scores else out


MLPNP_PARAMS_DTYPE = np.dtype([("model", "<i4"), ("cam", "<f4", (8,)), ("kb8_precision", "<f4"), ("th2", "<f4"), ("min_set", "<i4"),
                               ("min_inliers", "<i4"), ("max_iterations", "<i4"), ("call_iterations", "<i4")])
MLPNP_STATE_DTYPE = np.dtype([("iterations", "<i4"), ("best_inliers", "<i4"), ("best_Tcw", "<f4", (12,))])
MLPNP_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("no_more", "<i4"), ("n_inliers", "<i4"), ("n_correspondences", "<i4"),
                               ("iterations_run", "<i4"), ("hypothesis", "<i4"), ("refined", "<i4"), ("Tcw", "<f4", (12,))])
assert MLPNP_PARAMS_DTYPE.itemsize == 60 and MLPNP_STATE_DTYPE.itemsize == 56 and MLPNP_RESULT_DTYPE.itemsize == 76
CAMERA_PINHOLE, CAMERA_KB8 = 0, 1


def MLPnPRansacParameters(n_correspondences, probability=0.99, minInliers=8, maxIterations=300, minSet=6, epsilon=0.4):
    """MLPnPsolver::SetRansacParameters (src/MLPnPsolver.cpp:225-263) in its own arithmetic (orbx_mlpnp_ransac_parameters; host
    code, no device).  Defaults: include/MLPnPsolver.h; Tracking::Relocalization passes (0.99, 10, 300, 6, 0.5, 5.991).
    Returns (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon) as adjusted to the number of correspondences."""
    mi, it, ep = C.c_int32(0), C.c_int32(0), C.c_float(0)
    _check(lib().orbx_mlpnp_ransac_parameters(int(n_correspondences), float(probability), int(minInliers), int(maxIterations),
                                              int(minSet), float(epsilon), C.addressof(mi), C.addressof(it), C.addressof(ep)))
    return mi.value, it.value, ep.value


def mlpnp_sets(n_correspondences, n_sets, seed=None):
    """The six-point index sets of MLPnPsolver::iterate (src/MLPnPsolver.cpp:129-148) drawn the reference's way from the host's
    libc: RandomInt(0, d - 1) = int(((double)rand() / ((double)RAND_MAX + 1.0)) * d), swap-with-back removal.  seed: srand(seed)
    first (None: the process' rand() state as it stands).  Returns [n_sets][6] int32 indices into the correspondence list;
    fewer than 6 correspondences return zeros (the library does not read them)."""
    global _libc
    if _libc is None:
        _libc = C.CDLL(None)
        _libc.rand.restype = C.c_int
        _libc.srand.argtypes = [C.c_uint]
    if seed is not None:
        _libc.srand(int(seed))
    sets = np.zeros((n_sets, 6), np.int32)
    if n_correspondences < 6:
        return sets
    rand_max = 2147483647  # glibc RAND_MAX
    for it in range(n_sets):
        avail = list(range(n_correspondences))
        for j in range(6):
            d = len(avail)
            randi = int((float(_libc.rand()) / (float(rand_max) + 1.0)) * d)
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


def mlpnp_params(camera, min_inliers, max_iterations, call_iterations=5, th2=5.991, kb8_precision=1e-6, n=1):
    """orbx_mlpnp_params records: camera = (fx, fy, cx, cy) for a pinhole, (fx, fy, cx, cy, k0, k1, k2, k3) for KannalaBrandt8;
    min_inliers / max_iterations as MLPnPRansacParameters adjusted them; call_iterations = iterate's nIterations."""
    prm = np.zeros(n, MLPNP_PARAMS_DTYPE)
    cam = np.asarray(camera, np.float32).reshape(-1)
    prm["model"] = CAMERA_KB8 if len(cam) == 8 else CAMERA_PINHOLE
    prm["cam"][:, :len(cam)] = cam
    prm["kb8_precision"], prm["th2"], prm["min_set"] = kb8_precision, th2, 6
    prm["min_inliers"], prm["max_iterations"], prm["call_iterations"] = min_inliers, max_iterations, call_iterations
    return prm


def MLPnPIterate(kpsUn, worldPos, hasPoint, levelSigma2, params, sets, state=None, best_mask=None, n_left=None,
                 want_hyp=False, device=0):
    """One MLPnPsolver::iterate call (src/MLPnPsolver.cpp:107-223) on the GPU (orbx_mlpnp_iterate).  kpsUn = mvKeysUn (KP_DTYPE),
    worldPos [n][3] / hasPoint [n] = vpMapPointMatches, levelSigma2 = mvLevelSigma2, params = an mlpnp_params record, sets =
    [n_sets][6] indices into the correspondence list (mlpnp_sets), state / best_mask = what an earlier call returned (None: a
    fresh solver), n_left = the number of left-camera keypoints (None: all).  Returns (result record, vbInliers [n] bool, state,
    best_mask[, hyp_inliers [n_sets]])."""
    k = np.ascontiguousarray(kpsUn, KP_DTYPE)
    n = len(k)
    wp = np.ascontiguousarray(worldPos, np.float32).reshape(n, 3)
    hp = np.ascontiguousarray(hasPoint, np.uint8).reshape(n)
    sig = np.ascontiguousarray(levelSigma2, np.float32)
    prm = np.ascontiguousarray(params, MLPNP_PARAMS_DTYPE).reshape(1)
    st = np.ascontiguousarray(sets, np.int32).reshape(-1, 6)
    state = np.zeros(1, MLPNP_STATE_DTYPE) if state is None else np.array(state, MLPNP_STATE_DTYPE).reshape(1)
    bm = np.zeros(n, np.uint8) if best_mask is None else np.array(best_mask, np.uint8).reshape(n)
    res = np.zeros(1, MLPNP_RESULT_DTYPE)
    inl = np.zeros(n, np.uint8)
    hyp = np.full(len(st), -1, np.int32)
    _check(lib().orbx_mlpnp_iterate(int(device), _p(k), n, n if n_left is None else int(n_left), _p(wp), _p(hp), _p(sig), len(sig),
                                    _p(prm), _p(st), len(st), _p(state), _p(bm), _p(res), _p(inl), _p(hyp) if want_hyp else None))
    out = (res[0], inl.astype(bool), state, bm)
    return out + (hyp,) if want_hyp else out


def MLPnPIterateBatch(ex, image, worldPos, hasPoint, params, sets, states=None, best_masks=None, want_hyp=False):
    """MLPnPIterate for n_problems solvers in one call (orbx_mlpnp_iterate_batch): problem p uses the keypoints of image image[p]
    of ex's last extraction batch.  worldPos [P][cap][3], hasPoint [P][cap] (the row layout SearchByBoWBatch returns its matches
    in: hasPoint = matches >= 0), params [P] records, sets [P][n_sets][6].  Returns (results [P], vbInliers [P][cap] bool,
    states [P], best_masks [P][cap][, hyp_inliers [P][n_sets]])."""
    img = np.ascontiguousarray(image, np.int32).reshape(-1)
    P, cap = len(img), ex.capacity
    wp = np.ascontiguousarray(worldPos, np.float32).reshape(P, cap, 3)
    hp = np.ascontiguousarray(hasPoint, np.uint8).reshape(P, cap)
    prm = np.ascontiguousarray(params, MLPNP_PARAMS_DTYPE).reshape(P)
    st = np.ascontiguousarray(sets, np.int32).reshape(P, -1, 6)
    states = np.zeros(P, MLPNP_STATE_DTYPE) if states is None else np.array(states, MLPNP_STATE_DTYPE).reshape(P)
    bm = np.zeros((P, cap), np.uint8) if best_masks is None else np.array(best_masks, np.uint8).reshape(P, cap)
    res = np.zeros(P, MLPNP_RESULT_DTYPE)
    inl = np.zeros((P, cap), np.uint8)
    hyp = np.full((P, st.shape[1]), -1, np.int32)
    _check(lib().orbx_mlpnp_iterate_batch(ex._h, P, _p(img), _p(wp), _p(hp), _p(prm), _p(st), st.shape[1], _p(states), _p(bm),
                                          _p(res), _p(inl), _p(hyp) if want_hyp else None))
    out = (res, inl.astype(bool), states, bm)
    return out + (hyp,) if want_hyp else out


SIM3_PARAMS_DTYPE = np.dtype([("model1", "<i4"), ("cam1", "<f4", (8,)), ("model2", "<i4"), ("cam2", "<f4", (8,)),
                              ("kb8_precision", "<f4"), ("fix_scale", "<i4"), ("min_inliers", "<i4"), ("max_iterations", "<i4"),
                              ("call_iterations", "<i4")])
SIM3_STATE_DTYPE = np.dtype([("iterations", "<i4"), ("best_inliers", "<i4"), ("best_R", "<f4", (9,)), ("best_t", "<f4", (3,)),
                             ("best_s", "<f4")])
SIM3_RESULT_DTYPE = np.dtype([("converged", "<i4"), ("no_more", "<i4"), ("n_inliers", "<i4"), ("n_correspondences", "<i4"),
                              ("iterations_run", "<i4"), ("hypothesis", "<i4"), ("R12", "<f4", (9,)), ("t12", "<f4", (3,)),
                              ("s12", "<f4"), ("T12", "<f4", (12,))])
assert SIM3_PARAMS_DTYPE.itemsize == 92 and SIM3_STATE_DTYPE.itemsize == 60 and SIM3_RESULT_DTYPE.itemsize == 124


def Sim3RansacParameters(n_correspondences, probability=0.99, minInliers=6, maxIterations=300):
    """Sim3Solver::SetRansacParameters (src/Sim3Solver.cc:120-145) in its own arithmetic (orbx_sim3_ransac_parameters; host code,
    no device).  Defaults: include/Sim3Solver.h; LoopClosing::DetectCommonRegionsFromBoW passes (0.99, 15, 300).  Returns
    mRansacMaxIts as adjusted to the number of correspondences."""
    it = C.c_int32(0)
    _check(lib().orbx_sim3_ransac_parameters(int(n_correspondences), float(probability), int(minInliers), int(maxIterations),
                                             C.addressof(it)))
    return it.value


def sim3_sets(n_correspondences, n_sets, seed=None):
    """The triples of Sim3Solver::iterate (src/Sim3Solver.cc:170-183) drawn the reference's way from the host's libc, as
    mlpnp_sets draws MLPnPsolver's six.  Returns [n_sets][3] int32 indices into the correspondence list; fewer than 3
    correspondences return zeros (the library does not read them)."""
    global _libc
    if _libc is None:
        _libc = C.CDLL(None)
        _libc.rand.restype = C.c_int
        _libc.srand.argtypes = [C.c_uint]
    if seed is not None:
        _libc.srand(int(seed))
    sets = np.zeros((n_sets, 3), np.int32)
    if n_correspondences < 3:
        return sets
    rand_max = 2147483647  # glibc RAND_MAX
    for it in range(n_sets):
        avail = list(range(n_correspondences))
        for j in range(3):
            d = len(avail)
            randi = int((float(_libc.rand()) / (float(rand_max) + 1.0)) * d)
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


def sim3_params(camera1, camera2, min_inliers, max_iterations, call_iterations=20, fix_scale=False, kb8_precision=1e-6, n=1):
    """orbx_sim3_params records: camera1 / camera2 = (fx, fy, cx, cy) for a pinhole, (fx, fy, cx, cy, k0, k1, k2, k3) for
    KannalaBrandt8; max_iterations as Sim3RansacParameters adjusted it; call_iterations = iterate's nIterations."""
    prm = np.zeros(n, SIM3_PARAMS_DTYPE)
    for k, camera in (("1", camera1), ("2", camera2)):
        cam = np.asarray(camera, np.float32).reshape(-1)
        prm["model" + k] = CAMERA_KB8 if len(cam) == 8 else CAMERA_PINHOLE
        prm["cam" + k][:, :len(cam)] = cam
    prm["kb8_precision"], prm["fix_scale"] = kb8_precision, int(bool(fix_scale))
    prm["min_inliers"], prm["max_iterations"], prm["call_iterations"] = min_inliers, max_iterations, call_iterations
    return prm


def Sim3Iterate(Tcw1, Tcw2, worldPos1, worldPos2, matched, octave1, octave2, levelSigma2_1, levelSigma2_2, params, sets,
                state=None, best_mask=None, want_hyp=False, device=0):
    """One Sim3Solver::iterate call (src/Sim3Solver.cc:147-281) on the GPU (orbx_sim3_iterate).  Tcw1 / Tcw2 = the key frames'
    poses (3 x 4 or 4 x 4), worldPos1 / worldPos2 [n][3] = the map point of key frame 1 at i1 and vpMatched12[i1], matched [n],
    octave1 / octave2 [n], the two mvLevelSigma2 tables, params = a sim3_params record, sets = [n_sets][3] indices into the
    correspondence list (sim3_sets), state / best_mask = what an earlier call returned (None: a fresh solver).  Returns (result
    record, vbInliers [n] bool, state, best_mask[, hyp_inliers [n_sets]])."""
    m = np.ascontiguousarray(matched, np.uint8).reshape(-1)
    n = len(m)
    T1 = np.ascontiguousarray(np.asarray(Tcw1, np.float32).reshape(-1)[:12])
    T2 = np.ascontiguousarray(np.asarray(Tcw2, np.float32).reshape(-1)[:12])
    w1 = np.ascontiguousarray(worldPos1, np.float32).reshape(n, 3)
    w2 = np.ascontiguousarray(worldPos2, np.float32).reshape(n, 3)
    o1 = np.ascontiguousarray(octave1, np.int32).reshape(n)
    o2 = np.ascontiguousarray(octave2, np.int32).reshape(n)
    s1 = np.ascontiguousarray(levelSigma2_1, np.float32)
    s2 = np.ascontiguousarray(levelSigma2_2, np.float32)
    prm = np.ascontiguousarray(params, SIM3_PARAMS_DTYPE).reshape(1)
    st = np.ascontiguousarray(sets, np.int32).reshape(-1, 3)
    state = np.zeros(1, SIM3_STATE_DTYPE) if state is None else np.array(state, SIM3_STATE_DTYPE).reshape(1)
    bm = np.zeros(n, np.uint8) if best_mask is None else np.array(best_mask, np.uint8).reshape(n)
    res = np.zeros(1, SIM3_RESULT_DTYPE)
    inl = np.zeros(n, np.uint8)
    hyp = np.full(len(st), -1, np.int32)
    _check(lib().orbx_sim3_iterate(int(device), n, _p(T1), _p(T2), _p(w1), _p(w2), _p(m), _p(o1), _p(o2), _p(s1), len(s1), _p(s2),
                                   len(s2), _p(prm), _p(st), len(st), _p(state), _p(bm), _p(res), _p(inl),
                                   _p(hyp) if want_hyp else None))
    out = (res[0], inl.astype(bool), state, bm)
    return out + (hyp,) if want_hyp else out


def Sim3IterateBatch(n, Tcw1, Tcw2, worldPos1, worldPos2, matched, octave1, octave2, levelSigma2_1, levelSigma2_2, params, sets,
                     states=None, best_masks=None, want_hyp=False, device=0):
    """Sim3Iterate for n_problems solvers in one call (orbx_sim3_iterate_batch): n [P] key points per problem, Tcw1 / Tcw2
    [P][12], worldPos1 / worldPos2 [P][cap][3], matched / octave1 / octave2 [P][cap], the two mvLevelSigma2 tables (shared),
    params [P] records, sets [P][n_sets][3].  Returns (results [P], vbInliers [P][cap] bool, states [P], best_masks [P][cap][,
    hyp_inliers [P][n_sets]])."""
    nn = np.ascontiguousarray(n, np.int32).reshape(-1)
    P = len(nn)
    m = np.ascontiguousarray(matched, np.uint8).reshape(P, -1)
    cap = m.shape[1]
    T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(P, 12)
    T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(P, 12)
    w1 = np.ascontiguousarray(worldPos1, np.float32).reshape(P, cap, 3)
    w2 = np.ascontiguousarray(worldPos2, np.float32).reshape(P, cap, 3)
    o1 = np.ascontiguousarray(octave1, np.int32).reshape(P, cap)
    o2 = np.ascontiguousarray(octave2, np.int32).reshape(P, cap)
    s1 = np.ascontiguousarray(levelSigma2_1, np.float32)
    s2 = np.ascontiguousarray(levelSigma2_2, np.float32)
    prm = np.ascontiguousarray(params, SIM3_PARAMS_DTYPE).reshape(P)
    st = np.ascontiguousarray(sets, np.int32).reshape(P, -1, 3)
    states = np.zeros(P, SIM3_STATE_DTYPE) if states is None else np.array(states, SIM3_STATE_DTYPE).reshape(P)
    bm = np.zeros((P, cap), np.uint8) if best_masks is None else np.array(best_masks, np.uint8).reshape(P, cap)
    res = np.zeros(P, SIM3_RESULT_DTYPE)
    inl = np.zeros((P, cap), np.uint8)
    hyp = np.full((P, st.shape[1]), -1, np.int32)
    _check(lib().orbx_sim3_iterate_batch(int(device), P, cap, _p(nn), _p(T1), _p(T2), _p(w1), _p(w2), _p(m), _p(o1), _p(o2),
                                         _p(s1), len(s1), _p(s2), len(s2), _p(prm), _p(st), st.shape[1], _p(states), _p(bm),
                                         _p(res), _p(inl), _p(hyp) if want_hyp else None))
    out = (res, inl.astype(bool), states, bm)
    return out + (hyp,) if want_hyp else out


SIM3OPT_PARAMS_DTYPE = np.dtype([("model1", "<i4"), ("cam1", "<f4", (4,)), ("model2", "<i4"), ("cam2", "<f4", (4,)), ("th2", "<f4"),
                                 ("fix_scale", "<i4"), ("all_points", "<i4")])
SIM3_POSE_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])   # g2o::Sim3: r (x y z w), t, s
SIM3OPT_RESULT_DTYPE = np.dtype([("n_in", "<i4"), ("n_correspondences", "<i4"), ("n_bad", "<i4"), ("n_in_kf2", "<i4"),
                                 ("n_out_kf2", "<i4"), ("trials", "<i4"), ("early_return", "<i4")])
assert SIM3OPT_PARAMS_DTYPE.itemsize == 52 and SIM3_POSE_DTYPE.itemsize == 64 and SIM3OPT_RESULT_DTYPE.itemsize == 28


def sim3opt_params(camera1, camera2, th2, fix_scale, all_points=False, n=1):
    """orbx_sim3opt_params records: camera1 / camera2 = (fx, fy, cx, cy) of a pinhole.  Eight parameters name a KannalaBrandt8
    camera, which the library rejects (include/orbx.h says why)."""
    prm = np.zeros(n, SIM3OPT_PARAMS_DTYPE)
    for k, camera in (("1", camera1), ("2", camera2)):
        cam = np.asarray(camera, np.float32).reshape(-1)
        prm["model" + k] = CAMERA_KB8 if len(cam) == 8 else CAMERA_PINHOLE
        prm["cam" + k] = cam[:4]
    prm["th2"], prm["fix_scale"], prm["all_points"] = th2, int(bool(fix_scale)), int(bool(all_points))
    return prm


def sim3_pose(q, t, s, n=1):
    """orbx_sim3_pose records from r (x y z w), t and s."""
    S = np.zeros(n, SIM3_POSE_DTYPE)
    S["q"], S["t"], S["s"] = np.asarray(q, float), np.asarray(t, float), s
    return S


def OptimizeSim3(kpsUn1, worldPos1, worldPos2, matched, idx2, kpsUn2, trackLevel2, Tcw1, Tcw2, invLevelSigma2_1, invLevelSigma2_2,
                 g2oS12, th2, bFixScale, bAllPoints=False, camera1=None, camera2=None, device=0):
    """Optimizer::OptimizeSim3 (src/Optimizer.cc:2164-2424) on the GPU (orbx_optimize_sim3).  Over the n key points of key frame
    1: kpsUn1 [n] KP_DTYPE, worldPos1 / worldPos2 [n][3] = the map point of key frame 1 at i and vpMatches1[i], matched [n]
    (vpMatches1[i] is set, key frame 1 has a map point there, neither is bad), idx2 [n] = the index of vpMatches1[i] in key frame 2
    (< 0: not there), kpsUn2 [n2], trackLevel2 [n] = mnTrackScaleLevel (read where idx2 < 0), Tcw1 / Tcw2 (3 x 4 or 4 x 4), the two
    mvInvLevelSigma2 tables, g2oS12 = a sim3_pose record (or (q, t, s)), camera1 / camera2 = (fx, fy, cx, cy).  Returns (nIn,
    g2oS12 record, matched [n] uint8 with the cleared entries zeroed, mAcumHessian, result record).  mAcumHessian is zeros (7, 7),
    as the reference sets it and never accumulates, and None on the early return (result["early_return"]: fewer than 10 pairs left
    after round one), which the reference takes before it touches the matrix."""
    if camera1 is None or camera2 is None:
        raise ValueError("OptimizeSim3: camera1 and camera2 = (fx, fy, cx, cy) of the two key frames are required")
    m = np.array(matched, np.uint8).reshape(-1)
    n = len(m)
    k1 = np.ascontiguousarray(kpsUn1, KP_DTYPE).reshape(n)
    k2 = np.ascontiguousarray(kpsUn2, KP_DTYPE).reshape(-1)
    w1 = np.ascontiguousarray(worldPos1, np.float32).reshape(n, 3)
    w2 = np.ascontiguousarray(worldPos2, np.float32).reshape(n, 3)
    i2 = np.ascontiguousarray(idx2, np.int32).reshape(n)
    tl = np.ascontiguousarray(trackLevel2, np.int32).reshape(n)
    T1 = np.ascontiguousarray(np.asarray(Tcw1, np.float32).reshape(-1)[:12])
    T2 = np.ascontiguousarray(np.asarray(Tcw2, np.float32).reshape(-1)[:12])
    s1 = np.ascontiguousarray(invLevelSigma2_1, np.float32)
    s2 = np.ascontiguousarray(invLevelSigma2_2, np.float32)
    prm = sim3opt_params(camera1, camera2, th2, bFixScale, bAllPoints)
    S = np.array(g2oS12, SIM3_POSE_DTYPE).reshape(1) if isinstance(g2oS12, np.ndarray) else sim3_pose(*g2oS12)
    res = np.zeros(1, SIM3OPT_RESULT_DTYPE)
    nin = _check(lib().orbx_optimize_sim3(int(device), n, _p(k1), _p(w1), _p(w2), _p(m), _p(i2), _p(k2), len(k2), _p(tl), _p(T1),
                                          _p(T2), _p(s1), len(s1), _p(s2), len(s2), _p(prm), _p(S), _p(res)))
    return nin, S[0], m, None if res[0]["early_return"] else np.zeros((7, 7)), res[0]


def OptimizeSim3Batch(n, kpsUn1, worldPos1, worldPos2, matched, idx2, kpsUn2, n2, trackLevel2, Tcw1, Tcw2, invLevelSigma2_1,
                      invLevelSigma2_2, g2oS12, params, device=0):
    """OptimizeSim3 for P pairs in one launch (orbx_optimize_sim3_batch): n [P] key points per problem, kpsUn1 / matched / idx2 /
    trackLevel2 [P][cap], worldPos1 / worldPos2 [P][cap][3], kpsUn2 [P][cap2] with n2 [P] key points each, Tcw1 / Tcw2 [P][12], the
    two mvInvLevelSigma2 tables (shared), g2oS12 [P] sim3_pose records, params [P] sim3opt_params records.  Returns (results [P],
    g2oS12 [P], matched [P][cap])."""
    nn = np.ascontiguousarray(n, np.int32).reshape(-1)
    P = len(nn)
    m = np.array(matched, np.uint8).reshape(P, -1)
    cap = m.shape[1]
    k1 = np.ascontiguousarray(kpsUn1, KP_DTYPE).reshape(P, cap)
    k2 = np.ascontiguousarray(kpsUn2, KP_DTYPE).reshape(P, -1)
    nn2 = np.ascontiguousarray(n2, np.int32).reshape(P)
    w1 = np.ascontiguousarray(worldPos1, np.float32).reshape(P, cap, 3)
    w2 = np.ascontiguousarray(worldPos2, np.float32).reshape(P, cap, 3)
    i2 = np.ascontiguousarray(idx2, np.int32).reshape(P, cap)
    tl = np.ascontiguousarray(trackLevel2, np.int32).reshape(P, cap)
    T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(P, 12)
    T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(P, 12)
    s1 = np.ascontiguousarray(invLevelSigma2_1, np.float32)
    s2 = np.ascontiguousarray(invLevelSigma2_2, np.float32)
    prm = np.ascontiguousarray(params, SIM3OPT_PARAMS_DTYPE).reshape(P)
    S = np.array(g2oS12, SIM3_POSE_DTYPE).reshape(P)
    res = np.zeros(P, SIM3OPT_RESULT_DTYPE)
    _check(lib().orbx_optimize_sim3_batch(int(device), P, cap, _p(nn), _p(k1), _p(w1), _p(w2), _p(m), _p(i2), _p(k2), k2.shape[1],
                                          _p(nn2), _p(tl), _p(T1), _p(T2), _p(s1), len(s1), _p(s2), len(s2), _p(prm), _p(S), _p(res)))
    return res, S, m


# ---- inertial pose optimisation (Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame)
IMU_PREINTEGRATED_DTYPE = np.dtype([("dR", "<f4", (9,)), ("dV", "<f4", (3,)), ("dP", "<f4", (3,)), ("JRg", "<f4", (9,)),
                                    ("JVg", "<f4", (9,)), ("JVa", "<f4", (9,)), ("JPg", "<f4", (9,)), ("JPa", "<f4", (9,)),
                                    ("C", "<f4", (225,)), ("b", "<f4", (6,)), ("dT", "<f4")])   # orbx_imu_preintegrated
IMU_STATE_DTYPE = np.dtype([("Rwb", "<f8", (9,)), ("twb", "<f8", (3,)), ("vwb", "<f8", (3,)), ("bg", "<f8", (3,)),
                            ("ba", "<f8", (3,))])                                               # orbx_imu_state
IMU_PRIOR_DTYPE = np.dtype([("state", IMU_STATE_DTYPE), ("H", "<f8", (225,))])                  # orbx_imu_prior
POSE_INERTIAL_FRAME_DTYPE = np.dtype([("Rwb", "<f4", (9,)), ("twb", "<f4", (3,)), ("vwb", "<f4", (3,)), ("bias", "<f4", (6,)),
                                      ("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Rcb", "<f4", (9,)), ("tcb", "<f4", (3,)),
                                      ("tbc", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("bf", "<f4"),
                                      ("camera_model", "<i4"), ("n_cameras", "<i4")])           # orbx_pose_inertial_frame
POSE_INERTIAL_RESULT_DTYPE = np.dtype([("state", IMU_STATE_DTYPE), ("H", "<f8", (225,)), ("n_good", "<i4"), ("n_inliers_mono", "<i4"),
                                       ("n_outliers_mono", "<i4"), ("n_inliers_stereo", "<i4"), ("n_outliers_stereo", "<i4"),
                                       ("rounds", "<i4"), ("status", "<i4"), ("recovered", "<i4")])   # orbx_pose_inertial_result
assert IMU_PREINTEGRATED_DTYPE.itemsize == 1168 and IMU_STATE_DTYPE.itemsize == 168 and IMU_PRIOR_DTYPE.itemsize == 1968
assert POSE_INERTIAL_FRAME_DTYPE.itemsize == 220 and POSE_INERTIAL_RESULT_DTYPE.itemsize == 2000
PI_SOLVE_FAILED, PI_BAD_COVARIANCE = 1, 2


def _record(value, dtype, n=1):
    """n records of a structured dtype from records of it or from mappings of its fields (matrices in any shape)."""
    if isinstance(value, np.ndarray) and value.dtype == dtype:
        return np.ascontiguousarray(value).reshape(n)
    items = [value] if isinstance(value, dict) else list(value)
    out = np.zeros(n, dtype)
    if len(items) != n:
        raise ValueError("expected %d records, got %d" % (n, len(items)))
    for r, item in zip(out, items):
        for name in dtype.names:
            sub = dtype.fields[name][0]
            if sub.names:   # a nested record (orbx_imu_prior::state): its fields sit beside the outer ones in a mapping
                r[name] = _record(item[name] if name in item else item, sub)[0]
            elif name in item:
                r[name] = np.asarray(item[name]).reshape(sub.shape)
            elif name == "n_cameras":
                r[name] = 1
            elif name != "camera_model":
                raise KeyError(name)
    return out


def _pose_inertial_arrays(kpsUn, uRight, worldPos, hasPoint, trackDepth, outlier, shape):
    k = np.ascontiguousarray(kpsUn, KP_DTYPE).reshape(shape)
    ur = None if uRight is None else np.ascontiguousarray(uRight, np.float32).reshape(shape)
    w = np.ascontiguousarray(worldPos, np.float32).reshape(shape + (3,))
    h = np.ascontiguousarray(hasPoint, np.uint8).reshape(shape)
    d = np.ascontiguousarray(trackDepth, np.float32).reshape(shape)
    out = np.zeros(shape, np.uint8) if outlier is None else np.array(outlier, np.uint8).reshape(shape)
    return k, ur, w, h, d, out


def pose_inertial_optimization_last_keyframe(kpsUn, uRight, worldPos, hasPoint, trackDepth, invLevelSigma2, frame, keyframe_state,
                                             preintegrated, bRecInit=False, outlier=None, device=0):
    """Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:4544-4931) on the GPU
    (orbx_pose_inertial_optimization_last_keyframe).  Over the frame's n key points: kpsUn [n] KP_DTYPE, uRight [n] (None: every
    edge mono), worldPos [n][3], hasPoint [n], trackDepth [n] (MapPoint::mTrackDepth); frame = a POSE_INERTIAL_FRAME_DTYPE record or
    a mapping of its fields, keyframe_state = IMU_STATE_DTYPE (the last key frame's Rwb, twb, vwb, bg, ba), preintegrated =
    IMU_PREINTEGRATED_DTYPE (mpImuPreintegrated).  Returns (n_good, result record, outlier [n]): the result holds the optimised
    state (the frame takes its float casts) and the new prior's H (with the state: the frame's ConstraintPoseImu); outlier keeps
    the given values where there is no point."""
    n = len(np.asarray(hasPoint).reshape(-1))
    k, ur, w, h, d, out = _pose_inertial_arrays(kpsUn, uRight, worldPos, hasPoint, trackDepth, outlier, (n,))
    s2 = np.ascontiguousarray(invLevelSigma2, np.float32)
    fr, st = _record(frame, POSE_INERTIAL_FRAME_DTYPE), _record(keyframe_state, IMU_STATE_DTYPE)
    pre = _record(preintegrated, IMU_PREINTEGRATED_DTYPE)
    res = np.zeros(1, POSE_INERTIAL_RESULT_DTYPE)
    ng = _check(lib().orbx_pose_inertial_optimization_last_keyframe(
        int(device), _p(k), None if ur is None else _p(ur), _p(w), _p(h), _p(d), n, _p(s2), len(s2), _p(fr), _p(st), _p(pre),
        int(bool(bRecInit)), _p(out), _p(res)))
    return ng, res[0], out


def pose_inertial_optimization_last_frame(kpsUn, uRight, worldPos, hasPoint, trackDepth, invLevelSigma2, frame, prev_state, prior,
                                          preintegrated, preintegrated_frame, bRecInit=False, outlier=None, device=0):
    """Optimizer::PoseInertialOptimizationLastFrame (src/Optimizer.cc:4933-5356) on the GPU
    (orbx_pose_inertial_optimization_last_frame): as the last key-frame call, with prev_state = the previous frame's estimate
    (IMU_STATE_DTYPE), prior = its ConstraintPoseImu (IMU_PRIOR_DTYPE, or a mapping with Rwb .. ba and H), preintegrated =
    mpImuPreintegrated (the walk edges) and preintegrated_frame = mpImuPreintegratedFrame (the inertial edge).  The caller drops
    the previous frame's prior afterwards, as the reference does."""
    n = len(np.asarray(hasPoint).reshape(-1))
    k, ur, w, h, d, out = _pose_inertial_arrays(kpsUn, uRight, worldPos, hasPoint, trackDepth, outlier, (n,))
    s2 = np.ascontiguousarray(invLevelSigma2, np.float32)
    fr, st, pr = _record(frame, POSE_INERTIAL_FRAME_DTYPE), _record(prev_state, IMU_STATE_DTYPE), _record(prior, IMU_PRIOR_DTYPE)
    pre, pref = _record(preintegrated, IMU_PREINTEGRATED_DTYPE), _record(preintegrated_frame, IMU_PREINTEGRATED_DTYPE)
    res = np.zeros(1, POSE_INERTIAL_RESULT_DTYPE)
    ng = _check(lib().orbx_pose_inertial_optimization_last_frame(
        int(device), _p(k), None if ur is None else _p(ur), _p(w), _p(h), _p(d), n, _p(s2), len(s2), _p(fr), _p(st), _p(pr), _p(pre),
        _p(pref), int(bool(bRecInit)), _p(out), _p(res)))
    return ng, res[0], out


def pose_inertial_optimization_batch(n, kpsUn, uRight, worldPos, hasPoint, trackDepth, invLevelSigma2, frames, states, preintegrated,
                                     bRecInit, priors=None, preintegrated_frame=None, outlier=None, device=0):
    """P problems in one launch: orbx_pose_inertial_optimization_last_keyframe_batch, or _last_frame_batch when priors (and
    preintegrated_frame) are given.  n [P] key points per problem, kpsUn / uRight (or None) / hasPoint / trackDepth [P][cap],
    worldPos [P][cap][3], frames / states / records / bRecInit [P].  Returns (results [P], outlier [P][cap]); problem p has the
    bits of the one-shot call on the same data."""
    nn = np.ascontiguousarray(n, np.int32).reshape(-1)
    P = len(nn)
    cap = np.asarray(hasPoint).reshape(P, -1).shape[1]
    k, ur, w, h, d, out = _pose_inertial_arrays(kpsUn, uRight, worldPos, hasPoint, trackDepth, outlier, (P, cap))
    s2 = np.ascontiguousarray(invLevelSigma2, np.float32)
    fr, st = _record(frames, POSE_INERTIAL_FRAME_DTYPE, P), _record(states, IMU_STATE_DTYPE, P)
    pre = _record(preintegrated, IMU_PREINTEGRATED_DTYPE, P)
    rec = np.ascontiguousarray(bRecInit, np.int32).reshape(P)
    res = np.zeros(P, POSE_INERTIAL_RESULT_DTYPE)
    head = (int(device), P, cap, _p(nn), _p(k), None if ur is None else _p(ur), _p(w), _p(h), _p(d), _p(s2), len(s2), _p(fr), _p(st))
    if priors is None:
        _check(lib().orbx_pose_inertial_optimization_last_keyframe_batch(*head, _p(pre), _p(rec), _p(out), _p(res)))
    else:
        pr, pref = _record(priors, IMU_PRIOR_DTYPE, P), _record(preintegrated_frame, IMU_PREINTEGRATED_DTYPE, P)
        _check(lib().orbx_pose_inertial_optimization_last_frame_batch(*head, _p(pr), _p(pre), _p(pref), _p(rec), _p(out), _p(res)))
    return res, out


def pose_inertial_optimization_last_keyframe_batch(n, kpsUn, uRight, worldPos, hasPoint, trackDepth, invLevelSigma2, frames,
                                                   keyframe_states, preintegrated, bRecInit, outlier=None, device=0):
    return pose_inertial_optimization_batch(n, kpsUn, uRight, worldPos, hasPoint, trackDepth, invLevelSigma2, frames, keyframe_states,
                                            preintegrated, bRecInit, outlier=outlier, device=device)


def pose_inertial_optimization_last_frame_batch(n, kpsUn, uRight, worldPos, hasPoint, trackDepth, invLevelSigma2, frames, prev_states,
                                                priors, preintegrated, preintegrated_frame, bRecInit, outlier=None, device=0):
    return pose_inertial_optimization_batch(n, kpsUn, uRight, worldPos, hasPoint, trackDepth, invLevelSigma2, frames, prev_states,
                                            preintegrated, bRecInit, priors=priors, preintegrated_frame=preintegrated_frame,
                                            outlier=outlier, device=device)


# orbx_debug_inertial_linalg: ORBX_ILA_* and, per operation, the doubles of one item of `in` and of `out`
(ILA_LDLT15, ILA_LDLT30, ILA_EIG9, ILA_EIG15, ILA_CLAMP15, ILA_PINV15, ILA_INVERSE9, ILA_EXP_SO3, ILA_LOG_SO3, ILA_JR, ILA_JR_INV,
 ILA_NORMALIZE_F) = range(12)
ILA_OPS, ILA_MAX_ITEMS = 12, 4096
ILA_ITEM = {ILA_LDLT15: (240, 16), ILA_LDLT30: (930, 31), ILA_EIG9: (81, 90), ILA_EIG15: (225, 240), ILA_CLAMP15: (225, 225),
            ILA_PINV15: (225, 225), ILA_INVERSE9: (81, 82), ILA_EXP_SO3: (3, 9), ILA_LOG_SO3: (9, 3), ILA_JR: (3, 9),
            ILA_JR_INV: (3, 9), ILA_NORMALIZE_F: (9, 9)}


def debug_inertial_linalg(op, items, prefill=0.0, device=0):
    """One of the inertial solvers' pieces of csrc/orbx_linalg.h alone on the device (orbx_debug_inertial_linalg): items
    [n][doubles of one input item] -> [n][doubles of one output item]; prefill is what `out` holds going in."""
    n_in, n_out = ILA_ITEM[op]
    a = np.ascontiguousarray(items, np.float64).reshape(-1, n_in)
    out = np.empty((len(a), n_out), np.float64)
    out[...] = prefill
    _check(lib().orbx_debug_inertial_linalg(int(device), int(op), len(a), _p(a), _p(out)))
    return out


# ---- local bundle adjustment (Optimizer::LocalBundleAdjustment)
LBA_KEYFRAME_DTYPE = np.dtype([("q", "<f4", (4,)), ("t", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                               ("bf", "<f4"), ("model", "<i4"), ("fixed", "<i4"), ("camera2", "<i4")])
LBA_EDGE_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"), ("u_right", "<f4"), ("inv_sigma2", "<f4")])
assert LBA_KEYFRAME_DTYPE.itemsize == 60 and LBA_EDGE_DTYPE.itemsize == 24
LBA_MAX_LOCAL = 128
LBA_DONE, LBA_ABORTED, LBA_STOPPED, LBA_EMPTY = 0, 1, 2, 3
LBA_STOP_ITERATIONS, LBA_STOP_QMAX, LBA_STOP_RHO_ZERO, LBA_STOP_SMALL_GAIN = 0, 1, 2, 3


class _LbaProblem(C.Structure):    # orbx_lba_problem
    _fields_ = [("keyframes", C.c_void_p), ("points", C.c_void_p), ("edges", C.c_void_p), ("n_local", C.c_int32),
                ("n_fixed", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32)]


class _LbaParams(C.Structure):     # orbx_lba_params
    _fields_ = [("max_iterations", C.c_int32), ("stop", C.c_int32), ("lambda_init", C.c_float)]


class _LbaResult(C.Structure):     # orbx_lba_result
    _fields_ = [("poses", C.c_void_p), ("points", C.c_void_p), ("erase", C.c_void_p), ("chi2", C.c_void_p),
                ("depth_positive", C.c_void_p), ("num_fixedKF", C.c_int32), ("num_OptKF", C.c_int32), ("num_MPs", C.c_int32),
                ("num_edges", C.c_int32), ("status", C.c_int32), ("iterations", C.c_int32), ("trials", C.c_int32),
                ("stop_reason", C.c_int32), ("lambda_", C.c_double), ("chi2_initial", C.c_double), ("chi2_final", C.c_double)]


def lba_keyframes(q, t, cam, fixed, model=CAMERA_PINHOLE, camera2=0):
    """orbx_lba_keyframe records: q [n][4] (x y z w) and t [n][3] of Tcw, cam = (fx, fy, cx, cy, bf) for all or [n][5], fixed [n]."""
    q = np.asarray(q, np.float32).reshape(-1, 4)
    k = np.zeros(len(q), LBA_KEYFRAME_DTYPE)
    k["q"], k["t"] = q, np.asarray(t, np.float32).reshape(-1, 3)
    cam = np.broadcast_to(np.asarray(cam, np.float32), (len(q), 5))
    for j, name in enumerate(("fx", "fy", "cx", "cy", "bf")):
        k[name] = cam[:, j]
    k["fixed"], k["model"], k["camera2"] = fixed, model, camera2
    return k


def LocalBundleAdjustment(keyframes, n_local, points, edges, max_iterations=10, lambda_init=0.0, stop=False, device=0):
    """Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1109-1516) on the GPU (orbx_local_bundle_adjustment) over the flat graph
    of include/orbx.h: keyframes = LBA_KEYFRAME_DTYPE records, the n_local local key frames first and the fixed ones behind them;
    points [nP][3] float; edges = LBA_EDGE_DTYPE records in the reference's order (grouped by ascending point).  lambda_init = 100
    for an inertial map; stop = *pbStopFlag.  Returns a dict: poses [n_local][7] double (q x y z w, t), points [nP][3] double, erase /
    depth_positive [nE] uint8, chi2 [nE] double (what every edge holds after the last trial), and the counters num_fixedKF,
    num_OptKF, num_MPs, num_edges, status (LBA_DONE / LBA_ABORTED / LBA_STOPPED / LBA_EMPTY), iterations, trials, stop_reason, lambda,
    chi2_initial, chi2_final.  The caller applies SetPose / SetWorldPos with the float casts and erases the flagged observations."""
    kf = np.ascontiguousarray(keyframes, LBA_KEYFRAME_DTYPE).reshape(-1)
    X = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    ed = np.ascontiguousarray(edges, LBA_EDGE_DTYPE).reshape(-1)
    n_local = int(n_local)
    poses, pts = np.zeros((max(n_local, 0), 7)), np.zeros((len(X), 3))
    erase, depth, chi2 = np.zeros(len(ed), np.uint8), np.zeros(len(ed), np.uint8), np.zeros(len(ed))
    prob = _LbaProblem(_p(kf).value, _p(X).value, _p(ed).value, n_local, len(kf) - n_local, len(X), len(ed))
    prm = _LbaParams(int(max_iterations), int(bool(stop)), float(lambda_init))
    res = _LbaResult(_p(poses).value, _p(pts).value, _p(erase).value, _p(chi2).value, _p(depth).value)
    _check(lib().orbx_local_bundle_adjustment(int(device), C.byref(prob), C.byref(prm), C.byref(res)))
    out = dict(poses=poses, points=pts, erase=erase, chi2=chi2, depth_positive=depth)
    for name in ("num_fixedKF", "num_OptKF", "num_MPs", "num_edges", "status", "iterations", "trials", "stop_reason", "chi2_initial",
                 "chi2_final"):
        out[name] = getattr(res, name)
    out["lambda"] = res.lambda_
    return out


# ---- full bundle adjustment (Optimizer::GlobalBundleAdjustemnt)
BA_MAX_KF = 1024
BA_BLOCKED_FROM_KF = 63
BA_SOLVER_AUTO, BA_SOLVER_BLOCKED, BA_SOLVER_ONE_WORKGROUP = 0, 1, 2


class _BaParams(C.Structure):      # orbx_ba_params
    _fields_ = [("max_iterations", C.c_int32), ("robust", C.c_int32), ("lambda_init", C.c_float), ("solver", C.c_int32),
                ("stop_flag", C.c_void_p)]


class _BaResult(C.Structure):      # orbx_ba_result
    _fields_ = [("poses", C.c_void_p), ("points", C.c_void_p), ("chi2", C.c_void_p), ("status", C.c_int32), ("iterations", C.c_int32),
                ("trials", C.c_int32), ("stop_reason", C.c_int32), ("lambda_", C.c_double), ("chi2_initial", C.c_double),
                ("chi2_final", C.c_double)]


def BundleAdjustment(keyframes, points, edges, max_iterations=5, robust=True, lambda_init=0.0, stop=None, solver=0, device=0):
    """Optimizer::BundleAdjustment (src/Optimizer.cc:47-372, behind GlobalBundleAdjustemnt) on the GPU (orbx_bundle_adjustment):
    keyframes = LBA_KEYFRAME_DTYPE records in vpKFs order (fixed != 0: the map's initial key frame), points [nP][3] float in vpMP
    order, edges = LBA_EDGE_DTYPE records grouped by ascending point.  robust: Huber kernels with the deltas of :129.  stop: None, or
    a one-element int32 numpy array the caller may set from another thread while the call runs (pbStopFlag).  solver: BA_SOLVER_*.
    Returns a dict: poses [nKF][7] double (q x y z w, t), points [nP][3] double, chi2 [nE] double, status (LBA_DONE / LBA_STOPPED /
    LBA_EMPTY), iterations, trials, stop_reason, lambda, chi2_initial, chi2_final."""
    kf = np.ascontiguousarray(keyframes, LBA_KEYFRAME_DTYPE).reshape(-1)
    X = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    ed = np.ascontiguousarray(edges, LBA_EDGE_DTYPE).reshape(-1)
    if stop is not None and not (isinstance(stop, np.ndarray) and stop.dtype == np.int32 and stop.size == 1):
        raise TypeError("stop must be None or a one-element int32 numpy array")
    # the fixed key frames need not come last in vpKFs: every key frame counts as local, the fixed flag says which stay
    poses, pts, chi2 = np.zeros((len(kf), 7)), np.zeros((len(X), 3)), np.zeros(len(ed))
    prob = _LbaProblem(_p(kf).value, _p(X).value, _p(ed).value, len(kf), 0, len(X), len(ed))
    prm = _BaParams(int(max_iterations), int(bool(robust)), float(lambda_init), int(solver), None if stop is None else _p(stop).value)
    res = _BaResult(_p(poses).value, _p(pts).value, _p(chi2).value)
    _check(lib().orbx_bundle_adjustment(int(device), C.byref(prob), C.byref(prm), C.byref(res)))
    out = dict(poses=poses, points=pts, chi2=chi2)
    for name in ("status", "iterations", "trials", "stop_reason", "chi2_initial", "chi2_final"):
        out[name] = getattr(res, name)
    out["lambda"] = res.lambda_
    return out


# ---- bundle adjustments of KannalaBrandt8 key frames and two-camera rigs
CAMERA_NONE = -1
LBA_RIG_CAMERA_DTYPE = np.dtype([("k", "<f4", (4,)), ("model2", "<i4"), ("p2", "<f4", (8,)), ("trl_q", "<f4", (4,)),
                                 ("trl_t", "<f4", (3,))])
assert LBA_RIG_CAMERA_DTYPE.itemsize == 80


class _LbaRigProblem(C.Structure):   # orbx_lba_rig_problem
    _fields_ = [("base", _LbaProblem), ("cams", C.c_void_p), ("edge_camera", C.c_void_p)]


def lba_rig_cameras(n, k=None, model2=CAMERA_NONE, p2=None, trl_q=(0, 0, 0, 1), trl_t=(0, 0, 0)):
    """orbx_lba_rig_camera records for n key frames: k = the left camera's KB8 mvParameters[4..7] ([4] for all or [n][4]), model2 and
    p2 = the second camera's model (CAMERA_NONE / CAMERA_PINHOLE / CAMERA_KB8) and its eight mvParameters, trl_q (x y z w) / trl_t =
    GetRelativePoseTrl().  Whether a key frame uses its second camera is lba_keyframes' camera2."""
    c = np.zeros(int(n), LBA_RIG_CAMERA_DTYPE)
    c["k"] = 0 if k is None else np.broadcast_to(np.asarray(k, np.float32), (len(c), 4))
    c["model2"] = model2
    c["p2"] = 0 if p2 is None else np.broadcast_to(np.asarray(p2, np.float32), (len(c), 8))
    c["trl_q"] = np.broadcast_to(np.asarray(trl_q, np.float32), (len(c), 4))
    c["trl_t"] = np.broadcast_to(np.asarray(trl_t, np.float32), (len(c), 3))
    return c


def _lba_rig_problem(kf, X, ed, cams, edge_camera, n_local):
    cm = np.ascontiguousarray(cams, LBA_RIG_CAMERA_DTYPE).reshape(-1)
    ec = np.ascontiguousarray(edge_camera, np.uint8).reshape(-1)
    if len(cm) != len(kf) or len(ec) != len(ed):
        raise ValueError("cams must have one record per key frame and edge_camera one entry per edge")
    prob = _LbaRigProblem(_LbaProblem(_p(kf).value, _p(X).value, _p(ed).value, n_local, len(kf) - n_local, len(X), len(ed)),
                          _p(cm).value, _p(ec).value)
    return prob, (cm, ec)


def LocalBundleAdjustmentRig(keyframes, cams, n_local, points, edges, edge_camera, max_iterations=10, lambda_init=0.0, stop=False,
                             device=0):
    """LocalBundleAdjustment for KannalaBrandt8 key frames and two-camera rigs (orbx_local_bundle_adjustment_rig): the arguments of
    LocalBundleAdjustment plus cams = LBA_RIG_CAMERA_DTYPE records, one per key frame (lba_rig_cameras), and edge_camera [nE] uint8 (0
    an observation of the left camera, 1 of the second one: an EdgeSE3ProjectXYZToBody edge).  keyframes["model"] may be CAMERA_KB8 and
    keyframes["camera2"] says whether the second camera is used.  Returns LocalBundleAdjustment's dict."""
    kf = np.ascontiguousarray(keyframes, LBA_KEYFRAME_DTYPE).reshape(-1)
    X = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    ed = np.ascontiguousarray(edges, LBA_EDGE_DTYPE).reshape(-1)
    n_local = int(n_local)
    prob, keep = _lba_rig_problem(kf, X, ed, cams, edge_camera, n_local)
    poses, pts = np.zeros((max(n_local, 0), 7)), np.zeros((len(X), 3))
    erase, depth, chi2 = np.zeros(len(ed), np.uint8), np.zeros(len(ed), np.uint8), np.zeros(len(ed))
    prm = _LbaParams(int(max_iterations), int(bool(stop)), float(lambda_init))
    res = _LbaResult(_p(poses).value, _p(pts).value, _p(erase).value, _p(chi2).value, _p(depth).value)
    _check(lib().orbx_local_bundle_adjustment_rig(int(device), C.byref(prob), C.byref(prm), C.byref(res)))
    out = dict(poses=poses, points=pts, erase=erase, chi2=chi2, depth_positive=depth)
    for name in ("num_fixedKF", "num_OptKF", "num_MPs", "num_edges", "status", "iterations", "trials", "stop_reason", "chi2_initial",
                 "chi2_final"):
        out[name] = getattr(res, name)
    out["lambda"] = res.lambda_
    return out


# ---- map-merge bundle adjustment (the welding BA of LoopClosing::MergeLocal)
class _MbaParams(C.Structure):     # orbx_mba_params
    _fields_ = [("iterations_first", C.c_int32), ("iterations_second", C.c_int32), ("lambda_init", C.c_float), ("reserved", C.c_int32),
                ("stop_flag", C.c_void_p)]


class _MbaResult(C.Structure):     # orbx_mba_result
    _fields_ = [("poses", C.c_void_p), ("points", C.c_void_p), ("erase", C.c_void_p), ("chi2", C.c_void_p),
                ("depth_positive", C.c_void_p), ("level", C.c_void_p), ("status", C.c_int32), ("rounds", C.c_int32),
                ("n_level1", C.c_int32), ("reserved", C.c_int32), ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2),
                ("stop_reason", C.c_int32 * 2), ("lambda_", C.c_double * 2), ("chi2_initial", C.c_double * 2),
                ("chi2_final", C.c_double * 2)]


def _merge_ba(entry, prob, n_local, nP, nE, iterations_first, iterations_second, lambda_init, stop, device):
    if stop is not None and not (isinstance(stop, np.ndarray) and stop.dtype == np.int32 and stop.size == 1):
        raise TypeError("stop must be None or a one-element int32 numpy array")
    fn = getattr(lib(), entry)
    poses, pts = np.zeros((max(n_local, 0), 7)), np.zeros((nP, 3))
    erase, depth, level, chi2 = np.zeros(nE, np.uint8), np.zeros(nE, np.uint8), np.zeros(nE, np.uint8), np.zeros(nE)
    prm = _MbaParams(int(iterations_first), int(iterations_second), float(lambda_init), 0, None if stop is None else _p(stop).value)
    res = _MbaResult(_p(poses).value, _p(pts).value, _p(erase).value, _p(chi2).value, _p(depth).value, _p(level).value)
    _check(fn(int(device), C.byref(prob), C.byref(prm), C.byref(res)))
    out = dict(poses=poses, points=pts, erase=erase, chi2=chi2, depth_positive=depth, level=level, status=res.status, rounds=res.rounds,
               n_level1=res.n_level1)
    for name in ("iterations", "trials", "stop_reason", "chi2_initial", "chi2_final"):
        out[name] = list(getattr(res, name))
    out["lambda"] = list(res.lambda_)
    return out


def merge_bundle_adjustment(keyframes, n_adjust, points, edges, iterations_first=5, iterations_second=10, lambda_init=0.0, stop=None,
                            device=0):
    """The map-merge Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) (src/Optimizer.cc:3567-3994) on the
    GPU (orbx_merge_bundle_adjustment): keyframes = LBA_KEYFRAME_DTYPE records, the n_adjust key frames of vpAdjustKF first (fixed ==
    0), those of vpFixedKF behind them (fixed != 0, there may be none); points [nP][3] float; edges = LBA_EDGE_DTYPE records grouped
    by ascending point.  stop: None, or a one-element int32 numpy array (pbStopFlag) as BundleAdjustment takes it.  Returns a dict:
    poses [n_adjust][7] double, points [nP][3] double, erase / depth_positive / level [nE] uint8, chi2 [nE] double, status (LBA_DONE /
    LBA_STOPPED / LBA_EMPTY), rounds, n_level1 and, per round as lists of two, iterations, trials, stop_reason, lambda, chi2_initial,
    chi2_final."""
    kf = np.ascontiguousarray(keyframes, LBA_KEYFRAME_DTYPE).reshape(-1)
    X = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    ed = np.ascontiguousarray(edges, LBA_EDGE_DTYPE).reshape(-1)
    n_adjust = int(n_adjust)
    prob = _LbaProblem(_p(kf).value, _p(X).value, _p(ed).value, n_adjust, len(kf) - n_adjust, len(X), len(ed))
    return _merge_ba("orbx_merge_bundle_adjustment", prob, n_adjust, len(X), len(ed), iterations_first, iterations_second, lambda_init,
                     stop, device)


def merge_bundle_adjustment_rig(keyframes, cams, n_adjust, points, edges, edge_camera, iterations_first=5, iterations_second=10,
                                lambda_init=0.0, stop=None, device=0):
    """merge_bundle_adjustment for KannalaBrandt8 left cameras (orbx_merge_bundle_adjustment_rig): plus cams and edge_camera as
    LocalBundleAdjustmentRig takes them; this overload builds no second-camera edge, so edge_camera must be all zero."""
    kf = np.ascontiguousarray(keyframes, LBA_KEYFRAME_DTYPE).reshape(-1)
    X = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    ed = np.ascontiguousarray(edges, LBA_EDGE_DTYPE).reshape(-1)
    n_adjust = int(n_adjust)
    prob, keep = _lba_rig_problem(kf, X, ed, cams, edge_camera, n_adjust)
    return _merge_ba("orbx_merge_bundle_adjustment_rig", prob, n_adjust, len(X), len(ed), iterations_first, iterations_second,
                     lambda_init, stop, device)


def BundleAdjustmentRig(keyframes, cams, points, edges, edge_camera, max_iterations=5, robust=True, lambda_init=0.0, stop=None,
                        solver=0, device=0):
    """BundleAdjustment for KannalaBrandt8 key frames and two-camera rigs (orbx_bundle_adjustment_rig): the arguments of
    BundleAdjustment plus cams and edge_camera as LocalBundleAdjustmentRig takes them.  Returns BundleAdjustment's dict."""
    kf = np.ascontiguousarray(keyframes, LBA_KEYFRAME_DTYPE).reshape(-1)
    X = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    ed = np.ascontiguousarray(edges, LBA_EDGE_DTYPE).reshape(-1)
    if stop is not None and not (isinstance(stop, np.ndarray) and stop.dtype == np.int32 and stop.size == 1):
        raise TypeError("stop must be None or a one-element int32 numpy array")
    prob, keep = _lba_rig_problem(kf, X, ed, cams, edge_camera, len(kf))
    poses, pts, chi2 = np.zeros((len(kf), 7)), np.zeros((len(X), 3)), np.zeros(len(ed))
    prm = _BaParams(int(max_iterations), int(bool(robust)), float(lambda_init), int(solver), None if stop is None else _p(stop).value)
    res = _BaResult(_p(poses).value, _p(pts).value, _p(chi2).value)
    _check(lib().orbx_bundle_adjustment_rig(int(device), C.byref(prob), C.byref(prm), C.byref(res)))
    out = dict(poses=poses, points=pts, chi2=chi2)
    for name in ("status", "iterations", "trials", "stop_reason", "chi2_initial", "chi2_final"):
        out[name] = getattr(res, name)
    out["lambda"] = res.lambda_
    return out


def ba_dense_solve(A, b, device=0):
    """The blocked LDLT of the full bundle adjustment alone (orbx_ba_dense_solve): A [n][n] symmetric positive definite, b [n], in
    double.  Returns dict(x [n], ok); ok == 0: a pivot was <= 0 or not finite and x is the zeros it was created with."""
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64).reshape(-1)
    if A.ndim != 2 or A.shape != (len(b), len(b)):
        raise ValueError("A must be [n][n] and b [n]")
    x = np.zeros(len(b))
    ok = C.c_int32(-1)
    _check(lib().orbx_ba_dense_solve(int(device), len(b), _p(A), _p(b), _p(x), C.byref(ok)))
    return dict(x=x, ok=ok.value)


def lba_dense_solve(A, b, device=0):
    """The one-workgroup LDLT of the local bundle adjustment alone (orbx_lba_dense_solve): as ba_dense_solve, n a multiple of 6 up
    to 6 * LBA_MAX_LOCAL."""
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64).reshape(-1)
    if A.ndim != 2 or A.shape != (len(b), len(b)):
        raise ValueError("A must be [n][n] and b [n]")
    x = np.zeros(len(b))
    ok = C.c_int32(-1)
    _check(lib().orbx_lba_dense_solve(int(device), len(b), _p(A), _p(b), _p(x), C.byref(ok)))
    return dict(x=x, ok=ok.value)


# ---- Sim3 pose graph (Optimizer::OptimizeEssentialGraph)
PG_MAX_KF = 877
PG_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("Sji", SIM3_POSE_DTYPE)])
assert PG_EDGE_DTYPE.itemsize == 72


class _PgProblem(C.Structure):     # orbx_pg_problem
    _fields_ = [("vertices", C.c_void_p), ("fixed", C.c_void_p), ("n_vertices", C.c_int32), ("edges", C.c_void_p),
                ("n_edges", C.c_int32), ("fix_scale", C.c_int32), ("points", C.c_void_p), ("point_ref", C.c_void_p),
                ("n_points", C.c_int32)]


class _PgParams(C.Structure):      # orbx_pg_params
    _fields_ = [("max_iterations", C.c_int32), ("lambda_init", C.c_double)]


class _PgResult(C.Structure):      # orbx_pg_result
    _fields_ = [("vertices", C.c_void_p), ("points", C.c_void_p), ("chi2", C.c_void_p), ("status", C.c_int32),
                ("iterations", C.c_int32), ("trials", C.c_int32), ("stop_reason", C.c_int32), ("lambda_", C.c_double),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double)]


def pg_edges(i, j, Sji):
    """orbx_pg_edge records: vertex 0 = i, vertex 1 = j, the measurements as SIM3_POSE_DTYPE records."""
    i = np.asarray(i, np.int32).reshape(-1)
    e = np.zeros(len(i), PG_EDGE_DTYPE)
    e["i"], e["j"] = i, np.asarray(j, np.int32).reshape(-1)
    e["Sji"] = np.asarray(Sji, SIM3_POSE_DTYPE).reshape(-1)
    return e


def _pg_problem(vertices, fixed, edges, fix_scale, points, point_ref):
    V = np.ascontiguousarray(vertices, SIM3_POSE_DTYPE).reshape(-1)
    fx = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    if len(fx) != len(V):
        raise ValueError("fixed must have one entry per vertex")
    ed = np.ascontiguousarray(edges, PG_EDGE_DTYPE).reshape(-1)
    X = ref = None
    if points is not None:
        X = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        ref = np.ascontiguousarray(point_ref, np.int32).reshape(-1)
        if len(ref) != len(X):
            raise ValueError("point_ref must have one entry per point")
    prob = _PgProblem(_p(V).value, _p(fx).value, len(V), _p(ed).value, len(ed), int(bool(fix_scale)),
                      None if X is None else _p(X).value, None if X is None else _p(ref).value, 0 if X is None else len(X))
    return prob, (V, fx, ed, X, ref)


def OptimizeEssentialGraph(vertices, fixed, edges, bFixScale, points=None, point_ref=None, max_iterations=20, lambda_init=1e-16,
                           device=0):
    """The optimiser and the map-point correction of the loop-closing Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1530-1826)
    on the GPU (orbx_optimize_pose_graph) over the flat graph of include/orbx.h: vertices = SIM3_POSE_DTYPE records (Siw), fixed
    [nV], edges = PG_EDGE_DTYPE records in the reference's order, points [nP][3] float with point_ref [nP] (the vertex each is
    corrected through, -1: left alone), both optional.  Returns a dict: vertices [nV] SIM3_POSE_DTYPE (the double Sim3; the caller
    recovers [R | t / s]), points [nP][3] float32 (None without points; a point with reference -1 keeps its input), chi2 [nE] at
    the returned estimate, status (LBA_DONE / LBA_EMPTY), iterations, trials, stop_reason (LBA_STOP_*), lambda, chi2_initial,
    chi2_final."""
    prob, keep = _pg_problem(vertices, fixed, edges, bFixScale, points, point_ref)
    V, ed, X = keep[0], keep[2], keep[3]
    outV, chi2 = np.zeros(len(V), SIM3_POSE_DTYPE), np.zeros(len(ed))
    outX = None if X is None else X.copy()
    prm = _PgParams(int(max_iterations), float(lambda_init))
    res = _PgResult(_p(outV).value, None if outX is None else _p(outX).value, _p(chi2).value)
    _check(lib().orbx_optimize_pose_graph(int(device), C.byref(prob), C.byref(prm), C.byref(res)))
    out = dict(vertices=outV, points=outX, chi2=chi2)
    for name in ("status", "iterations", "trials", "stop_reason", "chi2_initial", "chi2_final"):
        out[name] = getattr(res, name)
    out["lambda"] = res.lambda_
    return out


def pose_graph_evaluate(vertices, fixed, edges, bFixScale, jacobians=True, device=0):
    """orbx_pose_graph_evaluate: the errors [nE][7] of the edges at the given vertices and, with jacobians, both numeric Jacobians
    [nE][2][7][7] (vertex i, vertex j; zero for a fixed vertex) as the optimiser's first linearisation computes them."""
    prob, keep = _pg_problem(vertices, fixed, edges, bFixScale, None, None)
    nE = len(keep[2])
    err = np.zeros((nE, 7))
    jac = np.zeros((nE, 2, 7, 7)) if jacobians else None
    _check(lib().orbx_pose_graph_evaluate(int(device), C.byref(prob), _p(err), None if jac is None else _p(jac)))
    return (err, jac) if jacobians else err


# orbx_debug_linalg: ORBX_LINALG_* and, per operation, the numpy type and the elements of one item of `in` and of `out`
(LINALG_RCP64, LINALG_RSQRT64, LINALG_JACOBI_CS, LINALG_SVD3, LINALG_NULL_VECTOR4, LINALG_LDLT6, LINALG_LDLT6_DAMPED, LINALG_LDLT7,
 LINALG_NULL_VECTOR_SYM9, LINALG_NULL_VECTOR_SYM12, LINALG_SUM16, LINALG_HUBER, LINALG_LM_STEP) = range(13)
LINALG_OPS, LINALG_MAX_ITEMS = 13, 65536
LINALG_ITEM = {LINALG_RCP64: (np.float64, 1, 1), LINALG_RSQRT64: (np.float64, 1, 1), LINALG_JACOBI_CS: (np.float64, 3, 3),
               LINALG_SVD3: (np.float64, 9, 21), LINALG_NULL_VECTOR4: (np.float32, 16, 4), LINALG_LDLT6: (np.float64, 27, 7),
               LINALG_LDLT6_DAMPED: (np.float64, 28, 7), LINALG_LDLT7: (np.float64, 36, 8), LINALG_NULL_VECTOR_SYM9: (np.float64, 144, 36),
               LINALG_NULL_VECTOR_SYM12: (np.float64, 192, 48), LINALG_SUM16: (np.float64, 64, 64),
               LINALG_HUBER: (np.float64, 3, 2), LINALG_LM_STEP: (np.float64, 11, 10)}


def debug_linalg(op, items, prefill=0.0, device=0):
    """One function of csrc/orbx_linalg.h alone on the device (orbx_debug_linalg): items [n][elements of one input item] ->
    [n][elements of one output item].  prefill (a scalar or an array of the output's shape) is what `out` holds going in: it comes
    back wherever the function leaves an output untouched."""
    dt, n_in, n_out = LINALG_ITEM[op]
    a = np.ascontiguousarray(items, dt).reshape(-1, n_in)
    out = np.empty((len(a), n_out), dt)
    out[...] = prefill
    _check(lib().orbx_debug_linalg(int(device), int(op), len(a), _p(a), _p(out)))
    return out


# orbx_debug_geometry: ORBX_GEOM_* and, per operation, the numpy type and the elements of one item of `in` and of `out`
(GEOM_CAM_PROJECT, GEOM_CAM_UNPROJECT, GEOM_CAM_UNPROJECT_ROUNDED_TAN, GEOM_KB8_PROJECT_D, GEOM_KB8_PROJECT_JAC, GEOM_SE3_MAP,
 GEOM_SE3_COMPOSE, GEOM_QMUL, GEOM_QROT, GEOM_NORMALIZE_ROTATION, GEOM_QUAT_FROM_R, GEOM_OPLUS, GEOM_SIM3_EXP, GEOM_SIM3_OPLUS,
 GEOM_SO_INVERSE, GEOM_RODRIGUES2ROT, GEOM_ROT2RODRIGUES) = range(17)
GEOM_OPS, GEOM_MAX_ITEMS = 17, 65536
GEOM_ITEM = {GEOM_CAM_PROJECT: (np.float32, 12, 2), GEOM_CAM_UNPROJECT: (np.float32, 12, 3),
             GEOM_CAM_UNPROJECT_ROUNDED_TAN: (np.float32, 12, 3), GEOM_KB8_PROJECT_D: (np.float64, 7, 2),
             GEOM_KB8_PROJECT_JAC: (np.float64, 7, 6), GEOM_SE3_MAP: (np.float64, 10, 3), GEOM_SE3_COMPOSE: (np.float64, 14, 7),
             GEOM_QMUL: (np.float64, 8, 4), GEOM_QROT: (np.float64, 7, 3), GEOM_NORMALIZE_ROTATION: (np.float64, 4, 4),
             GEOM_QUAT_FROM_R: (np.float64, 9, 4), GEOM_OPLUS: (np.float64, 13, 7), GEOM_SIM3_EXP: (np.float64, 7, 8),
             GEOM_SIM3_OPLUS: (np.float64, 16, 8), GEOM_SO_INVERSE: (np.float64, 8, 17), GEOM_RODRIGUES2ROT: (np.float64, 3, 9),
             GEOM_ROT2RODRIGUES: (np.float64, 9, 3)}


def geom_kb8_items(k, X):
    """Items of GEOM_KB8_PROJECT_D / _JAC: k [n][8] float32 in the first 32 bytes, X [n][3] float64 behind them, as [n][7] doubles."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    items = np.empty((len(X), 7), np.float64)
    items[:, :4].view(np.float32)[...] = np.broadcast_to(np.asarray(k, np.float32).reshape(-1, 8), (len(X), 8))
    items[:, 4:] = X
    return items


def debug_geometry(op, items, prefill=0.0, device=0):
    """One camera model or SE3 / Sim3 map of the solvers alone on the device (orbx_debug_geometry): items [n][elements of one
    input item] -> [n][elements of one output item]; prefill is what `out` holds going in."""
    dt, n_in, n_out = GEOM_ITEM[op]
    a = np.ascontiguousarray(items, dt).reshape(-1, n_in)
    out = np.empty((len(a), n_out), dt)
    out[...] = prefill
    _check(lib().orbx_debug_geometry(int(device), int(op), len(a), _p(a), _p(out)))
    return out


class _NpCamera(C.Structure):      # orbx_np_camera
    _fields_ = [("model", C.c_int32), ("p", C.c_float * 8), ("kb8_precision", C.c_float), ("Tcw", C.c_float * 12),
                ("Ow", C.c_float * 3)]


class _NpKeyFrame(C.Structure):    # orbx_np_keyframe
    _fields_ = [("cam", _NpCamera * 2), ("n_cameras", C.c_int32), ("n_left", C.c_int32), ("n", C.c_int32), ("nlevels", C.c_int32),
                ("mb", C.c_float), ("reserved", C.c_int32), ("kps", C.c_void_p), ("kps_raw", C.c_void_p), ("u_right", C.c_void_p),
                ("depth", C.c_void_p), ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p)]


class _NpParams(C.Structure):      # orbx_np_params
    _fields_ = [("mbf", C.c_float), ("inertial", C.c_int32), ("far_points", C.c_int32), ("th_far", C.c_float),
                ("ratio_factor", C.c_float), ("monocular", C.c_int32), ("only_stereo", C.c_int32), ("coarse", C.c_int32),
                ("check_orientation", C.c_int32)]


class _NpBow(C.Structure):         # orbx_np_bow
    _fields_ = [("node_ids", C.c_void_p), ("node_start", C.c_void_p), ("feature_idx", C.c_void_p), ("desc", C.c_void_p),
                ("has_map_point", C.c_void_p), ("n_nodes", C.c_int32), ("reserved", C.c_int32)]


class _NpNeighbour(C.Structure):   # orbx_np_neighbour
    _fields_ = [("kf", _NpKeyFrame), ("bow", _NpBow), ("ep", C.c_float * 2), ("F12", C.c_float * 9), ("median_depth", C.c_float)]


NP_CREATED, NP_LOW_PARALLAX, NP_TRIANGULATE, NP_UNPROJECT, NP_Z1, NP_Z2, NP_REPROJ1, NP_REPROJ2, NP_ZERO_DIST, NP_FAR, NP_SCALE = range(11)
NP_NO_MATCH = 255


def np_camera(params, Tcw, Ow=None, kb8_precision=1e-6):
    """One camera of a key frame for TriangulateMatches / CreateNewMapPoints: params = (fx, fy, cx, cy) for a pinhole or (fx, fy, cx,
    cy, k0..k3) for KannalaBrandt8, Tcw = the 3 x 4 (or 4 x 4) pose, Ow = the camera centre (None: -Rcw^T tcw in float32)."""
    prm = np.asarray(params, np.float32).reshape(-1)
    T = np.asarray(Tcw, np.float32).reshape(-1, 4)[:3]
    if Ow is None:
        Ow = -(T[:, :3].T @ T[:, 3])
    c = _NpCamera()
    c.model = CAMERA_KB8 if len(prm) == 8 else CAMERA_PINHOLE
    c.p[:len(prm)] = prm.tolist()
    c.kb8_precision = kb8_precision
    c.Tcw[:] = T.reshape(12).tolist()
    c.Ow[:] = np.asarray(Ow, np.float32).reshape(3).tolist()
    return c


class NpKeyFrame:
    """What LocalMapping::CreateNewMapPoints reads of a key frame (orbx_np_keyframe).  cameras = one np_camera or (left, right);
    kps = mvKeysUn (single camera) or mvKeys | mvKeysRight with n_left = NLeft (two cameras); uRight / depth = mvuRight / mvDepth
    (None: monocular); kpsRaw = mvKeys where it differs from mvKeysUn (read by UnprojectStereo)."""

    def __init__(self, cameras, kps, scaleFactors, levelSigma2, uRight=None, depth=None, mb=0.0, n_left=-1, kpsRaw=None):
        cams = list(cameras) if isinstance(cameras, (list, tuple)) else [cameras]
        self.kps = np.ascontiguousarray(kps, KP_DTYPE)
        self.raw = None if kpsRaw is None else np.ascontiguousarray(kpsRaw, KP_DTYPE)
        self.ur = None if uRight is None else np.ascontiguousarray(uRight, np.float32)
        self.depth = None if depth is None else np.ascontiguousarray(depth, np.float32)
        self.sf, self.sg = np.ascontiguousarray(scaleFactors, np.float32), np.ascontiguousarray(levelSigma2, np.float32)
        s = self.c = _NpKeyFrame()
        for j, c in enumerate(cams):
            s.cam[j] = c
        s.n_cameras, s.n_left, s.n, s.nlevels, s.mb = len(cams), int(n_left), len(self.kps), len(self.sf), float(mb)
        s.kps, s.scale_factors, s.level_sigma2 = _p(self.kps), _p(self.sf), _p(self.sg)
        s.kps_raw = None if self.raw is None else _p(self.raw)
        s.u_right = None if self.ur is None else _p(self.ur)
        s.depth = None if self.depth is None else _p(self.depth)


def _np_params(mbf, inertial, far_points, th_far, ratio_factor, monocular=False, only_stereo=False, coarse=False, check_ori=False):
    return _NpParams(float(mbf), int(inertial), int(far_points), float(th_far), float(ratio_factor), int(monocular),
                     int(only_stereo), int(coarse), int(check_ori))


def TriangulateMatches(kf1, kf2, matches12, ratio_factor, mbf=0.0, inertial=False, far_points=False, th_far=0.0, device=0):
    """The per-match geometry of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:504-707) for one pair of NpKeyFrame and a
    match list matches12[n1] (idx2 or -1) on the GPU (orbx_triangulate_matches).  ratio_factor = 1.5f * mfScaleFactor, mbf = the
    current key frame's.  Returns (n_created, status [n1] NP_*, x3d [n1][3], point_stereo [n1] bool)."""
    m = np.ascontiguousarray(matches12, np.int32).reshape(-1)
    n1 = kf1.c.n
    if len(m) != n1:
        raise ValueError("one match entry per feature of key frame 1")
    prm = _np_params(mbf, inertial, far_points, th_far, ratio_factor)
    status, x3d, ps = np.full(n1, NP_NO_MATCH, np.uint8), np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8)
    n = _check(lib().orbx_triangulate_matches(int(device), C.addressof(kf1.c), C.addressof(kf2.c), _p(m), C.addressof(prm),
                                              _p(status), _p(x3d), _p(ps)))
    return n, status, x3d, ps.astype(bool)


def _np_bow(fv, desc, has_map_point, keep):
    ids, start, feats = (np.ascontiguousarray(fv[0], np.uint32), np.ascontiguousarray(fv[1], np.int32),
                         np.ascontiguousarray(fv[2], np.uint32))
    d, h = np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(has_map_point, np.uint8)
    keep.extend([ids, start, feats, d, h])
    return _NpBow(_p(ids), _p(start), _p(feats), _p(d), _p(h), len(ids), 0)


def CreateNewMapPoints(kf1, fv1, desc1, hasMapPoint1, neighbours, ratio_factor, mbf=0.0, monocular=False, inertial=False,
                       far_points=False, th_far=0.0, bCoarse=False, bOnlyStereo=False, check_ori=False, device=0):
    """The neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:458-727) in one call (orbx_create_new_map_points),
    single-camera key frames.  kf1 = NpKeyFrame of the current key frame, fv1 / desc1 / hasMapPoint1 as SearchForTriangulation takes
    them; neighbours = up to 30 dicts with kf (NpKeyFrame), fv, desc, hasMapPoint, ep, F12 and median_depth (monocular only).
    Returns a dict: n_matches [K] (-1 = skipped by the baseline test), n_created [K], matches12 [K][n1], status [K][n1], x3d
    [K][n1][3], point_stereo [K][n1], has_map_point1 [n1] (the final flags), total."""
    K, n1 = len(neighbours), kf1.c.n
    keep = []
    b1 = _np_bow(fv1, desc1, hasMapPoint1, keep)
    nbs = (_NpNeighbour * max(K, 1))()
    for k, nb in enumerate(neighbours):
        nbs[k].kf = nb["kf"].c
        nbs[k].bow = _np_bow(nb["fv"], nb["desc"], nb["hasMapPoint"], keep)
        nbs[k].ep[:] = np.asarray(nb["ep"], np.float32).reshape(2).tolist()
        if nb.get("F12") is not None:
            nbs[k].F12[:] = np.asarray(nb["F12"], np.float32).reshape(9).tolist()
        nbs[k].median_depth = float(nb.get("median_depth", 0.0))
    prm = _np_params(mbf, inertial, far_points, th_far, ratio_factor, monocular, bOnlyStereo, bCoarse, check_ori)
    nm, nc = np.zeros(K, np.int32), np.zeros(K, np.int32)
    m = np.full((K, n1), -1, np.int32)
    status, x3d, ps = np.full((K, n1), NP_NO_MATCH, np.uint8), np.zeros((K, n1, 3), np.float32), np.zeros((K, n1), np.uint8)
    flags = np.zeros(n1, np.uint8)
    total = _check(lib().orbx_create_new_map_points(int(device), C.addressof(kf1.c), C.addressof(b1), C.addressof(nbs), K,
                                                    C.addressof(prm), _p(nm), _p(nc), _p(m), _p(status), _p(x3d), _p(ps), _p(flags)))
    return dict(n_matches=nm, n_created=nc, matches12=m, status=status, x3d=x3d, point_stereo=ps.astype(bool),
                has_map_point1=flags, total=total)


def _pose_frames_kb8(q, t, cam_left, cam_right, trl_q, trl_t, n_frames):
    fr = np.zeros(n_frames, POSE_KB8_DTYPE)
    fr["q"] = np.asarray(q, np.float32).reshape(n_frames, 4)
    fr["t"] = np.asarray(t, np.float32).reshape(n_frames, 3)
    fr["kb8_left"] = np.asarray(cam_left, np.float32).reshape(-1, 8)
    if cam_right is not None:
        fr["kb8_right"] = np.asarray(cam_right, np.float32).reshape(-1, 8)
    fr["trl_q"] = [0, 0, 0, 1] if trl_q is None else np.asarray(trl_q, np.float32).reshape(-1, 4)
    if trl_t is not None:
        fr["trl_t"] = np.asarray(trl_t, np.float32).reshape(-1, 3)
    return fr


def PoseOptimizationKB8(kps, nLeft, worldPos, hasPoint, invLevelSigma2, q, t, camLeft, camRight=None, TrlQ=None, TrlT=None,
                        outlier=None, device=0):
    """Optimizer::PoseOptimization(Frame*) for a KannalaBrandt8 frame on the GPU (orbx_pose_optimization_kb8).  kps = mvKeys then
    mvKeysRight (KP_DTYPE, N = Nleft + Nright; N == nLeft: monocular KB8), camLeft / camRight = the 8 KB8 parameters, (TrlQ, TrlT) =
    GetRelativePoseTrl() as Sophus stores it (x y z w, t), other arguments as PoseOptimization.  Returns (nGood, q, t, outlier)."""
    k = np.ascontiguousarray(kps, KP_DTYPE)
    n = len(k)
    nLeft = int(nLeft)
    wp = np.ascontiguousarray(worldPos, np.float32).reshape(n, 3)
    hp = np.ascontiguousarray(hasPoint, np.uint8).reshape(n)
    sig = np.ascontiguousarray(invLevelSigma2, np.float32)
    fr = _pose_frames_kb8(q, t, camLeft, camRight, TrlQ, TrlT, 1)
    out = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, np.uint8).reshape(n)
    ng = _check(lib().orbx_pose_optimization_kb8(int(device), _p(k), nLeft, n - nLeft, _p(wp), _p(hp), _p(sig), len(sig), _p(fr),
                                                 _p(out)))
    return ng, fr["q"][0].copy(), fr["t"][0].copy(), out.astype(bool)


def PoseOptimizationFisheyeBatch(ex, first_left, first_right, n_frames, worldPos, hasPoint, q, t, camLeft, camRight=None, TrlQ=None,
                                 TrlT=None, outlier=None, want_trials=False):
    """PoseOptimizationKB8 of the frames of ex's last extraction batch in ONE kernel launch (orbx_pose_optimization_fisheye_batch):
    frame f = left image first_left + f, right image first_right + f (-1: monocular KB8).  worldPos [n_frames][2 cap][3],
    hasPoint / outlier [n_frames][2 cap] in the row layout of SearchByProjectionFisheyeBatch's match (left keypoints, then the
    right ones), q [n_frames][4], t [n_frames][3], cameras / Trl one row for all frames or one per frame.
    Returns (nGood, q, t, outlier[, trials])."""
    n2 = 2 * ex.capacity
    wp = np.ascontiguousarray(worldPos, np.float32).reshape(n_frames, n2, 3)
    hp = np.ascontiguousarray(hasPoint, np.uint8).reshape(n_frames, n2)
    fr = _pose_frames_kb8(q, t, camLeft, camRight, TrlQ, TrlT, n_frames)
    out = np.zeros((n_frames, n2), np.uint8) if outlier is None else np.array(outlier, np.uint8).reshape(n_frames, n2)
    ng = np.zeros(n_frames, np.int32)
    tr = np.zeros(n_frames, np.int32)
    _check(lib().orbx_pose_optimization_fisheye_batch(ex._h, int(first_left), int(first_right), int(n_frames), _p(wp), _p(hp),
                                                      _p(fr), _p(out), _p(ng), _p(tr)))
    res = (ng, fr["q"].copy(), fr["t"].copy(), out.astype(bool))
    return res + (tr,) if want_trials else res


def debug_sincos(angles, fused=True, device=0):
    """Test hook: the device's sinf / cosf (csrc/orbx_sincos.h: glibc's FMA or SSE2 variant; fused=2: k_describe's branch-free
    restatement of the FMA variant, glibc_sincosf_sel) of angles in radians."""
    a = np.ascontiguousarray(angles, np.float32)
    sn, cs = np.zeros_like(a), np.zeros_like(a)
    _check(lib().orbx_debug_sincos(device, _p(a), a.size, 2 if fused == 2 else (1 if fused else 0), _p(sn), _p(cs)))
    return sn, cs


def debug_fast_atan2(y, x, device=0):
    """Test hook: k_describe's branch-free cv::fastAtan2 (fast_atan2_sel) of the pairs (y[i], x[i]), in degrees."""
    y, x = np.ascontiguousarray(y, np.float32).ravel(), np.ascontiguousarray(x, np.float32).ravel()
    if y.size != x.size:
        raise ValueError("y and x must have the same length")
    out = np.zeros_like(y)
    _check(lib().orbx_debug_fast_atan2(device, _p(y), _p(x), y.size, _p(out)))
    return out


def bf_knn2(descQ, descT, device=0):
    """cv::BFMatcher(NORM_HAMMING).knnMatch(Q, T, 2) + Lowe ratio 0.7 of ComputeStereoFishEyeMatches
    (src/Frame.cc:1293-1302). Returns (idx[nQ,2], dist[nQ,2], ratio_ok[nQ])."""
    q = np.ascontiguousarray(descQ, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(descT, np.uint8).reshape(-1, 32)
    idx = np.zeros((len(q), 2), np.int32)
    dist = np.zeros((len(q), 2), np.int32)
    ok = np.zeros(len(q), np.uint8)
    _check(lib().orbx_bf_knn2(device, _p(q), len(q), _p(t), len(t), _p(idx), _p(dist), _p(ok)))
    return idx, dist, ok


def kb8_rig(cam1, cam2, R12, t12, precision=1e-6):
    """orbx_kb8_rig as 29 float32: the two KannalaBrandt8 parameter vectors (fx fy cx cy k0 k1 k2 k3), the Newton stop
    of unproject, and mRlr (row-major) / mtlr (include/Frame.h:208-209)."""
    rig = np.concatenate([np.asarray(cam1, np.float32).ravel(), np.asarray(cam2, np.float32).ravel(),
                          np.array([precision], np.float32), np.asarray(R12, np.float32).ravel(),
                          np.asarray(t12, np.float32).ravel()]).astype(np.float32)
    if rig.size != 29:
        raise ValueError("kb8_rig: need 8 + 8 camera parameters, a 3x3 rotation and a 3-vector")
    return rig


def ComputeStereoFishEyeMatches(kpsL, descL, monoL, kpsR, descR, monoR, rig, level_sigma2, device=0):
    """Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1273-1331) incl. KannalaBrandt8::TriangulateMatches.
    Returns (nMatches, descMatches, mvLeftToRightMatch, mvRightToLeftMatch, mvDepth, mvStereo3Dpoints[nL, 3])."""
    kl, kr = np.ascontiguousarray(kpsL, KP_DTYPE), np.ascontiguousarray(kpsR, KP_DTYPE)
    dl = np.ascontiguousarray(descL, np.uint8).reshape(-1, 32)
    dr = np.ascontiguousarray(descR, np.uint8).reshape(-1, 32)
    if len(dl) != len(kl) or len(dr) != len(kr):
        raise ValueError("one descriptor row per keypoint")
    rig = np.ascontiguousarray(rig, np.float32)
    if rig.size != 29:
        raise ValueError("rig: use kb8_rig()")
    s2 = np.ascontiguousarray(level_sigma2, np.float32)
    l2r, r2l = np.zeros(len(kl), np.int32), np.zeros(len(kr), np.int32)
    depth, pts = np.zeros(len(kl), np.float32), np.zeros((len(kl), 3), np.float32)
    nd = C.c_int(0)
    n = _check(lib().orbx_fisheye_stereo_match(device, _p(kl), _p(dl), len(kl), int(monoL), _p(kr), _p(dr), len(kr),
                                               int(monoR), _p(rig), _p(s2), len(s2), _p(l2r), _p(r2l), _p(depth),
                                               _p(pts), C.byref(nd)))
    return n, nd.value, l2r, r2l, depth, pts


def fisheye_match_async(left, right, rig, first_left=0, first_right=0, n_pairs=1):
    """Enqueue Frame::ComputeStereoFishEyeMatches for n_pairs image pairs of the extractors' last (batch) extraction;
    everything stays on the device (config C4 in batched mode)."""
    rig = np.ascontiguousarray(rig, np.float32)
    if rig.size != 29:
        raise ValueError("rig: use kb8_rig()")
    _check(lib().orbx_fisheye_stereo_match_batch(left._h, first_left, right._h, first_right, n_pairs, _p(rig)))


def fisheye_download(left, right, pair=0):
    """Host copy of one pair of the last fisheye_match_async: (nMatches, descMatches, l2r, r2l, depth, p3d), arrays
    sized by the handles' capacities (entries beyond the keypoint counts are -1 / 0)."""
    l2r, r2l = np.zeros(left.capacity, np.int32), np.zeros(right.capacity, np.int32)
    depth, pts = np.zeros(left.capacity, np.float32), np.zeros((left.capacity, 3), np.float32)
    nd = C.c_int(0)
    n = _check(lib().orbx_fisheye_download(left._h, pair, _p(l2r), _p(r2l), _p(depth), _p(pts), left.capacity,
                                           right.capacity, C.byref(nd)))
    return n, nd.value, l2r, r2l, depth, pts


def cvtColorGray(img, rgb=True, device=0):
    """cv::cvtColor(img, COLOR_RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY) as Tracking::GrabImage* calls it
    (src/Tracking.cc:1394-1412): img is H x W x 3|4 uint8, rgb = the reference's mbRGB."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, cn = img.shape
    dst = np.zeros((h, w), np.uint8)
    _check(lib().orbx_cvt_gray(device, _p(img), w, h, img.strides[0], cn, int(bool(rgb)), _p(dst), dst.strides[0]))
    return dst


def resize(img, dst_w, dst_h, device=0):
    """cv::resize(img, out, Size(dst_w, dst_h)) with INTER_LINEAR (src/System.cc:297-298) for H x W [x 3|4] uint8 images."""
    img = np.ascontiguousarray(img, np.uint8)
    cn = 1 if img.ndim == 2 else img.shape[2]
    h, w = img.shape[:2]
    dst = np.zeros((dst_h, dst_w) if img.ndim == 2 else (dst_h, dst_w, cn), np.uint8)
    _check(lib().orbx_resize_linear(device, _p(img), w, h, img.strides[0], cn, _p(dst), dst_w, dst_h, dst.strides[0]))
    return dst


def remap(img, map_x, map_y, device=0):
    """cv::remap(img, out, map_x, map_y, cv::INTER_LINEAR) with CV_32FC1 maps (src/System.cc:294-295) for H x W [x 3|4] uint8."""
    img = np.ascontiguousarray(img, np.uint8)
    mx = np.ascontiguousarray(map_x, np.float32)
    my = np.ascontiguousarray(map_y, np.float32)
    if mx.shape != my.shape or mx.ndim != 2:
        raise ValueError("map_x and map_y must be two float images of the same size")
    cn = 1 if img.ndim == 2 else img.shape[2]
    h, w = img.shape[:2]
    dh, dw = mx.shape
    dst = np.zeros((dh, dw) if img.ndim == 2 else (dh, dw, cn), np.uint8)
    _check(lib().orbx_remap_linear(device, _p(img), w, h, img.strides[0], cn, _p(mx), _p(my), dw, _p(dst), dw, dh, dst.strides[0]))
    return dst


class CLAHE:
    """cv::createCLAHE(clipLimit, tileGridSize) as the TUM-VI examples use it (Examples/Stereo/stereo_tum_vi.cc:100,142-143)."""

    def __init__(self, clipLimit=3.0, tileGridSize=(8, 8), device=0):
        self.clip, self.tiles, self.device = float(clipLimit), (int(tileGridSize[0]), int(tileGridSize[1])), device

    def apply(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        if img.ndim != 2:
            raise ValueError("CLAHE needs a single-channel image")
        h, w = img.shape
        dst = np.zeros((h, w), np.uint8)
        _check(lib().orbx_clahe(self.device, _p(img), w, h, img.strides[0], self.clip, self.tiles[0], self.tiles[1], _p(dst),
                                dst.strides[0]))
        return dst


class Preproc:
    """Device-resident pre-processing chain [CLAHE] -> [remap | resize] -> [gray] in front of the extractor
    (include/orbx.h orbx_preproc_*).  maps = (map_x, map_y) float arrays of shape (n_maps, out_h, out_w) or (out_h, out_w)."""

    def __init__(self, src_w, src_h, channels=1, rgb=True, maps=None, out_size=None, clahe=None, max_batch=2, device=0):
        prm = _PreprocParams()
        prm.src_w, prm.src_h, prm.channels, prm.rgb_order = src_w, src_h, channels, int(bool(rgb))
        keep = []
        if maps is not None:
            mx = np.ascontiguousarray(maps[0], np.float32)
            my = np.ascontiguousarray(maps[1], np.float32)
            if mx.ndim == 2:
                mx, my = mx[None], my[None]
            prm.n_maps, prm.out_h, prm.out_w = mx.shape
            prm.map_x, prm.map_y, prm.map_stride = mx.ctypes.data, my.ctypes.data, mx.shape[2]
            keep = [mx, my]
        elif out_size is not None:
            prm.out_w, prm.out_h = out_size
        if clahe is not None:
            prm.clahe_clip_limit, (prm.clahe_tiles_x, prm.clahe_tiles_y) = float(clahe[0]), clahe[1]
        h = C.c_void_p()
        _check(lib().orbx_preproc_create(C.byref(prm), max_batch, device, C.byref(h)))
        del keep
        self._h = h
        ow, oh = C.c_int(), C.c_int()
        _check(lib().orbx_preproc_output_size(self._h, C.byref(ow), C.byref(oh)))
        self.out_w, self.out_h, self.channels, self.src_w, self.src_h = ow.value, oh.value, channels, src_w, src_h

    def __del__(self):
        if getattr(self, "_h", None):
            lib().orbx_preproc_destroy(self._h)
            self._h = None

    def run(self, frame, map_index=0):
        frame = np.ascontiguousarray(frame, np.uint8)
        dst = np.zeros((self.out_h, self.out_w), np.uint8)
        _check(lib().orbx_preproc_run(self._h, _p(frame), frame.strides[0], map_index, _p(dst), dst.strides[0]))
        return dst

    def run_device(self, d_frames_ptr, n_frames, row_pitch, image_pitch):
        """-> (device pointer, w, h, row_pitch, image_pitch) of the pre-processed gray frames (owned by the handle)."""
        out, w, h = C.c_void_p(), C.c_int(), C.c_int()
        rp, ip = C.c_ssize_t(), C.c_ssize_t()
        _check(lib().orbx_preproc_run_device(self._h, C.c_void_p(d_frames_ptr), n_frames, row_pitch, image_pitch, C.byref(out),
                                             C.byref(w), C.byref(h), C.byref(rp), C.byref(ip)))
        return out.value, w.value, h.value, rp.value, ip.value

    def plan(self):
        """What the handle decided at creation and what its last enqueue launched (orbx_debug_preproc_plan); remap / resize /
        clahe_vec4 / gray_segs are None for a stage that is not part of the plan or has not run."""
        info = np.zeros(8, np.int32)
        _check(lib().orbx_debug_preproc_plan(self._h, _p(info)))
        opt = [None if v < 0 else int(v) for v in info[2:6]]
        return {"lds_table": bool(info[0]), "resize_prepared": bool(info[1]), "remap": opt[0],
                "resize": None if opt[1] is None else ("plain" if opt[1] else "generic"),
                "clahe_vec4": None if opt[2] is None else bool(opt[2]), "gray_segs": opt[3], "frames": int(info[6])}


REMAP_LDS, REMAP_WINDOWS, REMAP_GENERIC = 2, 1, 0   # Preproc.plan()["remap"]: k_remap_lds / k_remap1 / k_remap


def remap_footprints(map_x, map_y, src_w, src_h):
    """The k_remap_lds footprint table a plan would build for these maps (orbx_debug_remap_footprints; host only, no device):
    an int32 array (n_maps, tiles_x, tiles_y, 8), or None when the plan keeps k_remap1."""
    mx = np.ascontiguousarray(map_x, np.float32)
    my = np.ascontiguousarray(map_y, np.float32)
    if mx.ndim == 2:
        mx, my = mx[None], my[None]
    if mx.shape != my.shape or mx.ndim != 3:
        raise ValueError("map_x and map_y must be float images of the same size")
    nm, dh, dw = mx.shape
    tx, ty = (dw + 127) // 128, (dh + 7) // 8
    tab = np.zeros((nm, tx, ty, 8), np.int32)
    gx, gy = C.c_int(), C.c_int()
    rc = lib().orbx_debug_remap_footprints(_p(mx), _p(my), dw, dw, dh, src_w, src_h, nm, _p(tab), tab.size, C.byref(gx), C.byref(gy))
    _check(rc)
    if (gx.value, gy.value) != (tx, ty):
        raise OrbxError("unexpected tile grid %d x %d" % (gx.value, gy.value))
    return tab if rc == 1 else None


def front_tables(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height):
    """The tables that stand in for the fronts of k_detect and k_resize at this frame size (orbx_debug_front_tables; host only,
    no device): (cells, tiles, tile_pitch, tile_rows) -- cells a uint32 array (FAST cells, 16), tiles the flat uint32 table of
    the resize levels (include/orbx.h describes both)."""
    prm = _Params(int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST), int(minThFAST))
    info = np.zeros(4, np.int32)
    _check(lib().orbx_debug_front_tables(C.byref(prm), width, height, None, 0, None, 0, _p(info)))
    cells = np.zeros((int(info[0]), 16), np.uint32)
    tiles = np.zeros(int(info[1]), np.uint32)
    _check(lib().orbx_debug_front_tables(C.byref(prm), width, height, _p(cells), cells.size, _p(tiles) if tiles.size else None,
                                         tiles.size, _p(info)))
    return cells, tiles, int(info[2]), int(info[3])


def resize_stream_tables(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, quads=64):
    """k_resize_stream's lane tables at this frame size (orbx_debug_resize_stream_tables; host only, no device): a list with
    one uint32 array [strips, 3, quads, 4] per level (None for level 0 and for a level that cannot stream)."""
    prm = _Params(int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST), int(minThFAST))
    off = np.zeros(12, np.int32)   # ORBX_MAX_LEVELS
    n = _check(lib().orbx_debug_resize_stream_tables(C.byref(prm), width, height, quads, None, 0, _p(off)))
    tab = np.zeros(n, np.uint32)
    _check(lib().orbx_debug_resize_stream_tables(C.byref(prm), width, height, quads, _p(tab) if n else None, n, _p(off)))
    ends = sorted([int(o) for o in off if o >= 0] + [n])
    return [tab[o:ends[ends.index(int(o)) + 1]].reshape(-1, 3, quads, 4) if l < nlevels and o >= 0 else None
            for l, o in enumerate(off[:nlevels])]


def octree_plan(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height):
    """k_octree's plan at this frame size (orbx_debug_octree_plan; host only, no device): (working threads of the level's workgroup,
    dynamic LDS bytes of the batch's launch), one entry per level."""
    prm = _Params(int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST), int(minThFAST))
    nt, lds = np.zeros(int(nlevels), np.int32), np.zeros(int(nlevels), np.int32)
    _check(lib().orbx_debug_octree_plan(C.byref(prm), width, height, _p(nt), _p(lds)))
    return nt, lds


def _octree_candidates(candidates, nlevels):
    """candidates[image][level] -> (counts[image * nlevels + level], the triples back to back) as orbx_debug_octree takes them."""
    counts, parts = [], [np.zeros((0, 3), np.int32)]
    for per_level in candidates:
        if len(per_level) != nlevels:
            raise ValueError("one candidate array per level")
        for c in per_level:
            c = np.asarray(c, np.int32).reshape(-1, 3)
            counts.append(len(c))
            parts.append(c)
    return np.array(counts, np.int32), np.ascontiguousarray(np.concatenate(parts))


def octree_check(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, candidates):
    """The argument check of ORBextractor.debug_octree (orbx_debug_octree_check; host only, no device): raises OrbxError(E_BADARG)
    for a candidate outside the detectable window, a response outside 1 .. 255, a pixel given twice, a FAST cell or a level with
    more candidates than it holds."""
    prm = _Params(int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST), int(minThFAST))
    counts, flat = _octree_candidates(candidates, int(nlevels))
    _check(lib().orbx_debug_octree_check(C.byref(prm), int(width), int(height), len(candidates), _p(counts), _p(flat)))


def introsort_device(v, nt, device=0):
    """orbx_debug_introsort_device_nt: the device's std::sort replica on a copy of the uint64 array v; nt = 64 (one wave) or the
    workgroup form with 128 / 256 / 512 threads."""
    a = np.array(v, np.uint64)
    _check(lib().orbx_debug_introsort_device_nt(int(device), _p(a), len(a), int(nt)))
    return a


def describe_plan(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, n_images):
    """k_describe's launch plan for a batch of n_images frames of this size (orbx_debug_describe_plan; host only, no device):
    (nk, tasks, magic, taskOff[nlevels]) -- keypoints per wave, workgroups per image, the multiplier of the XCD remap's division
    (0 = no remap) and the first task of every level."""
    prm = _Params(int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST), int(minThFAST))
    out = np.zeros(3 + 12, np.int32)   # ORBX_MAX_LEVELS
    _check(lib().orbx_debug_describe_plan(C.byref(prm), int(width), int(height), int(n_images), _p(out)))
    return int(out[0]), int(out[1]), int(out[2:3].view(np.uint32)[0]), out[3:3 + int(nlevels)].copy()


class ORBVocabulary:
    """ORBVocabulary (DBoW2::TemplatedVocabulary<FORB>) on the device: loadFromTextFile (src/System.cc:131) or the file's
    columns (parent, is_leaf, descriptor, weight per node); transform() = Frame::ComputeBoW (src/Frame.cc:846-851)."""

    def __init__(self, k=None, L=None, parent=None, is_leaf=None, desc=None, weight=None, scoring=0, weighting=0, path=None,
                 device=0):
        h = C.c_void_p()
        if path is not None:
            _check(lib().orbx_vocabulary_load_text(device, path.encode(), C.byref(h)))
        else:
            parent = np.ascontiguousarray(parent, np.int32)
            leaf = np.ascontiguousarray(is_leaf, np.uint8)
            d = np.ascontiguousarray(desc, np.uint8)
            w = np.ascontiguousarray(weight, np.float64)
            _check(lib().orbx_vocabulary_create(device, k, L, scoring, weighting, len(parent), _p(parent), _p(leaf), _p(d), _p(w),
                                                C.byref(h)))
        self._h = h
        info = np.zeros(6, np.int32)
        _check(lib().orbx_vocabulary_info(self._h, _p(info)))
        self.k, self.L, self.n_nodes, self.n_words, self.scoring, self.weighting = (int(x) for x in info)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().orbx_vocabulary_destroy(self._h)
            self._h = None

    def transform(self, desc, levelsup=4):
        """-> (word_ids, values), (node_ids, node_start, feature_idx): mBowVec and mFeatVec (CSR)."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        words, values = np.zeros(n, np.uint32), np.zeros(n, np.float64)
        nodes, start, feats = np.zeros(n, np.uint32), np.zeros(n + 1, np.int32), np.zeros(n, np.uint32)
        nw, nn = C.c_int(), C.c_int()
        nf = _check(lib().orbx_bow_transform(self._h, _p(d), n, levelsup, _p(words), _p(values), C.byref(nw), _p(nodes), _p(start),
                                             _p(feats), C.byref(nn)))
        return (words[:nw.value].copy(), values[:nw.value].copy()), (nodes[:nn.value].copy(), start[:nn.value + 1].copy(), feats[:nf].copy())

    def transform_batch(self, extractor, levelsup=4):
        """ComputeBoW for every image of the extractor's last extraction, on its stream (results stay on the device)."""
        _check(lib().orbx_bow_transform_batch(extractor._h, self._h, levelsup))

    @staticmethod
    def download(extractor, image):
        cap = extractor.capacity
        words, values = np.zeros(cap, np.uint32), np.zeros(cap, np.float64)
        nodes, start, feats = np.zeros(cap, np.uint32), np.zeros(cap + 1, np.int32), np.zeros(cap, np.uint32)
        nw, nn = C.c_int(), C.c_int()
        nf = _check(lib().orbx_bow_download(extractor._h, image, _p(words), _p(values), C.byref(nw), _p(nodes), _p(start), _p(feats),
                                            C.byref(nn), cap))
        return (words[:nw.value].copy(), values[:nw.value].copy()), (nodes[:nn.value].copy(), start[:nn.value + 1].copy(), feats[:nf].copy())


class _KfdbDetails(C.Structure):   # orbx_kfdb_details
    _fields_ = [("cap", C.c_int32), ("n_scored", C.c_void_p), ("max_common_words", C.c_void_p), ("kf_id", C.c_void_p),
                ("common_words", C.c_void_p), ("score", C.c_void_p), ("acc_score", C.c_void_p), ("best_kf_id", C.c_void_p)]


KFDB_DETAIL_DTYPE = np.dtype([("kf_id", "<i4"), ("common_words", "<i4"), ("score", "<f4"), ("acc_score", "<f4"), ("best_kf_id", "<i4")])


class KeyFrameDatabase:
    """ORB_SLAM3::KeyFrameDatabase (src/KeyFrameDatabase.cc) on the device.  Key frames and maps are ints (mnId); a BoW vector is
    the (word_ids, values) pair ORBVocabulary.transform returns.  The covisible lists (GetBestCovisibilityKeyFrames(10)), the
    query's connected key frames and the bad maps stay with the caller and are handed over (set_covisibles, arguments)."""

    def __init__(self, voc, max_keyframes, max_words):
        self._h = None
        h = C.c_void_p()
        _check(lib().orbx_kfdb_create(voc._h if voc is not None else None, max_keyframes, max_words, C.byref(h)))
        self._h = h
        self.max_keyframes, self.max_words = max_keyframes, max_words

    def close(self):
        if getattr(self, "_h", None):
            lib().orbx_kfdb_destroy(self._h)
            self._h = None

    __del__ = close

    def __len__(self):
        return _check(lib().orbx_kfdb_size(self._h))

    @staticmethod
    def _bow(bow):
        w, v = np.ascontiguousarray(bow[0], np.uint32), np.ascontiguousarray(bow[1], np.float64)
        if w.ndim != 1 or w.shape != v.shape:
            raise ValueError("a BoW vector is (word_ids[n], values[n])")
        return w, v

    def profile(self, on=-1):
        """Switches the device-event bracket of the detect calls (on = True / False) and returns the last call's milliseconds."""
        ms = C.c_float()
        _check(lib().orbx_kfdb_profile(self._h, int(on), C.byref(ms)))
        return ms.value

    def add(self, kf_id, map_id, bow):
        w, v = self._bow(bow)
        _check(lib().orbx_kfdb_add(self._h, kf_id, map_id, _p(w), _p(v), len(w)))

    def add_from_batch(self, extractor, image, kf_id, map_id):
        """add() with the BoW vector of `image` of the extractor's last ORBVocabulary.transform_batch (device to device)."""
        _check(lib().orbx_kfdb_add_from_batch(self._h, extractor._h, image, kf_id, map_id))

    def erase(self, kf_id):
        _check(lib().orbx_kfdb_erase(self._h, kf_id))

    def clear(self):
        _check(lib().orbx_kfdb_clear(self._h))

    def clearMap(self, map_id):
        return _check(lib().orbx_kfdb_clear_map(self._h, map_id))

    def set_covisibles(self, kf_ids, best10):
        """best10[i] = up to ten key-frame ids, GetBestCovisibilityKeyFrames(10) of kf_ids[i]."""
        ids = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        b = np.full((len(ids), 10), -1, np.int32)
        for r, row in enumerate(best10):
            row = np.asarray(row, np.int32).reshape(-1)[:10]
            b[r, :len(row)] = row
        _check(lib().orbx_kfdb_set_covisibles(self._h, len(ids), _p(ids), _p(b)))

    def _details(self, nq, want):
        if not want:
            return None, None
        cap = max(len(self), 1)
        a = {"n": np.zeros(nq, np.int32), "max": np.zeros(nq, np.int32), "kf": np.zeros((nq, cap), np.int32),
             "words": np.zeros((nq, cap), np.int32), "score": np.zeros((nq, cap), np.float32), "acc": np.zeros((nq, cap), np.float32),
             "best": np.zeros((nq, cap), np.int32)}
        d = _KfdbDetails(cap, *(a[k].ctypes.data for k in ("n", "max", "kf", "words", "score", "acc", "best")))
        return a, d

    @staticmethod
    def _detail_records(a, q):
        rec = np.zeros(int(a["n"][q]), KFDB_DETAIL_DTYPE)
        for name, key in (("kf_id", "kf"), ("common_words", "words"), ("score", "score"), ("acc_score", "acc"), ("best_kf_id", "best")):
            rec[name] = a[key][q, :len(rec)]
        return {"max_common_words": int(a["max"][q]), "scored": rec}

    def DetectRelocalizationCandidates(self, bow, map_id, details=False):
        """-> vpRelocCandidates as a list of ids [, {"max_common_words", "scored": records in the order of lScoreAndMatch}]."""
        w, v = self._bow(bow)
        cap = max(len(self), 1)
        cand, n = np.zeros(cap, np.int32), C.c_int()
        a, d = self._details(1, details)
        _check(lib().orbx_kfdb_detect_relocalization_candidates(self._h, _p(w), _p(v), len(w), map_id, _p(cand), cap, C.byref(n),
                                                                C.byref(d) if d else None))
        out = [int(x) for x in cand[:n.value]]
        return (out, self._detail_records(a, 0)) if details else out

    def DetectRelocalizationCandidatesBatch(self, extractor, first_image, map_ids, details=False):
        """One DetectRelocalizationCandidates per frame of the extractor's last transform_batch, frames first_image .. +len(map_ids),
        in frame order, with the queries read on the device."""
        maps = np.ascontiguousarray(map_ids, np.int32).reshape(-1)
        nq, cap = len(maps), max(len(self), 1)
        cand, n = np.zeros((nq, cap), np.int32), np.zeros(nq, np.int32)
        a, d = self._details(nq, details)
        _check(lib().orbx_kfdb_detect_relocalization_candidates_batch(self._h, extractor._h, first_image, nq, _p(maps), _p(cand), cap,
                                                                      _p(n), C.byref(d) if d else None))
        out = [[int(x) for x in cand[q, :n[q]]] for q in range(nq)]
        return (out, [self._detail_records(a, q) for q in range(nq)]) if details else out

    def DetectNBestCandidates(self, bow, map_id, connected_ids, nNumCandidates, bad_map_ids=(), details=False):
        """-> (vpLoopCand, vpMergeCand) [, details]."""
        w, v = self._bow(bow)
        conn = np.ascontiguousarray(list(connected_ids), np.int32).reshape(-1)
        bad = np.ascontiguousarray(list(bad_map_ids), np.int32).reshape(-1)
        k = max(int(nNumCandidates), 1)
        loop, merge, nl, nm = np.zeros(k, np.int32), np.zeros(k, np.int32), C.c_int(), C.c_int()
        a, d = self._details(1, details)
        _check(lib().orbx_kfdb_detect_n_best_candidates(self._h, _p(w), _p(v), len(w), map_id, _p(conn), len(conn), _p(bad), len(bad),
                                                        int(nNumCandidates), _p(loop), C.byref(nl), _p(merge), C.byref(nm),
                                                        C.byref(d) if d else None))
        out = ([int(x) for x in loop[:nl.value]], [int(x) for x in merge[:nm.value]])
        return (out[0], out[1], self._detail_records(a, 0)) if details else out


def SearchByBoW(kf_fv, kf_kps, kf_desc, kf_valid, f_fv, f_kps, f_desc, n_left_f=-1, nnratio=0.7, check_ori=True, device=0):
    """ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (src/ORBmatcher.cc:230-404): feature vectors as the CSR triples
    ORBVocabulary.transform returns; -> (nmatches, match[n_f] = keyframe feature index or -1)."""
    kn, ks, kfi = (np.ascontiguousarray(kf_fv[0], np.uint32), np.ascontiguousarray(kf_fv[1], np.int32), np.ascontiguousarray(kf_fv[2], np.uint32))
    fn, fs, ffi = (np.ascontiguousarray(f_fv[0], np.uint32), np.ascontiguousarray(f_fv[1], np.int32), np.ascontiguousarray(f_fv[2], np.uint32))
    kk, fk = np.ascontiguousarray(kf_kps, KP_DTYPE), np.ascontiguousarray(f_kps, KP_DTYPE)
    kd, fd = np.ascontiguousarray(kf_desc, np.uint8), np.ascontiguousarray(f_desc, np.uint8)
    kv = np.ascontiguousarray(kf_valid, np.uint8)
    match = np.zeros(len(fk), np.int32)
    n = _check(lib().orbx_search_by_bow(device, _p(kn), _p(ks), _p(kfi), len(kn), _p(kk), _p(kd), _p(kv), len(kk), _p(fn), _p(fs),
                                        _p(ffi), len(fn), _p(fk), _p(fd), len(fk), int(n_left_f), float(nnratio), int(bool(check_ori)),
                                        _p(match)))
    return n, match


def SearchByBoWBatch(ex, first_image, kf_fvs, kf_kps, kf_descs, kf_valids, n_left_f=-1, nnratio=0.7, check_ori=True):
    """SearchByBoW(KeyFrame, Frame) for the frames of ex's last extraction batch in one call (orbx_search_by_bow_batch): the frames'
    keypoints, descriptors and feature vectors (ORBVocabulary.transform_batch) stay on the device; the key frame of pair f comes
    as kf_fvs[f] = (node_ids, node_start, feature_idx), kf_kps[f], kf_descs[f], kf_valids[f].
    Returns (n_matches [F], list of match arrays [n_f])."""
    F = len(kf_fvs)
    nn = np.array([len(fv[0]) for fv in kf_fvs], np.int32)
    nk = np.array([len(k) for k in kf_kps], np.int32)
    ns, ks = max(int(nn.max()) if F else 0, 1), max(int(nk.max()) if F else 0, 1)
    ids, st = np.zeros((F, ns), np.uint32), np.zeros((F, ns + 1), np.int32)
    fi, K = np.zeros((F, ks), np.uint32), np.zeros((F, ks), KP_DTYPE)
    D, V = np.zeros((F, ks, 32), np.uint8), np.zeros((F, ks), np.uint8)
    for f in range(F):
        ids[f, :nn[f]] = kf_fvs[f][0]
        st[f, :nn[f] + 1] = kf_fvs[f][1]
        fi[f, :len(kf_fvs[f][2])] = kf_fvs[f][2]
        K[f, :nk[f]] = kf_kps[f]
        D[f, :nk[f]] = np.asarray(kf_descs[f], np.uint8).reshape(-1, 32)
        V[f, :nk[f]] = kf_valids[f]
    cap = ex.capacity
    match = np.full((F, cap), -1, np.int32)
    nm = np.zeros(F, np.int32)
    _check(lib().orbx_search_by_bow_batch(ex._h, int(first_image), F, _p(ids), _p(st), _p(nn), ns, _p(fi), _p(K), _p(D), _p(V), _p(nk), ks,
                                          int(n_left_f), float(nnratio), int(bool(check_ori)), _p(match), _p(nm)))
    return nm, match


def SearchByBoWKeyFrames(fv1, kps1, desc1, valid1, fv2, kps2, desc2, valid2, nnratio=0.75, check_ori=True, device=0):
    """ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (src/ORBmatcher.cc:766-884) ->
    (nmatches, matches12[n1] = feature of pKF2 or -1)."""
    n1n, s1, f1 = (np.ascontiguousarray(fv1[0], np.uint32), np.ascontiguousarray(fv1[1], np.int32), np.ascontiguousarray(fv1[2], np.uint32))
    n2n, s2, f2 = (np.ascontiguousarray(fv2[0], np.uint32), np.ascontiguousarray(fv2[1], np.int32), np.ascontiguousarray(fv2[2], np.uint32))
    k1, k2 = np.ascontiguousarray(kps1, KP_DTYPE), np.ascontiguousarray(kps2, KP_DTYPE)
    d1, d2 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(desc2, np.uint8)
    v1, v2 = np.ascontiguousarray(valid1, np.uint8), np.ascontiguousarray(valid2, np.uint8)
    m = np.full(len(k1), -1, np.int32)
    n = _check(lib().orbx_search_by_bow_keyframes(device, _p(n1n), _p(s1), _p(f1), len(n1n), _p(k1), _p(d1), _p(v1), len(k1), _p(n2n),
                                                  _p(s2), _p(f2), len(n2n), _p(k2), _p(d2), _p(v2), len(k2), float(nnratio),
                                                  int(bool(check_ori)), _p(m)))
    return n, m


def UndistortKeyPoints(kps, K, dist, device=0):
    """Frame::UndistortKeyPoints (src/Frame.cc:853-885): mvKeysUn from mvKeys; K = (fx, fy, cx, cy), dist = mDistCoef."""
    k = np.ascontiguousarray(kps, KP_DTYPE)
    K = np.ascontiguousarray(K, np.float32)
    d = np.ascontiguousarray(dist, np.float32).ravel()
    out = np.zeros(len(k), KP_DTYPE)
    _check(lib().orbx_undistort_keypoints(device, _p(k), len(k), _p(K), _p(d) if len(d) else None, len(d), _p(out)))
    return out


def ComputeImageBounds(cols, rows, K, dist, device=0):
    """Frame::ComputeImageBounds (src/Frame.cc:887-919) -> (mnMinX, mnMinY, mnMaxX, mnMaxY)."""
    K = np.ascontiguousarray(K, np.float32)
    d = np.ascontiguousarray(dist, np.float32).ravel()
    b = np.zeros(4, np.float32)
    _check(lib().orbx_compute_image_bounds(device, int(cols), int(rows), _p(K), _p(d) if len(d) else None, len(d), _p(b)))
    return b


def GetFeaturesInArea(kpsUn, bounds, queries, device=0, return_grid=False):
    """Frame::AssignFeaturesToGrid + GetFeaturesInArea (src/Frame.cc:520-547,765-844) for a batch of queries
    (rows of x, y, r, minLevel, maxLevel).  Returns a list of index arrays (reference order), optionally the
    grid as (cell_start[3073], items[n])."""
    k = np.ascontiguousarray(kpsUn, KP_DTYPE)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 5)
    offs = np.zeros(len(q) + 1, np.int32)
    cs = np.zeros(64 * 48 + 1, np.int32)
    items = np.zeros(max(len(k), 1), np.int32)
    cap = max(1, len(k)) * max(1, len(q))
    idx = np.zeros(min(cap, 1 << 26), np.int32)
    tot = _check(lib().orbx_features_in_area(device, _p(k), len(k), bounds[0], bounds[1], bounds[2], bounds[3], _p(q),
                                             len(q), _p(offs), _p(idx), len(idx), _p(cs), _p(items)))
    res = [idx[offs[i]:offs[i + 1]].copy() for i in range(len(q))]
    assert tot == offs[-1]
    return (res, cs, items[:len(k)]) if return_grid else res


class ORBmatcher:
    """Mirror of the hot-path part of ORB_SLAM3::ORBmatcher (include/ORBmatcher.h:36-101)."""
    TH_HIGH, TH_LOW, HISTO_LENGTH = TH_HIGH, TH_LOW, HISTO_LENGTH

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.mfNNratio, self.mbCheckOrientation, self.device = float(nnratio), bool(checkOri), device

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8).reshape(32)
        b = np.ascontiguousarray(b, np.uint8).reshape(32)
        return lib().orbx_hamming256(_p(a), _p(b))

    def SearchByProjection(self, kpsUn, desc, uRight, bounds, scaleFactors, mapPoints, occupied, th=1.0,
                           bFarPoints=False, thFarPoints=50.0):
        """src/ORBmatcher.cc:41-221 (local map points -> frame, pinhole case).  mapPoints: MP_DTYPE records.
        Returns (nmatches, match[n] = map point index or -1, updated occupied[n])."""
        k = np.ascontiguousarray(kpsUn, KP_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        mp = np.ascontiguousarray(mapPoints, MP_DTYPE)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        occ = np.ascontiguousarray(occupied, np.uint8).copy()
        ur = None if uRight is None else np.ascontiguousarray(uRight, np.float32)
        match = np.full(len(k), -1, np.int32)
        n = _check(lib().orbx_search_by_projection(
            self.device, _p(k), _p(d), None if ur is None else _p(ur), len(k), bounds[0], bounds[1], bounds[2],
            bounds[3], _p(sf), len(sf), _p(mp), len(mp), float(th), int(bFarPoints), float(thFarPoints),
            self.mfNNratio, _p(occ), _p(match)))
        return n, match, occ

    def SearchByProjectionFrame(self, kpsUn, desc, uRight, bounds, projectedPoints, occupied):
        """Matching part of SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1594-1806,
        pinhole case); projectedPoints: PP_DTYPE records computed by the caller's pose / camera projection.
        Returns (nmatches, match[n] = LastFrame point index or -1, updated occupied[n])."""
        k = np.ascontiguousarray(kpsUn, KP_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        pp = np.ascontiguousarray(projectedPoints, PP_DTYPE)
        occ = np.ascontiguousarray(occupied, np.uint8).copy()
        ur = None if uRight is None else np.ascontiguousarray(uRight, np.float32)
        match = np.full(len(k), -1, np.int32)
        n = _check(lib().orbx_search_by_projection_frame(
            self.device, _p(k), _p(d), None if ur is None else _p(ur), len(k), bounds[0], bounds[1], bounds[2],
            bounds[3], _p(pp), len(pp), int(self.mbCheckOrientation), _p(occ), _p(match)))
        return n, match, occ

    def SearchForInitializationBatch(self, ex, first_image, kps1, desc1, bounds2, vbPrevMatched, windowSize=10):
        """SearchForInitialization for the frames of ex's last extraction batch in one call (orbx_search_for_initialization_batch):
        pair f matches F1 = (kps1[f], desc1[f]) -- lists of per-pair arrays -- against image first_image + f of the batch.
        Returns (n_matches [F], list of vnMatches12, list of updated vbPrevMatched)."""
        F = len(kps1)
        n1 = np.array([len(k) for k in kps1], np.int32)
        stride = max(int(n1.max()) if F else 0, 1)
        K = np.zeros((F, stride), KP_DTYPE)
        D = np.zeros((F, stride, 32), np.uint8)
        P = np.zeros((F, stride, 2), np.float32)
        for f in range(F):
            K[f, :n1[f]] = kps1[f]
            D[f, :n1[f]] = np.asarray(desc1[f], np.uint8).reshape(-1, 32)
            P[f, :n1[f]] = np.asarray(vbPrevMatched[f], np.float32).reshape(-1, 2)
        M = np.full((F, stride), -1, np.int32)
        nm = np.zeros(F, np.int32)
        _check(lib().orbx_search_for_initialization_batch(
            ex._h, int(first_image), F, _p(K), _p(D), _p(n1), stride, bounds2[0], bounds2[1], bounds2[2], bounds2[3], _p(P), _p(M),
            int(windowSize), self.mfNNratio, int(self.mbCheckOrientation), _p(nm)))
        return nm, [M[f, :n1[f]].copy() for f in range(F)], [P[f, :n1[f]].copy() for f in range(F)]

    def SearchByProjectionFrameBatch(self, ex, first_image, n_frames, bounds, points, n_points, occupied=None, stereo_pair0=-1):
        """SearchByProjectionFrame on the frames of ex's last extraction batch in one call (include/orbx.h:
        orbx_search_by_projection_frame_batch): points [n_frames][stride] PP_DTYPE, n_points [n_frames].
        Returns (n_matches [n_frames], match [n_frames][cap], occupied [n_frames][cap])."""
        pp = np.ascontiguousarray(points, PP_DTYPE).reshape(n_frames, -1)
        npts = np.ascontiguousarray(n_points, np.int32)
        cap = ex.capacity
        occ_in = None if occupied is None else np.ascontiguousarray(occupied, np.uint8).reshape(n_frames, cap)
        occ = np.zeros((n_frames, cap), np.uint8)
        match = np.full((n_frames, cap), -1, np.int32)
        nm = np.zeros(n_frames, np.int32)
        _check(lib().orbx_search_by_projection_frame_batch(
            ex._h, int(first_image), int(n_frames), bounds[0], bounds[1], bounds[2], bounds[3], _p(pp), _p(npts), pp.shape[1],
            int(self.mbCheckOrientation), int(stereo_pair0), None if occ_in is None else _p(occ_in), _p(occ), _p(match), _p(nm)))
        return nm, match, occ

    def SearchByProjectionFrameBatchDevice(self, ex, first_image, n_frames, bounds, occupied=None, stereo_pair0=-1):
        """SearchByProjectionFrame on the frames of ex's last extraction batch with the views made ON THE DEVICE by
        project_last_frames (orbx_search_by_projection_frame_batch with points = NULL)."""
        npts = np.ascontiguousarray(ex._lf_n[:n_frames], np.int32)
        cap = ex.capacity
        occ_in = None if occupied is None else np.ascontiguousarray(occupied, np.uint8).reshape(n_frames, cap)
        occ = np.zeros((n_frames, cap), np.uint8)
        match = np.full((n_frames, cap), -1, np.int32)
        nm = np.zeros(n_frames, np.int32)
        _check(lib().orbx_search_by_projection_frame_batch(
            ex._h, int(first_image), int(n_frames), bounds[0], bounds[1], bounds[2], bounds[3], None, _p(npts), ex._lf_stride,
            int(self.mbCheckOrientation), int(stereo_pair0), None if occ_in is None else _p(occ_in), _p(occ), _p(match), _p(nm)))
        return nm, match, occ

    def SearchByProjectionBatch(self, ex, first_image, n_frames, bounds, mapPoints, n_map_points, occupied=None, th=1.0,
                                bFarPoints=False, thFarPoints=50.0, stereo_pair0=-1):
        """SearchByProjection (local map points) on the frames of ex's last extraction batch in one call
        (orbx_search_by_projection_batch): mapPoints [n_frames][stride] MP_DTYPE.  Returns (n_matches, match, occupied)."""
        mp = np.ascontiguousarray(mapPoints, MP_DTYPE).reshape(n_frames, -1)
        npts = np.ascontiguousarray(n_map_points, np.int32)
        cap = ex.capacity
        occ_in = None if occupied is None else np.ascontiguousarray(occupied, np.uint8).reshape(n_frames, cap)
        occ = np.zeros((n_frames, cap), np.uint8)
        match = np.full((n_frames, cap), -1, np.int32)
        nm = np.zeros(n_frames, np.int32)
        _check(lib().orbx_search_by_projection_batch(
            ex._h, int(first_image), int(n_frames), bounds[0], bounds[1], bounds[2], bounds[3], _p(mp), _p(npts), mp.shape[1],
            float(th), int(bFarPoints), float(thFarPoints), self.mfNNratio, int(stereo_pair0),
            None if occ_in is None else _p(occ_in), _p(occ), _p(match), _p(nm)))
        return nm, match, occ

    def SearchByProjectionBatchDevice(self, ex, first_image, n_frames, bounds, occupied=None, th=1.0, bFarPoints=False,
                                      thFarPoints=50.0, stereo_pair0=-1):
        """SearchByProjection (local map points) on the frames of ex's last extraction batch with the views made ON THE DEVICE by
        project_map_points (orbx_search_by_projection_batch with map_points = NULL)."""
        n = ex._map_n
        npts = np.full(n_frames, n, np.int32)
        cap = ex.capacity
        occ_in = None if occupied is None else np.ascontiguousarray(occupied, np.uint8).reshape(n_frames, cap)
        occ = np.zeros((n_frames, cap), np.uint8)
        match = np.full((n_frames, cap), -1, np.int32)
        nm = np.zeros(n_frames, np.int32)
        _check(lib().orbx_search_by_projection_batch(
            ex._h, int(first_image), int(n_frames), bounds[0], bounds[1], bounds[2], bounds[3], None, _p(npts), n,
            float(th), int(bFarPoints), float(thFarPoints), self.mfNNratio, int(stereo_pair0),
            None if occ_in is None else _p(occ_in), _p(occ), _p(match), _p(nm)))
        return nm, match, occ

    def SearchByProjectionKeyFrame(self, kpsUn, desc, bounds, projectedPoints, occupied, ORBdist=100):
        """Matching part of the relocalisation matcher SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
        (src/ORBmatcher.cc:1808-1918); projectedPoints: PP_DTYPE records of pKF's map points after the caller's projection
        and gates; occupied[i2] <=> CurrentFrame.mvpMapPoints[i2] != NULL.
        Returns (nmatches, match[n] = point index or -1, updated occupied[n])."""
        k = np.ascontiguousarray(kpsUn, KP_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        pp = np.ascontiguousarray(projectedPoints, PP_DTYPE)
        occ = np.ascontiguousarray(occupied, np.uint8).copy()
        match = np.full(len(k), -1, np.int32)
        n = _check(lib().orbx_search_by_projection_keyframe(
            self.device, _p(k), _p(d), len(k), bounds[0], bounds[1], bounds[2], bounds[3], _p(pp), len(pp), int(ORBdist),
            int(self.mbCheckOrientation), _p(occ), _p(match)))
        return n, match, occ

    def FuseSearch(self, kps, desc, uRight, bounds, invLevelSigma2, points, maxDist=TH_LOW):
        """The search of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (src/ORBmatcher.cc:1195-1256); points: FP_DTYPE records
        of the map points after the caller's projection and gates.  Returns (nFused, bestIdx[n_points] = keypoint index or -1,
        bestDist[n_points])."""
        k = np.ascontiguousarray(kps, KP_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        pp = np.ascontiguousarray(points, FP_DTYPE)
        ur = None if uRight is None else np.ascontiguousarray(uRight, np.float32)
        isg = np.ascontiguousarray(invLevelSigma2, np.float32)
        bi, bd = np.full(len(pp), -1, np.int32), np.full(len(pp), 256, np.int32)
        n = _check(lib().orbx_fuse_search(self.device, _p(k), _p(d), None if ur is None else _p(ur), len(k), bounds[0], bounds[1],
                                          bounds[2], bounds[3], _p(isg), len(isg), _p(pp), len(pp), int(maxDist), _p(bi), _p(bd)))
        return n, bi, bd

    def SearchBySim3(self, kps1, desc1, bounds1, kps2, desc2, bounds2, points1in2, points2in1):
        """ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1392-1592): pKF1's map points searched in pKF2 and pKF2's in pKF1 (FP_DTYPE
        records after the caller's Sim3 projections; one record per feature of the key frame they come from), TH_HIGH, no
        chi-square gate, then the agreement check.  Returns (nFound, vnMatch12[N1] = feature of pKF2 or -1)."""
        nl1 = int(np.max(np.ascontiguousarray(kps1, KP_DTYPE)["octave"], initial=0)) + 1
        nl2 = int(np.max(np.ascontiguousarray(kps2, KP_DTYPE)["octave"], initial=0)) + 1
        _, m1, _ = self.FuseSearch(kps2, desc2, None, bounds2, np.zeros(nl2, np.float32), points1in2, TH_HIGH)
        _, m2, _ = self.FuseSearch(kps1, desc1, None, bounds1, np.zeros(nl1, np.float32), points2in1, TH_HIGH)
        i1 = np.arange(len(m1))
        ok = (m1 >= 0) & (m1 < len(m2))
        ok[ok] = m2[m1[ok]] == i1[ok]
        out = np.where(ok, m1, -1).astype(np.int32)
        return int(ok.sum()), out

    def SearchForTriangulationRig(self, fv1, kps1, desc1, hasMapPoint1, nLeft1, fv2, kps2, desc2, hasMapPoint2, nLeft2, levelSigma2_1,
                                  levelSigma2_2, rig, bOnlyStereo=False, bCoarse=False):
        """ORBmatcher::SearchForTriangulation for two-camera key frames (src/ORBmatcher.cc:906-923,1007-1064): kps / desc hold
        mvKeys | mvKeysRight, rig = a TRI_RIG_DTYPE record.  Returns (nmatches, vMatches12[n1])."""
        n1n, s1, f1 = (np.ascontiguousarray(fv1[0], np.uint32), np.ascontiguousarray(fv1[1], np.int32), np.ascontiguousarray(fv1[2], np.uint32))
        n2n, s2, f2 = (np.ascontiguousarray(fv2[0], np.uint32), np.ascontiguousarray(fv2[1], np.int32), np.ascontiguousarray(fv2[2], np.uint32))
        k1, k2 = np.ascontiguousarray(kps1, KP_DTYPE), np.ascontiguousarray(kps2, KP_DTYPE)
        d1, d2 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(desc2, np.uint8)
        h1, h2 = np.ascontiguousarray(hasMapPoint1, np.uint8), np.ascontiguousarray(hasMapPoint2, np.uint8)
        g1, g2 = np.ascontiguousarray(levelSigma2_1, np.float32), np.ascontiguousarray(levelSigma2_2, np.float32)
        rg = np.ascontiguousarray(rig, TRI_RIG_DTYPE)
        m = np.full(len(k1), -1, np.int32)
        n = _check(lib().orbx_search_for_triangulation_rig(
            self.device, _p(n1n), _p(s1), _p(f1), len(n1n), _p(k1), _p(d1), _p(h1), int(nLeft1), len(k1), _p(n2n), _p(s2), _p(f2), len(n2n),
            _p(k2), _p(d2), _p(h2), int(nLeft2), len(k2), _p(g1), _p(g2), len(g1), _p(rg), int(bOnlyStereo), int(bCoarse),
            int(self.mbCheckOrientation), _p(m)))
        return n, m

    def SearchForTriangulation(self, fv1, kps1, desc1, hasMapPoint1, uRight1, fv2, kps2, desc2, hasMapPoint2, uRight2,
                               scaleFactors2, levelSigma2_2, ep, F12, bOnlyStereo=False, bCoarse=False):
        """ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (src/ORBmatcher.cc:886-1106),
        single-camera key frames; fv = (node ids, node start, feature indices) as ORBVocabulary.transform returns them.
        Returns (nmatches, vMatchedPairs as an [nmatches, 2] array in ascending idx1, vMatches12[n1])."""
        n1n, s1, f1 = (np.ascontiguousarray(fv1[0], np.uint32), np.ascontiguousarray(fv1[1], np.int32), np.ascontiguousarray(fv1[2], np.uint32))
        n2n, s2, f2 = (np.ascontiguousarray(fv2[0], np.uint32), np.ascontiguousarray(fv2[1], np.int32), np.ascontiguousarray(fv2[2], np.uint32))
        k1, k2 = np.ascontiguousarray(kps1, KP_DTYPE), np.ascontiguousarray(kps2, KP_DTYPE)
        d1, d2 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(desc2, np.uint8)
        h1, h2 = np.ascontiguousarray(hasMapPoint1, np.uint8), np.ascontiguousarray(hasMapPoint2, np.uint8)
        u1 = None if uRight1 is None else np.ascontiguousarray(uRight1, np.float32)
        u2 = None if uRight2 is None else np.ascontiguousarray(uRight2, np.float32)
        sf, sg = np.ascontiguousarray(scaleFactors2, np.float32), np.ascontiguousarray(levelSigma2_2, np.float32)
        epa = np.ascontiguousarray(ep, np.float32)
        Fa = None if F12 is None else np.ascontiguousarray(F12, np.float32).reshape(9)
        m = np.full(len(k1), -1, np.int32)
        n = _check(lib().orbx_search_for_triangulation(
            self.device, _p(n1n), _p(s1), _p(f1), len(n1n), _p(k1), _p(d1), _p(h1), None if u1 is None else _p(u1), len(k1),
            _p(n2n), _p(s2), _p(f2), len(n2n), _p(k2), _p(d2), _p(h2), None if u2 is None else _p(u2), len(k2), _p(sf), _p(sg),
            len(sf), _p(epa), None if Fa is None else _p(Fa), int(bOnlyStereo), int(bCoarse), int(self.mbCheckOrientation), _p(m)))
        idx1 = np.nonzero(m >= 0)[0]
        return n, np.stack([idx1, m[idx1]], axis=1).astype(np.int64), m

    def SearchByProjectionFisheye(self, kps, desc, n_left, bounds, scaleFactors, mapPoints, mapPointsRight, leftToRight,
                                  rightToLeft, occupied, th=1.0, bFarPoints=False, thFarPoints=50.0):
        """src/ORBmatcher.cc:41-221 with F.Nleft != -1: kps / desc = mvKeys then mvKeysRight (N = n_left + n_right rows),
        mapPointsRight = MPR_DTYPE records.  Returns (nmatches, match[N], updated occupied[N])."""
        k = np.ascontiguousarray(kps, KP_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        mp, mr = np.ascontiguousarray(mapPoints, MP_DTYPE), np.ascontiguousarray(mapPointsRight, MPR_DTYPE)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        l2r, r2l = np.ascontiguousarray(leftToRight, np.int32), np.ascontiguousarray(rightToLeft, np.int32)
        occ = np.ascontiguousarray(occupied, np.uint8).copy()
        match = np.full(len(k), -1, np.int32)
        n = _check(lib().orbx_search_by_projection_fisheye(
            self.device, _p(k), _p(d), int(n_left), len(k) - int(n_left), bounds[0], bounds[1], bounds[2], bounds[3], _p(sf),
            len(sf), _p(mp), _p(mr), len(mp), float(th), int(bFarPoints), float(thFarPoints), self.mfNNratio, _p(l2r), _p(r2l),
            _p(occ), _p(match)))
        return n, match, occ

    def SearchByProjectionFrameFisheye(self, kps, desc, n_left, bounds, projectedPoints, uvRight, occupied):
        """src/ORBmatcher.cc:1594-1806 with CurrentFrame.Nleft != -1; uvRight[i] = projection of point i into the right
        camera.  Returns (nmatches, match[N], updated occupied[N])."""
        k = np.ascontiguousarray(kps, KP_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        pp = np.ascontiguousarray(projectedPoints, PP_DTYPE)
        uv = np.ascontiguousarray(uvRight, np.float32).reshape(-1, 2)
        occ = np.ascontiguousarray(occupied, np.uint8).copy()
        match = np.full(len(k), -1, np.int32)
        n = _check(lib().orbx_search_by_projection_frame_fisheye(
            self.device, _p(k), _p(d), int(n_left), len(k) - int(n_left), bounds[0], bounds[1], bounds[2], bounds[3], _p(pp),
            _p(uv), len(pp), int(self.mbCheckOrientation), _p(occ), _p(match)))
        return n, match, occ

    def SearchByProjectionFisheyeBatch(self, ex, first_left, first_right, n_frames, bounds, mapPoints, mapPointsRight, n_points,
                                       leftToRight, rightToLeft, occupied=None, th=1.0, bFarPoints=False, thFarPoints=50.0):
        """SearchByProjectionFisheye on the two-camera frames of ex's last extraction batch in one call
        (orbx_search_by_projection_fisheye_batch): frame f = images first_left + f / first_right + f; mapPoints / mapPointsRight
        [n_frames][stride], leftToRight / rightToLeft [n_frames][cap], occupied [n_frames][2 cap] (rows [left | right]).
        Returns (n_matches [n_frames], match [n_frames][2 cap], occupied [n_frames][2 cap])."""
        cap = ex.capacity
        mp = np.ascontiguousarray(mapPoints, MP_DTYPE).reshape(n_frames, -1)
        mr = np.ascontiguousarray(mapPointsRight, MPR_DTYPE).reshape(n_frames, -1)
        npts = np.ascontiguousarray(n_points, np.int32)
        l2r = np.ascontiguousarray(leftToRight, np.int32).reshape(n_frames, cap)
        r2l = np.ascontiguousarray(rightToLeft, np.int32).reshape(n_frames, cap)
        occ_in = None if occupied is None else np.ascontiguousarray(occupied, np.uint8).reshape(n_frames, 2 * cap)
        occ, match, nm = np.zeros((n_frames, 2 * cap), np.uint8), np.full((n_frames, 2 * cap), -1, np.int32), np.zeros(n_frames, np.int32)
        _check(lib().orbx_search_by_projection_fisheye_batch(
            ex._h, int(first_left), int(first_right), int(n_frames), bounds[0], bounds[1], bounds[2], bounds[3], _p(mp), _p(mr), _p(npts),
            mp.shape[1], float(th), int(bFarPoints), float(thFarPoints), self.mfNNratio, _p(l2r), _p(r2l),
            None if occ_in is None else _p(occ_in), _p(occ), _p(match), _p(nm)))
        return nm, match, occ

    def SearchByProjectionFisheyeBatchDevice(self, ex, first_left, first_right, n_frames, bounds, leftToRight, rightToLeft, occupied=None,
                                             th=1.0, bFarPoints=False, thFarPoints=50.0):
        """SearchByProjectionFisheye on the two-camera frames of ex's last extraction batch with both cameras' views made ON THE
        DEVICE by project_map_points_fisheye (orbx_search_by_projection_fisheye_batch with map_points = map_points_right = NULL)."""
        cap, n = ex.capacity, ex._map_n
        npts = np.full(n_frames, n, np.int32)
        l2r = np.ascontiguousarray(leftToRight, np.int32).reshape(n_frames, cap)
        r2l = np.ascontiguousarray(rightToLeft, np.int32).reshape(n_frames, cap)
        occ_in = None if occupied is None else np.ascontiguousarray(occupied, np.uint8).reshape(n_frames, 2 * cap)
        occ, match, nm = np.zeros((n_frames, 2 * cap), np.uint8), np.full((n_frames, 2 * cap), -1, np.int32), np.zeros(n_frames, np.int32)
        _check(lib().orbx_search_by_projection_fisheye_batch(
            ex._h, int(first_left), int(first_right), int(n_frames), bounds[0], bounds[1], bounds[2], bounds[3], None, None, _p(npts), n,
            float(th), int(bFarPoints), float(thFarPoints), self.mfNNratio, _p(l2r), _p(r2l),
            None if occ_in is None else _p(occ_in), _p(occ), _p(match), _p(nm)))
        return nm, match, occ

    def SearchByProjectionFrameFisheyeBatch(self, ex, first_left, first_right, n_frames, bounds, points, uvRight, n_points, occupied=None):
        """SearchByProjectionFrameFisheye on the two-camera frames of ex's last extraction batch in one call
        (orbx_search_by_projection_frame_fisheye_batch): points [n_frames][stride] PP_DTYPE, uvRight [n_frames][stride][2].
        Returns (n_matches, match [n_frames][2 cap], occupied [n_frames][2 cap])."""
        cap = ex.capacity
        pp = np.ascontiguousarray(points, PP_DTYPE).reshape(n_frames, -1)
        uv = np.ascontiguousarray(uvRight, np.float32).reshape(n_frames, pp.shape[1], 2)
        npts = np.ascontiguousarray(n_points, np.int32)
        occ_in = None if occupied is None else np.ascontiguousarray(occupied, np.uint8).reshape(n_frames, 2 * cap)
        occ, match, nm = np.zeros((n_frames, 2 * cap), np.uint8), np.full((n_frames, 2 * cap), -1, np.int32), np.zeros(n_frames, np.int32)
        _check(lib().orbx_search_by_projection_frame_fisheye_batch(
            ex._h, int(first_left), int(first_right), int(n_frames), bounds[0], bounds[1], bounds[2], bounds[3], _p(pp), _p(uv), _p(npts),
            pp.shape[1], int(self.mbCheckOrientation), None if occ_in is None else _p(occ_in), _p(occ), _p(match), _p(nm)))
        return nm, match, occ

    def SearchForInitialization(self, kps1, desc1, kps2, desc2, bounds2, vbPrevMatched, windowSize=10):
        """src/ORBmatcher.cc:618-764.  kps = mvKeysUn of F1 / F2, bounds2 = (mnMinX, mnMinY, mnMaxX, mnMaxY)
        of F2.  Returns (nmatches, vnMatches12, updated vbPrevMatched)."""
        k1 = np.ascontiguousarray(kps1, KP_DTYPE)
        k2 = np.ascontiguousarray(kps2, KP_DTYPE)
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        prev = np.ascontiguousarray(vbPrevMatched, np.float32).reshape(-1, 2).copy()
        assert len(prev) == len(k1)
        m12 = np.full(len(k1), -1, np.int32)
        n = _check(lib().orbx_search_for_initialization(
            self.device, _p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), bounds2[0], bounds2[1], bounds2[2],
            bounds2[3], _p(prev), _p(m12), int(windowSize), self.mfNNratio, int(self.mbCheckOrientation)))
        return n, m12, prev
