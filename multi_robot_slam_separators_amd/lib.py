"""ctypes binding of the product library libsepfinder.so (C-ABI: include/sepfinder.h).

There is NO CPU fallback: if the shared library is missing, or no GPU is visible, every entry
point raises.  PyTorch is imported first (when installed) only so that this process ends up with
ONE HIP runtime: torch bundles libamdhip64.so (SONAME libamdhip64.so.7) and the library's
NEEDED entry resolves to the copy that is already loaded.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SEPFINDER_LIB") or os.path.join(_HERE, "libsepfinder.so")   # override: A/B builds
_lib = None


class SepfinderError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (_abi.STATUS_NAMES.get(code, code), msg))
        self.code = code


def build(force=False):
    """Compile the HIP sources for gfx950 (csrc/Makefile, hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-s", "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the separator-finder path)" % LIB_PATH)
    try:  # one HIP runtime per process (see module docstring)
        import torch  # noqa: F401
    except Exception:  # torch is plumbing, not a requirement of the C-ABI itself
        for cand in ("/opt/rocm/lib/libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
                break
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    sig = {
        "sf_abi_version": (C.c_int, []),
        "sf_default_params": (None, [P(_abi.Params)]),
        "sf_create": (C.c_int, [P(_abi.Params), C.c_int, P(vp)]),
        "sf_destroy": (None, [vp]),
        "sf_last_error": (C.c_char_p, [vp]),
        "sf_get_params": (C.c_int, [vp, P(_abi.Params)]),
        "sf_set_stream": (C.c_int, [vp, vp]),
        "sf_synchronize": (C.c_int, [vp]),
        "sf_nn_append_local": (C.c_int, [vp, vp, i32, i32]),
        "sf_nn_append_received": (C.c_int, [vp, vp, i32, i32]),
        "sf_nn_append_local_f32_device": (C.c_int, [vp, vp, i32, i32]),
        "sf_nn_append_received_f32_device": (C.c_int, [vp, vp, i32, i32]),
        "sf_nn_append_local_f16_device": (C.c_int, [vp, vp, i32, i32]),
        "sf_nn_append_received_f16_device": (C.c_int, [vp, vp, i32, i32]),
        "sf_nn_sizes": (C.c_int, [vp, P(i32), P(i32)]),
        "sf_nn_mark_local_used": (C.c_int, [vp, i32]),
        "sf_nn_mark_other_used": (C.c_int, [vp, i32]),
        "sf_nn_ignore_pair": (C.c_int, [vp, i32, i32]),
        "sf_nn_reset": (C.c_int, [vp]),
        "sf_nn_set_precision": (C.c_int, [vp, i32]),
        "sf_set_option": (C.c_int, [vp, i32, i32]),
        "sf_nn_find_matches": (C.c_int, [vp, vp, i32, P(i32)]),
        "sf_nn_last_row_minima": (C.c_int, [vp, vp, vp, i32]),
        "sf_nn_last_filter_dims": (C.c_int, [vp, P(i32)]),
        "sf_nn_walk": (C.c_int, [vp, vp, vp, i32, i32, vp, i32, P(i32)]),
        "sf_store_add_keyframe": (C.c_int, [vp, P(_abi.Features), P(i32)]),
        "sf_store_add_keyframes_device": (C.c_int, [vp, i32, i32, i32, vp, vp, vp, P(i32)]),
        "sf_brief_set_pattern": (C.c_int, [vp, vp, i32]),
        "sf_brief_get_pattern": (C.c_int, [vp, vp, i32, P(i32)]),
        "sf_orb_defaults": (None, [P(_abi.OrbParams)]),
        "sf_set_feature_type": (C.c_int, [vp, i32, P(_abi.OrbParams)]),
        "sf_get_feature_type": (C.c_int, [vp, P(i32), P(_abi.OrbParams)]),
        "sf_orb_set_pattern": (C.c_int, [vp, vp, i32]),
        "sf_orb_get_pattern": (C.c_int, [vp, vp, i32, P(i32)]),
        "sf_extract_keyframe_device": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp, i32, P(_abi.StereoCamera),
                                                 P(i32), P(i32), vp, vp, vp]),
        "sf_fast_defaults": (None, [P(_abi.FastParams)]),
        "sf_fast_set_params": (C.c_int, [vp, P(_abi.FastParams)]),
        "sf_fast_get_params": (C.c_int, [vp, P(_abi.FastParams)]),
        "sf_detect_fast_device": (C.c_int, [vp, vp, i32, i32, i32, i32, P(_abi.FastParams), vp, i32, P(i32)]),
        "sf_gftt_defaults": (None, [P(_abi.GfttParams)]),
        "sf_gftt_set_params": (C.c_int, [vp, P(_abi.GfttParams)]),
        "sf_gftt_get_params": (C.c_int, [vp, P(_abi.GfttParams)]),
        "sf_gftt_check_params": (C.c_int, [P(_abi.GfttParams)]),
        "sf_front_defaults": (None, [P(_abi.FrontParams)]),
        "sf_front_set_params": (C.c_int, [vp, P(_abi.FrontParams)]),
        "sf_front_get_params": (C.c_int, [vp, P(_abi.FrontParams)]),
        "sf_compute_roi": (C.c_int, [i32, i32, P(C.c_float), P(i32)]),
        "sf_corner_subpix_device": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, i32, i32, C.c_float]),
        "sf_orb_detector_defaults": (None, [P(_abi.OrbDetectorParams)]),
        "sf_set_feature_type_orb": (C.c_int, [vp, P(_abi.OrbDetectorParams), P(_abi.OrbParams)]),
        "sf_get_orb_detector": (C.c_int, [vp, P(_abi.OrbDetectorParams)]),
        "sf_detect_orb_device": (C.c_int, [vp, vp, i32, i32, i32, i32, P(_abi.OrbDetectorParams), P(_abi.OrbParams), vp, i32,
                                           P(i32)]),
        "sf_freak_defaults": (None, [P(_abi.FreakParams)]),
        "sf_set_feature_type_freak": (C.c_int, [vp, i32, P(_abi.FreakParams)]),
        "sf_get_freak_params": (C.c_int, [vp, P(_abi.FreakParams)]),
        "sf_freak_set_pairs": (C.c_int, [vp, vp, i32]),
        "sf_freak_get_pairs": (C.c_int, [vp, vp, i32, P(i32)]),
        "sf_freak_build_pattern": (C.c_int, [P(_abi.FreakParams), vp, vp]),
        "sf_freak_default_pairs": (None, [vp]),
        "sf_surf_defaults": (None, [P(_abi.SurfParams)]),
        "sf_set_feature_type_surf": (C.c_int, [vp, P(_abi.SurfParams)]),
        "sf_get_surf_params": (C.c_int, [vp, P(_abi.SurfParams)]),
        "sf_detect_surf_device": (C.c_int, [vp, vp, i32, i32, i32, i32, P(_abi.SurfParams), vp, i32, P(i32)]),
        "sf_surf_build_tables": (None, [vp, vp, vp]),
        "sf_surf_check_params": (C.c_int, [P(_abi.SurfParams)]),
        "sf_surf_batch_status": (C.c_int, [vp, P(i32)]),
        "sf_debug_surf_limits": (C.c_int, [vp, i32, i32]),
        "sf_surf_batch_plan": (C.c_int, [i32, i32, P(_abi.SurfParams), i32, P(i32), P(i32), P(i64)]),
        "sf_sift_defaults": (None, [P(_abi.SiftParams)]),
        "sf_set_feature_type_sift": (C.c_int, [vp, P(_abi.SiftParams)]),
        "sf_get_sift_params": (C.c_int, [vp, P(_abi.SiftParams)]),
        "sf_detect_sift_device": (C.c_int, [vp, vp, i32, i32, i32, i32, P(_abi.SiftParams), vp, i32, P(i32)]),
        "sf_sift_check_params": (C.c_int, [P(_abi.SiftParams)]),
        "sf_sift_build_tables": (C.c_int, [P(_abi.SiftParams), vp, vp, vp]),
        "sf_sift_plan": (C.c_int, [i32, i32, P(_abi.SiftParams), P(i32), vp, vp, P(i64), P(i64)]),
        "sf_debug_sift_limits": (C.c_int, [vp, i32]),
        "sf_debug_sift_plane": (C.c_int, [vp, i32, i32, i32, vp]),
        "sf_sift_batch_status": (C.c_int, [vp, P(i32)]),
        "sf_debug_sift_batch_chunk": (C.c_int, [vp, i32]),
        "sf_sift_batch_plan": (C.c_int, [i32, i32, P(_abi.SiftParams), i32, P(i32), P(i32), P(i64)]),
        "sf_detect_corners_device": (C.c_int, [vp, vp, i32, i32, i32, i32, C.c_double, C.c_double, vp, i32, P(i32)]),
        "sf_stereo_flow_defaults": (None, [P(_abi.StereoFlowParams)]),
        "sf_detector_defaults": (None, [P(_abi.DetectorParams)]),
        "sf_get_features_and_descriptor": (C.c_int, [vp, vp, vp, i32, i32, i32, P(_abi.StereoCamera), P(_abi.DetectorParams),
                                                     P(_abi.StereoFlowParams), vp, vp, vp, i32, P(i32), P(i32)]),
        "sf_stereo_correspondences_device": (C.c_int, [vp, vp, vp, i32, i32, i32, vp, i32, P(_abi.StereoFlowParams),
                                                       vp, vp, vp, vp]),
        "sf_grid_defaults": (None, [P(_abi.GridParams)]),
        "sf_grid_set_params": (C.c_int, [vp, P(_abi.GridParams)]),
        "sf_grid_get_params": (C.c_int, [vp, P(_abi.GridParams)]),
        "sf_compute_grid": (C.c_int, [i32, i32, P(C.c_float), P(_abi.GridParams), i32, P(i32)]),
        "sf_stereo_defaults": (None, [P(_abi.StereoParams)]),
        "sf_stereo_set_params": (C.c_int, [vp, P(_abi.StereoParams)]),
        "sf_stereo_get_params": (C.c_int, [vp, P(_abi.StereoParams)]),
        "sf_stereo_block_match_device": (C.c_int, [vp, vp, vp, i32, i32, i32, vp, i32, P(_abi.StereoFlowParams), i32,
                                                   vp, vp, vp, vp]),
        "sf_netvlad_load": (C.c_int, [vp, P(_abi.NetvladWeights)]),
        "sf_netvlad_infer_device": (C.c_int, [vp, vp, i32, i32, vp, i32]),
        "sf_netvlad_infer_batch_device": (C.c_int, [vp, vp, i32, i32, i32, vp, i32]),
        "sf_store_size": (C.c_int, [vp, P(i32)]),
        "sf_store_export_plan": (C.c_int, [vp, i32, i32, P(C.c_uint64), P(i32)]),
        "sf_store_export_keyframes_device": (C.c_int, [vp, i32, i32, vp, C.c_uint64]),
        "sf_store_import_keyframes_device": (C.c_int, [vp, vp, C.c_uint64, i32, i32, i32, P(i32)]),
        "sf_store_wire_status": (C.c_int, [vp, P(i32)]),
        "sf_store_clear": (C.c_int, [vp]),
        "sf_camera_add": (C.c_int, [vp, P(_abi.CameraModel), P(i32)]),
        "sf_camera_get": (C.c_int, [vp, i32, P(_abi.CameraModel)]),
        "sf_camera_count": (C.c_int, [vp, P(i32)]),
        "sf_camera_select": (C.c_int, [vp, i32]),
        "sf_store_set_camera": (C.c_int, [vp, i32, i32, i32]),
        "sf_store_get_camera": (C.c_int, [vp, i32, P(i32)]),
        "sf_estimate_transform": (C.c_int, [vp, P(_abi.Features), P(_abi.Features), vp]),
        "sf_estimate_transform_batch": (C.c_int, [vp, P(_abi.Features), P(_abi.Features), i32, vp]),
        "sf_verify_pairs": (C.c_int, [vp, vp, vp, i32, vp]),
        "sf_verify_pairs_device": (C.c_int, [vp, vp, vp, i32, vp]),
        "sf_verify_matches_device": (C.c_int, [vp, vp, i32, i32, i32, vp]),
        "sf_find_matches_and_verify_device": (C.c_int, [vp, i32, i32, vp, i32, C.POINTER(i32), vp]),
        "sf_compact_accepted_device": (C.c_int, [vp, vp, i32, vp, vp, P(i32)]),
        "sf_compact_accepted_device_async": (C.c_int, [vp, vp, i32, vp, vp, vp]),
        "sf_step_issue": (C.c_int, [vp, i32, i32]),
        "sf_step_retire": (C.c_int, [vp, P(_abi.StepResult)]),
        "sf_memcpy_device_async": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
        "sf_step_mirror": (C.c_int, [vp, vp, vp, i32]),
        "sf_step_mirror_pair": (C.c_int, [vp, vp, vp, vp, vp, i32]),
        "sf_step_mirror_streams": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
        "sf_accept_stream_set": (C.c_int, [vp, i32, vp, vp, vp, i32, vp, vp]),
        "sf_accept_stream_select": (C.c_int, [vp, i32]),
        "sf_accept_stream_status": (C.c_int, [vp, P(i32), P(i32)]),
        "sf_compact_accepted_indexed_mirrored_device_async": (C.c_int, [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "sf_last_match_results": (C.c_int, [vp, P(vp), P(vp), P(i32)]),
        "sf_compact_accepted_indexed_device_async": (C.c_int, [vp, vp, vp, i32, vp, vp, vp]),
        "sf_debug_correspondences": (C.c_int, [vp, i32, i32, vp, vp, i32, P(i32)]),
        "sf_debug_pass_state": (C.c_int, [vp, i32, i32, vp, P(i32), P(i32), P(i32)]),
        "sf_debug_counters": (C.c_int, [vp, vp, i32]),
        "sf_debug_knn2_u8": (C.c_int, [vp, i32, i32, vp, vp, vp]),
        "sf_debug_guided_points": (C.c_int, [vp, i32, vp, vp, P(i32)]),
        "sf_debug_plan_workspace": (C.c_int, [P(_abi.Params), i32, i32, i32, i32, i32, P(i64), i32]),
        "sf_debug_live_resources": (None, [P(i64)]),
        "sf_pack_separators": (C.c_int, [vp, i32, C.c_int8, C.c_int8, vp, vp, vp, vp, vp]),
        "sf_comm_unique_id": (C.c_int, [vp, i32]),
        "sf_comm_init": (C.c_int, [vp, vp, i32, i32]),
        "sf_comm_destroy": (C.c_int, [vp]),
        "sf_allgather_separators": (C.c_int, [vp, vp, i32, vp, i32, vp]),
        "sf_allgather_separators_device": (C.c_int, [vp, vp, vp, i32]),
        "sf_allgather_bytes_device": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "sf_nn_row_minima_device": (C.c_int, [vp, vp, vp, vp]),
        "sf_nn_walk_device": (C.c_int, [vp, vp, vp, vp, i32, i32, vp, i32, vp]),
        "sf_get_features_and_descriptor_batch_device": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, C.c_size_t, vp, vp, vp,
                                                                   P(i32), vp, vp, vp, vp]),
        "sf_image_set_gray_rule": (C.c_int, [vp, i32]),
        "sf_image_get_gray_rule": (C.c_int, [vp, P(i32)]),
        "sf_image_to_gray_device": (C.c_int, [vp, vp, i32, i32, i32, i32, C.c_size_t, i32, vp, i32, C.c_size_t]),
        "sf_netvlad_infer_u8_batch_device": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, C.c_size_t, vp, i32]),
        "sf_get_features_and_descriptor_u8": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, P(_abi.StereoCamera),
                                                        P(_abi.DetectorParams), P(_abi.StereoFlowParams), vp, vp, vp, i32,
                                                        P(i32), P(i32)]),
        "sf_add_keyframes_u8_batch_device": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, C.c_size_t,
                                                       P(_abi.StereoCamera), P(_abi.DetectorParams),
                                                       P(_abi.StereoFlowParams), P(i32), P(i32), vp, vp, vp, vp]),
        "sf_rectify_check_info": (C.c_int, [P(_abi.CameraInfo), vp]),
        "sf_rectify_plan_create": (C.c_int, [vp, P(_abi.CameraInfo), P(i32)]),
        "sf_rectify_plan_from_maps": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, P(i32)]),
        "sf_rectify_plan_count": (C.c_int, [vp, P(i32)]),
        "sf_rectify_plan_get": (C.c_int, [vp, i32, P(_abi.CameraInfo), P(i32)]),
        "sf_rectify_plan_clear": (C.c_int, [vp]),
        "sf_rectify_maps_device": (C.c_int, [vp, i32, vp, vp, i32]),
        "sf_image_rectify_device": (C.c_int, [vp, i32, vp, i32, vp, i32, i32, i32, i32, C.c_size_t, vp, vp, i32, C.c_size_t]),
        "sf_stereo_camera_from_info": (C.c_int, [P(_abi.CameraInfo), P(_abi.CameraInfo), vp, P(_abi.StereoCamera)]),
        "sf_depth_defaults": (None, [P(_abi.DepthParams)]),
        "sf_depth_set_params": (C.c_int, [vp, P(_abi.DepthParams)]),
        "sf_depth_get_params": (C.c_int, [vp, P(_abi.DepthParams)]),
        "sf_depth_mask_device": (C.c_int, [vp, vp, i32, i32, i32, i32, C.c_size_t, i32, C.c_float, C.c_float, vp, i32,
                                           C.c_size_t]),
        "sf_depth_set_size": (C.c_int, [vp, P(_abi.DepthSize)]),
        "sf_depth_get_size": (C.c_int, [vp, P(_abi.DepthSize)]),
        "sf_depth_interpolation_factor": (C.c_int, [i32, i32, i32, i32]),
        "sf_depth_interpolate_device": (C.c_int, [vp, vp, i32, i32, i32, i32, C.c_size_t, i32, i32, vp, i32, C.c_size_t]),
        "sf_depth_points_device": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, i32, P(_abi.StereoCamera), vp, vp]),
        "sf_detect_corners_masked_device": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, i32, C.c_double, C.c_double, vp, i32,
                                                      P(i32)]),
        "sf_detect_fast_masked_device": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, i32, P(_abi.FastParams), vp, i32, P(i32)]),
        "sf_extract_keyframe_depth_device": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, P(_abi.StereoCamera),
                                                       P(i32), P(i32), vp, vp, vp]),
        "sf_get_features_and_descriptor_depth": (C.c_int, [vp, vp, i32, vp, i32, i32, i32, i32, i32, P(_abi.StereoCamera),
                                                           P(_abi.DetectorParams), vp, vp, vp, i32, P(i32), P(i32)]),
        "sf_get_features_and_descriptor_depth_batch_device": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, C.c_size_t, i32,
                                                                         C.c_size_t, P(_abi.StereoCamera),
                                                                         P(_abi.DetectorParams), P(i32), vp, vp, vp, vp]),
        "sf_add_keyframes_depth_batch_device": (C.c_int, [vp, vp, i32, vp, i32, i32, i32, i32, i32, C.c_size_t, i32,
                                                          C.c_size_t, P(_abi.StereoCamera), P(_abi.DetectorParams), P(i32),
                                                          P(i32), vp, vp, vp, vp]),
        "sf_depth_registration_defaults": (None, [P(_abi.DepthRegistration)]),
        "sf_depth_register_check": (C.c_int, [P(_abi.DepthRegistration)]),
        "sf_depth_register_device": (C.c_int, [vp, P(_abi.DepthRegistration), vp, i32, i32, C.c_size_t, i32, vp, i32, C.c_size_t]),
        "sf_depth_fill_holes_device": (C.c_int, [vp, vp, i32, i32, i32, i32, C.c_size_t, i32, i32, i32, vp, i32, C.c_size_t]),
        "sf_debug_depth_register_limits": (C.c_int, [vp, i32, i32]),
        "sf_prof_enable": (C.c_int, [vp, C.c_int]),
        "sf_prof_select": (C.c_int, [vp, C.c_uint32]),
        "sf_stream_placement": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
        "sf_streams_prepare": (C.c_int, [vp]),
        "sf_prof_reset": (C.c_int, [vp]),
        "sf_prof_get": (C.c_int, [vp, C.c_int, P(i64), P(C.c_double)]),
        "sf_kernel_name": (C.c_char_p, [C.c_int]),
    }
    # the batch forms of Vis/FeatureType 2: the argument lists of their generic twins
    sig["sf_get_features_and_descriptor_orb_batch_device"] = sig["sf_get_features_and_descriptor_batch_device"]
    sig["sf_add_keyframes_orb_u8_batch_device"] = sig["sf_add_keyframes_u8_batch_device"]
    # ... and of Vis/FeatureType 0
    sig["sf_get_features_and_descriptor_surf_batch_device"] = sig["sf_get_features_and_descriptor_batch_device"]
    sig["sf_add_keyframes_surf_u8_batch_device"] = sig["sf_add_keyframes_u8_batch_device"]
    # ... and of Vis/FeatureType 1
    sig["sf_get_features_and_descriptor_sift_batch_device"] = sig["sf_get_features_and_descriptor_batch_device"]
    sig["sf_add_keyframes_sift_u8_batch_device"] = sig["sf_add_keyframes_u8_batch_device"]
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here = the library does not export the ABI
        fn.restype = res
        fn.argtypes = args
    if L.sf_abi_version() != _abi.SF_ABI_VERSION:
        raise ImportError("%s reports ABI version %d, this binding is written for %d (include/sepfinder.h): rebuild the "
                          "library" % (LIB_PATH, L.sf_abi_version(), _abi.SF_ABI_VERSION))
    _lib = L
    return L


EXPORTED = [
    "sf_abi_version", "sf_default_params", "sf_create", "sf_destroy", "sf_last_error", "sf_get_params",
    "sf_set_stream", "sf_synchronize", "sf_nn_append_local", "sf_nn_append_received",
    "sf_nn_append_local_f32_device", "sf_nn_append_received_f32_device", "sf_nn_append_local_f16_device",
    "sf_nn_append_received_f16_device", "sf_nn_sizes",
    "sf_nn_mark_local_used", "sf_nn_mark_other_used", "sf_nn_ignore_pair", "sf_nn_reset",
    "sf_nn_set_precision",
    "sf_set_option",
    "sf_nn_find_matches", "sf_nn_last_row_minima", "sf_nn_last_filter_dims", "sf_nn_walk", "sf_store_add_keyframe",
    "sf_store_add_keyframes_device", "sf_store_size", "sf_store_clear",
    "sf_camera_add", "sf_camera_get", "sf_camera_count", "sf_camera_select", "sf_store_set_camera", "sf_store_get_camera",
    "sf_brief_set_pattern", "sf_brief_get_pattern", "sf_extract_keyframe_device", "sf_detect_corners_device", "sf_stereo_flow_defaults", "sf_stereo_correspondences_device", "sf_detector_defaults", "sf_get_features_and_descriptor", "sf_netvlad_load", "sf_netvlad_infer_device", "sf_netvlad_infer_batch_device", "sf_estimate_transform",
    "sf_estimate_transform_batch", "sf_verify_pairs", "sf_verify_pairs_device", "sf_verify_matches_device", "sf_find_matches_and_verify_device", "sf_compact_accepted_device",
    "sf_compact_accepted_device_async", "sf_step_issue", "sf_step_retire", "sf_memcpy_device_async", "sf_step_mirror", "sf_step_mirror_pair", "sf_step_mirror_streams", "sf_accept_stream_set", "sf_accept_stream_select", "sf_accept_stream_status", "sf_last_match_results", "sf_compact_accepted_indexed_device_async", "sf_compact_accepted_indexed_mirrored_device_async",
    "sf_debug_correspondences", "sf_debug_pass_state", "sf_debug_counters", "sf_debug_guided_points", "sf_debug_plan_workspace", "sf_debug_live_resources", "sf_pack_separators", "sf_comm_unique_id", "sf_comm_init", "sf_comm_destroy",
    "sf_allgather_separators", "sf_allgather_separators_device", "sf_allgather_bytes_device", "sf_nn_row_minima_device", "sf_nn_walk_device",
    "sf_get_features_and_descriptor_batch_device", "sf_prof_enable", "sf_prof_select", "sf_prof_reset", "sf_prof_get",
    "sf_kernel_name", "sf_stream_placement", "sf_streams_prepare",
    "sf_orb_defaults", "sf_set_feature_type", "sf_get_feature_type", "sf_orb_set_pattern", "sf_orb_get_pattern",
    "sf_fast_defaults", "sf_fast_set_params", "sf_fast_get_params", "sf_detect_fast_device",
    "sf_gftt_defaults", "sf_gftt_set_params", "sf_gftt_get_params", "sf_gftt_check_params",
    "sf_orb_detector_defaults", "sf_set_feature_type_orb", "sf_get_orb_detector", "sf_detect_orb_device",
    "sf_image_set_gray_rule", "sf_image_get_gray_rule", "sf_image_to_gray_device", "sf_netvlad_infer_u8_batch_device",
    "sf_get_features_and_descriptor_u8", "sf_add_keyframes_u8_batch_device",
    "sf_get_features_and_descriptor_orb_batch_device", "sf_add_keyframes_orb_u8_batch_device",
    "sf_front_defaults", "sf_front_set_params", "sf_front_get_params", "sf_compute_roi", "sf_corner_subpix_device",
    "sf_stereo_defaults", "sf_stereo_set_params", "sf_stereo_get_params", "sf_stereo_block_match_device",
    "sf_grid_defaults", "sf_grid_set_params", "sf_grid_get_params", "sf_compute_grid",
    "sf_freak_defaults", "sf_set_feature_type_freak", "sf_get_freak_params", "sf_freak_set_pairs", "sf_freak_get_pairs",
    "sf_freak_build_pattern", "sf_freak_default_pairs",
    "sf_surf_defaults", "sf_set_feature_type_surf", "sf_get_surf_params", "sf_detect_surf_device", "sf_surf_build_tables",
    "sf_surf_check_params",
    "sf_get_features_and_descriptor_surf_batch_device", "sf_add_keyframes_surf_u8_batch_device", "sf_surf_batch_status",
    "sf_debug_surf_limits", "sf_surf_batch_plan",
    "sf_sift_defaults", "sf_set_feature_type_sift", "sf_get_sift_params", "sf_detect_sift_device", "sf_sift_check_params", "sf_sift_build_tables", "sf_sift_plan",
    "sf_debug_sift_limits", "sf_debug_sift_plane",
    "sf_get_features_and_descriptor_sift_batch_device", "sf_add_keyframes_sift_u8_batch_device", "sf_sift_batch_status",
    "sf_debug_sift_batch_chunk", "sf_sift_batch_plan",
    "sf_debug_knn2_u8",
    "sf_depth_defaults", "sf_depth_set_params", "sf_depth_get_params", "sf_depth_mask_device", "sf_depth_points_device",
    "sf_detect_corners_masked_device", "sf_detect_fast_masked_device", "sf_extract_keyframe_depth_device",
    "sf_get_features_and_descriptor_depth", "sf_get_features_and_descriptor_depth_batch_device",
    "sf_add_keyframes_depth_batch_device",
    "sf_depth_set_size", "sf_depth_get_size", "sf_depth_interpolation_factor", "sf_depth_interpolate_device",
    "sf_store_export_plan", "sf_store_export_keyframes_device", "sf_store_import_keyframes_device", "sf_store_wire_status",
    "sf_rectify_check_info", "sf_rectify_plan_create", "sf_rectify_plan_from_maps", "sf_rectify_plan_count",
    "sf_rectify_plan_get", "sf_rectify_plan_clear", "sf_rectify_maps_device", "sf_image_rectify_device",
    "sf_stereo_camera_from_info",
    "sf_depth_registration_defaults", "sf_depth_register_check", "sf_depth_register_device", "sf_depth_fill_holes_device",
    "sf_debug_depth_register_limits",
]


def rectify_check_info(info):
    """sf_rectify_check_info (no GPU, no handle): (status, iR) -- SF_OK and the plan's (P[:, :3] R)^-1 as float64 [3, 3], or
    SF_EINVAL and None for a block sf_rectify_plan_create refuses."""
    iR = np.zeros(9, np.float64)
    rc = load().sf_rectify_check_info(C.byref(info), C.c_void_p(iR.ctypes.data))
    return rc, (iR.reshape(3, 3) if rc == _abi.SF_OK else None)


def stereo_camera_from_info(left, right, local_transform=None):
    """sf_stereo_camera_from_info (no GPU, no handle): the _abi.StereoCamera of the rectified pair of two _abi.CameraInfo
    blocks; SepfinderError where the baseline -P_right[3] / P_right[0] is not positive."""
    cam = _abi.StereoCamera()
    lt = None if local_transform is None else np.ascontiguousarray(local_transform, np.float32).reshape(12)
    rc = load().sf_stereo_camera_from_info(C.byref(left), C.byref(right), None if lt is None else C.c_void_p(lt.ctypes.data),
                                           C.byref(cam))
    if rc != _abi.SF_OK:
        raise SepfinderError(rc, (load().sf_last_error(None) or b"").decode())
    return cam


depth_registration = _abi.depth_registration   # the block sf_depth_register_device takes (see _abi.depth_registration)


def depth_register_check(reg):
    """sf_depth_register_check (no GPU, no handle): (status, text) -- SF_OK and "", or SF_EINVAL and the reason for a block
    sf_depth_register_device refuses."""
    L = load()
    rc = L.sf_depth_register_check(C.byref(reg))
    return rc, ("" if rc == _abi.SF_OK else (L.sf_last_error(None) or b"").decode())


def depth_interpolation_factor(width, height, depth_width, depth_height):
    """sf_depth_interpolation_factor (no GPU, no handle): the integer factor by which a depth image of depth_width x
    depth_height divides a width x height image in both dimensions alike; 0: none, the depth keyframe calls make no mask."""
    return load().sf_depth_interpolation_factor(width, height, depth_width, depth_height)


def freak_build_pattern(params=None):
    """sf_freak_build_pattern (no GPU, no handle): the table FREAK samples with, float32 [64, 256, 43, 3] = (x, y, sigma)
    per scale, orientation and receptive field, and the int32 [64] border every scale asks for."""
    table = np.zeros((_abi.FREAK_SCALES, _abi.FREAK_ORIENTATIONS, _abi.FREAK_POINTS, 3), np.float32)
    sizes = np.zeros(_abi.FREAK_SCALES, np.int32)
    rc = load().sf_freak_build_pattern(C.byref(params) if params is not None else None, C.c_void_p(table.ctypes.data),
                                       C.c_void_p(sizes.ctypes.data))
    if rc != _abi.SF_OK:
        raise SepfinderError(rc, "FREAK parameters out of range")
    return table, sizes


def freak_default_pairs():
    """sf_freak_default_pairs (no GPU, no handle): the generated selection of a fresh handle, int32 [512] indices into
    the 903 pairs (i, j < i) -- NOT OpenCV's FREAK_DEF_PAIRS."""
    sel = np.zeros(_abi.FREAK_PAIRS, np.int32)
    load().sf_freak_default_pairs(C.c_void_p(sel.ctypes.data))
    return sel


def surf_build_tables():
    """sf_surf_build_tables (no GPU, no handle): the orientation samples' offsets int8 [109, 2] = (x, y) and weights float32
    [109], and the float32 [400] weights of the 20 x 20 descriptor gradients."""
    ori_w = np.zeros(_abi.SURF_ORI_SAMPLES, np.float32)
    ori_xy = np.zeros((_abi.SURF_ORI_SAMPLES, 2), np.int8)
    desc_w = np.zeros(_abi.SURF_PATCH * _abi.SURF_PATCH, np.float32)
    load().sf_surf_build_tables(C.c_void_p(ori_w.ctypes.data), C.c_void_p(ori_xy.ctypes.data), C.c_void_p(desc_w.ctypes.data))
    return ori_xy, ori_w, desc_w


def surf_batch_plan(width, height, n_keyframes, surf=None):
    """sf_surf_batch_plan (no GPU, no handle): (key capacity per image, images per chunk, workspace bytes) of the SURF batch
    forms on n_keyframes images of width x height (surf: _abi.SurfParams; None = the defaults)."""
    cap, chunk, ws = C.c_int32(), C.c_int32(), C.c_int64()
    rc = load().sf_surf_batch_plan(width, height, C.byref(surf) if surf is not None else None, n_keyframes, C.byref(cap),
                                   C.byref(chunk), C.byref(ws))
    if rc != _abi.SF_OK:
        raise SepfinderError(rc, "sf_surf_batch_plan refuses %d x %d, %d keyframes" % (width, height, n_keyframes))
    return cap.value, chunk.value, ws.value


def sift_build_tables(sift=None):
    """sf_sift_build_tables (no GPU, no handle): (sigmas float64 [n + 3], lengths int32 [n + 3], coefficients float32
    [n + 3, 520]) of the SIFT detector's blurs under sift (_abi.SiftParams; None = the defaults)."""
    n = (sift.n_octave_layers if sift is not None else 3) + 3
    rows = max(min(n, _abi.SIFT_MAX_LAYERS + 3), 4)
    sig, klen = np.zeros(rows, np.float64), np.zeros(rows, np.int32)
    coef = np.zeros((rows, _abi.SIFT_MAX_KLEN), np.float32)
    rc = load().sf_sift_build_tables(C.byref(sift) if sift is not None else None, C.c_void_p(sig.ctypes.data),
                                     C.c_void_p(klen.ctypes.data), C.c_void_p(coef.ctypes.data))
    if rc != _abi.SF_OK:
        raise SepfinderError(rc, "SIFT parameters out of range")
    return sig[:n], klen[:n], coef[:n]


def sift_plan(width, height, sift=None):
    """sf_sift_plan (no GPU, no handle): (octaves, [(w, h)] per octave, Gaussian samples, difference samples)."""
    n, g, d = C.c_int32(), C.c_int64(), C.c_int64()
    w, h = np.zeros(_abi.SIFT_MAX_OCTAVES, np.int32), np.zeros(_abi.SIFT_MAX_OCTAVES, np.int32)
    rc = load().sf_sift_plan(width, height, C.byref(sift) if sift is not None else None, C.byref(n), C.c_void_p(w.ctypes.data),
                             C.c_void_p(h.ctypes.data), C.byref(g), C.byref(d))
    if rc != _abi.SF_OK:
        raise SepfinderError(rc, "sf_sift_plan refuses %d x %d" % (width, height))
    return n.value, [(int(w[o]), int(h[o])) for o in range(n.value)], g.value, d.value


def sift_batch_plan(width, height, n_keyframes, sift=None):
    """sf_sift_batch_plan (no GPU, no handle): (extrema / keypoint capacity per image, images per chunk, workspace bytes) of
    the SIFT batch forms on n_keyframes images of width x height (sift: _abi.SiftParams; None = the defaults)."""
    cap, chunk, ws = C.c_int32(), C.c_int32(), C.c_int64()
    rc = load().sf_sift_batch_plan(width, height, C.byref(sift) if sift is not None else None, n_keyframes, C.byref(cap),
                                   C.byref(chunk), C.byref(ws))
    if rc != _abi.SF_OK:
        raise SepfinderError(rc, "sf_sift_batch_plan refuses %d x %d, %d keyframes" % (width, height, n_keyframes))
    return cap.value, chunk.value, ws.value


def debug_live_resources():
    """sf_debug_live_resources (include/sf_experimental.h): what the process's handles hold right now, as a dict keyed by
    _abi.LIVE_RESOURCES -- device blocks, their bytes, pinned host blocks, events.  No handle, no GPU."""
    out = (C.c_int64 * 4)()
    load().sf_debug_live_resources(out)
    return dict(zip(_abi.LIVE_RESOURCES, (int(v) for v in out)))


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def upload(array, device=0):
    """A host array as a torch tensor on the GPU (the small upload helper of the calls that take device images: torch is
    the plumbing here, and the tensor keeps the memory alive)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to(torch.device("cuda:%d" % device))


def _camera_image(image, fmt):
    """A uint8 image as the camera calls take it: [h, w, 3] for rgb8 / bgr8, [h, w] (or [h, w, 1]) for mono8, bytes of a
    pixel and pixels of a row contiguous, any row stride.  Returns (array, width, height, pitch)."""
    a = np.asarray(image)
    if a.dtype != np.uint8:
        raise ValueError("camera images are uint8, not %s" % a.dtype)
    if fmt == _abi.SF_IMAGE_MONO8 and a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    ch = 1 if fmt == _abi.SF_IMAGE_MONO8 else 3
    ok = (a.ndim == 2 and a.strides[1] == 1) if ch == 1 else (a.ndim == 3 and a.shape[2] == 3 and a.strides[2] == 1
                                                              and a.strides[1] == 3)
    if not ok or a.strides[0] < a.shape[1] * ch:
        a = np.ascontiguousarray(a)
        if a.ndim != (2 if ch == 1 else 3) or (ch == 3 and a.shape[2] != 3):
            raise ValueError("image of shape %s does not fit format %d" % (a.shape, fmt))
    return a, a.shape[1], a.shape[0], a.strides[0]


class SeparatorFinder:
    """One handle = one robot's separator-finder state on one GPU (single caller, like the
    reference's single-threaded geometry node)."""

    def __init__(self, params=None, device=0):
        self._L = load()
        self.params = _abi.copy_params(params) if params is not None else _abi.default_params()
        h = C.c_void_p()
        rc = self._L.sf_create(C.byref(self.params), device, C.byref(h))
        if rc != 0:
            raise SepfinderError(rc, (self._L.sf_last_error(None) or b"").decode())
        self._h = h
        self.device = device

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise SepfinderError(rc, (self._L.sf_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.sf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, hip_stream_ptr):
        self._check(self._L.sf_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def synchronize(self):
        self._check(self._L.sf_synchronize(self._h))

    # -- NN stage (data_handler.py:166-209) ---------------------------------------------------
    def nn_append_local(self, desc):
        d = np.ascontiguousarray(desc, dtype=np.float64)
        d = d.reshape(-1, d.shape[-1]) if d.ndim > 1 else d.reshape(-1, self.params.netvlad_dimensions)
        self._check(self._L.sf_nn_append_local(self._h, _ptr(d), d.shape[0], d.shape[1]))

    def nn_append_received(self, desc):
        d = np.ascontiguousarray(desc, dtype=np.float64)
        d = d.reshape(-1, d.shape[-1]) if d.ndim > 1 else d.reshape(-1, self.params.netvlad_dimensions)
        self._check(self._L.sf_nn_append_received(self._h, _ptr(d), d.shape[0], d.shape[1]))

    def nn_append_local_device(self, dptr, n, dim):
        self._check(self._L.sf_nn_append_local_f32_device(self._h, C.c_void_p(dptr), n, dim))

    def nn_append_received_device(self, dptr, n, dim):
        self._check(self._L.sf_nn_append_received_f32_device(self._h, C.c_void_p(dptr), n, dim))

    def nn_append_local_f16_device(self, dptr, n, dim):
        """n x dim IEEE binary16 descriptors in device memory (converted exactly to the fp32 database rows)."""
        self._check(self._L.sf_nn_append_local_f16_device(self._h, C.c_void_p(dptr), n, dim))

    def nn_append_received_f16_device(self, dptr, n, dim):
        self._check(self._L.sf_nn_append_received_f16_device(self._h, C.c_void_p(dptr), n, dim))

    def nn_sizes(self):
        a, b = C.c_int32(), C.c_int32()
        self._check(self._L.sf_nn_sizes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def nn_mark_local_used(self, idx):
        self._check(self._L.sf_nn_mark_local_used(self._h, int(idx)))

    def nn_mark_other_used(self, idx):
        self._check(self._L.sf_nn_mark_other_used(self._h, int(idx)))

    def nn_ignore_pair(self, idx_local, idx_other):
        self._check(self._L.sf_nn_ignore_pair(self._h, int(idx_local), int(idx_other)))

    def nn_reset(self):
        self._check(self._L.sf_nn_reset(self._h))

    def nn_set_precision(self, nn_precision):
        self._check(self._L.sf_nn_set_precision(self._h, int(nn_precision)))
        self.params.nn_precision = int(nn_precision)

    def set_option(self, option, value):
        """Execution options of a live handle (_abi.SF_OPT_*); none changes any output byte."""
        self._check(self._L.sf_set_option(self._h, int(option), int(value)))

    def nn_find_matches(self, cap=None):
        n_l, _ = self.nn_sizes()
        if cap is None:
            cap = max(1, min(max(n_l, 1), self.params.netvlad_max_matches_nb))
        out = np.zeros(max(cap, 1), dtype=_abi.MATCH_DTYPE)
        n = C.c_int32()
        self._check(self._L.sf_nn_find_matches(self._h, out.ctypes.data, cap, C.byref(n)))
        return out[: n.value]

    def nn_walk(self, row_min, row_arg, n_received, cap=None):
        """data_handler.py:191-205 on caller-provided per-row minima (host work; row-sharded NN of a multi-GPU node)."""
        d = np.ascontiguousarray(row_min, dtype=np.float64)
        a = np.ascontiguousarray(row_arg, dtype=np.int32)
        if cap is None:
            cap = max(1, min(max(d.size, 1), self.params.netvlad_max_matches_nb))
        out = np.zeros(max(cap, 1), dtype=_abi.MATCH_DTYPE)
        n = C.c_int32()
        self._check(self._L.sf_nn_walk(self._h, _ptr(d), _ptr(a), d.size, int(n_received), out.ctypes.data, cap,
                                       C.byref(n)))
        return out[: n.value]

    def nn_walk_device(self, d_row_min, d_row_arg, d_status, n_local, n_received, d_matches, cap, d_n_matches):
        """data_handler.py:191-205 on the device, on device-resident minima (raw pointers); asynchronous on the
        handle's stream.  d_matches: MATCH_DTYPE[cap], d_n_matches: int32[1] (device or pinned host memory)."""
        self._check(self._L.sf_nn_walk_device(self._h, C.c_void_p(d_row_min), C.c_void_p(d_row_arg),
                                              C.c_void_p(d_status) if d_status else None, int(n_local), int(n_received),
                                              C.c_void_p(d_matches), int(cap), C.c_void_p(d_n_matches)))

    def nn_row_minima_device(self, d_row_min, d_row_arg, d_status):
        """The NN kernels of this handle's local rows without the walk; results stay in device memory (raw pointers:
        float64[n_local], int32[n_local], int32[1]); asynchronous on the handle's stream."""
        self._check(self._L.sf_nn_row_minima_device(self._h, C.c_void_p(d_row_min), C.c_void_p(d_row_arg),
                                                    C.c_void_p(d_status)))

    def allgather_bytes_device(self, d_send, d_all, bytes_per_rank):
        self._check(self._L.sf_allgather_bytes_device(self._h, C.c_void_p(d_send), C.c_void_p(d_all), int(bytes_per_rank)))

    def nn_last_filter_dims(self):
        d = C.c_int32()
        self._check(self._L.sf_nn_last_filter_dims(self._h, C.byref(d)))
        return d.value

    def nn_last_row_minima(self):
        n_l, _ = self.nn_sizes()
        d = np.zeros(n_l, dtype=np.float64)
        i = np.zeros(n_l, dtype=np.int32)
        self._check(self._L.sf_nn_last_row_minima(self._h, _ptr(d), _ptr(i), n_l))
        return d, i

    # -- keyframe store ---------------------------------------------------------------------------
    def store_add_keyframe(self, feats):
        f = feats.c_struct()
        slot = C.c_int32()
        self._check(self._L.sf_store_add_keyframe(self._h, C.byref(f), C.byref(slot)))
        return slot.value

    def store_add_keyframes_device(self, n, rows, cols, d_desc, d_xyz, d_kp):
        first = C.c_int32()
        self._check(self._L.sf_store_add_keyframes_device(self._h, n, rows, cols, C.c_void_p(d_desc),
                                                          C.c_void_p(d_xyz), C.c_void_p(d_kp),
                                                          C.byref(first)))
        return first.value

    # -- feature extraction ------------------------------------------------
    def brief_set_pattern(self, tests):
        """tests: int8 [8 * bytes, 4] = (x1, y1, x2, y2) per descriptor bit."""
        t = np.ascontiguousarray(tests, dtype=np.int8).reshape(-1, 4)
        self._check(self._L.sf_brief_set_pattern(self._h, C.c_void_p(t.ctypes.data), t.shape[0] // 8))

    def brief_get_pattern(self):
        n = C.c_int32()
        buf = np.zeros((64 * 8, 4), np.int8)
        self._check(self._L.sf_brief_get_pattern(self._h, C.c_void_p(buf.ctypes.data), 64, C.byref(n)))
        return buf[:8 * n.value].copy()

    def set_feature_type(self, feature_type, orb=None):
        """Vis/FeatureType of the extraction calls: 6 = GFTT/BRIEF (a fresh handle), 8 = GFTT/ORB with orb
        (_abi.OrbParams; None = rtabmap's ORB/ defaults), 4 = FAST/BRIEF: type 6 with the corners of the FAST detector
        (fast_set_params; orb is ignored)."""
        self._check(self._L.sf_set_feature_type(self._h, int(feature_type), C.byref(orb) if orb is not None else None))

    def get_feature_type(self):
        """(feature type, _abi.OrbParams of the ORB extraction)."""
        ft, o = C.c_int32(), _abi.OrbParams()
        self._check(self._L.sf_get_feature_type(self._h, C.byref(ft), C.byref(o)))
        return ft.value, o

    def orb_set_pattern(self, tests):
        """tests: int8 [256, 4] = (x1, y1, x2, y2) per descriptor bit, within +-15."""
        t = np.ascontiguousarray(tests, dtype=np.int8).reshape(-1, 4)
        self._check(self._L.sf_orb_set_pattern(self._h, C.c_void_p(t.ctypes.data), t.shape[0] // 8))

    def orb_get_pattern(self):
        n = C.c_int32()
        buf = np.zeros((32 * 8, 4), np.int8)
        self._check(self._L.sf_orb_get_pattern(self._h, C.c_void_p(buf.ctypes.data), 32, C.byref(n)))
        return buf[:8 * n.value].copy()

    def set_feature_type_freak(self, feature_type, freak=None):
        """Vis/FeatureType 3 (FAST/FREAK: the corners of fast_set_params) or 5 (GFTT/FREAK) with freak (_abi.FreakParams;
        None = rtabmap's FREAK/ defaults): 64-byte rows.  set_feature_type(4 | 6 | 8) and set_feature_type_orb switch
        back."""
        self._check(self._L.sf_set_feature_type_freak(self._h, int(feature_type), C.byref(freak) if freak is not None else None))

    def get_freak_params(self):
        f = _abi.FreakParams()
        self._check(self._L.sf_get_freak_params(self._h, C.byref(f)))
        return f

    def freak_set_pairs(self, selected):
        """selected: 512 indices into the 903 pairs `for i in 1..42: for j in 0..i-1` -- OpenCV's selectedPairs format
        (FREAK_DEF_PAIRS pastes in unchanged)."""
        t = np.ascontiguousarray(selected, dtype=np.int32).reshape(-1)
        self._check(self._L.sf_freak_set_pairs(self._h, C.c_void_p(t.ctypes.data), t.size))

    def freak_get_pairs(self):
        n = C.c_int32()
        buf = np.zeros(_abi.FREAK_PAIRS, np.int32)
        self._check(self._L.sf_freak_get_pairs(self._h, C.c_void_p(buf.ctypes.data), buf.size, C.byref(n)))
        return buf[:n.value].copy()

    def set_feature_type_surf(self, surf=None):
        """Vis/FeatureType 0 (SURF) with surf (_abi.SurfParams; None = rtabmap's SURF/ defaults) on a handle created with
        desc_type 1 and desc_bytes 256 (512 with extended = 1): float32 rows of 64 (128) dimensions."""
        self._check(self._L.sf_set_feature_type_surf(self._h, C.byref(surf) if surf is not None else None))

    def get_surf_params(self):
        p = _abi.SurfParams()
        self._check(self._L.sf_get_surf_params(self._h, C.byref(p)))
        return p

    def detect_surf(self, d_image, width, height, pitch, max_features, d_kpts_out, cap, surf=None):
        """The fast-Hessian detector of SURF + rtabmap's limitKeypoints on the device (surf None = the handle's; any
        handle); returns the number of keypoints of the result (<= cap are written)."""
        n = C.c_int32()
        self._check(self._L.sf_detect_surf_device(self._h, C.c_void_p(d_image), width, height, pitch, max_features,
                                                  C.byref(surf) if surf is not None else None, C.c_void_p(d_kpts_out), cap,
                                                  C.byref(n)))
        return n.value

    def set_feature_type_sift(self, sift=None):
        """Vis/FeatureType 1 (SIFT) with sift (_abi.SiftParams; None = rtabmap's SIFT/ defaults) on a handle created with
        desc_type 1 and desc_bytes 512: float32 rows of 128 dimensions -- or with desc_type 2 (desc_bytes 128): the same
        128 integers per row as uint8."""
        self._check(self._L.sf_set_feature_type_sift(self._h, C.byref(sift) if sift is not None else None))

    def get_sift_params(self):
        p = _abi.SiftParams()
        self._check(self._L.sf_get_sift_params(self._h, C.byref(p)))
        return p

    def detect_sift(self, d_image, width, height, pitch, max_features, d_kpts_out, cap, sift=None):
        """The SIFT detector + retainBest / rtabmap's limitKeypoints on the device (sift: _abi.SiftParams, None = the
        handle's; any handle); returns the number of keypoints of the result (<= cap are written)."""
        n = C.c_int32()
        self._check(self._L.sf_detect_sift_device(self._h, C.c_void_p(d_image), width, height, pitch, max_features,
                                                  C.byref(sift) if sift is not None else None, C.c_void_p(d_kpts_out), cap,
                                                  C.byref(n)))
        return n.value

    def debug_sift_limits(self, candidate_cap=0):
        """sf_debug_sift_limits (include/sf_experimental.h): the extrema / keypoint capacity per image; 0 = the default."""
        self._check(self._L.sf_debug_sift_limits(self._h, candidate_cap))

    def debug_sift_plane(self, octave, layer, dog, d_out):
        """sf_debug_sift_plane: one int16 plane of the most recent detect_sift call's pyramid -> d_out (device pointer)."""
        self._check(self._L.sf_debug_sift_plane(self._h, octave, layer, int(bool(dog)), C.c_void_p(d_out)))

    def descriptor_bytes(self):
        """Row bytes the extraction calls write with the handle's feature type."""
        if self.get_feature_type()[0] == _abi.FEATURE_SURF:
            return 512 if self.get_surf_params().extended else 256
        if self.get_feature_type()[0] == _abi.FEATURE_SIFT:
            return _abi.SF_DESC_BYTES_U8 if self.params.desc_type == 2 else 512
        if self.get_feature_type()[0] in (_abi.FEATURE_FAST_FREAK, _abi.FEATURE_GFTT_FREAK):
            return _abi.FREAK_BYTES
        return 32 if self.get_feature_type()[0] in (_abi.FEATURE_GFTT_ORB, _abi.FEATURE_ORB) else self.brief_get_pattern().shape[0] // 8

    # -- NetVLAD inference -------------------------------------------------
    def netvlad_load(self, weights):
        """weights: dict of float32 numpy arrays in TensorFlow layouts -- conv_kernel[13] ([3, 3, Cin, Cout]),
        conv_bias[13], average_rgb [3], assignment [512, K], cluster_centers [512, K], wpca_kernel [512 K, pca_dim],
        wpca_bias [pca_dim]."""
        w = _abi.NetvladWeights()
        keep = []

        def ptr(a):
            a = np.ascontiguousarray(a, dtype=np.float32)
            keep.append(a)
            return a.ctypes.data
        for i in range(13):
            w.conv_kernel[i] = ptr(weights["conv_kernel"][i])
            w.conv_bias[i] = ptr(weights["conv_bias"][i])
        w.average_rgb = ptr(weights["average_rgb"])
        w.assignment = ptr(weights["assignment"])
        w.cluster_centers = ptr(weights["cluster_centers"])
        w.wpca_kernel = ptr(weights["wpca_kernel"])
        w.wpca_bias = ptr(weights["wpca_bias"])
        w.clusters = int(np.asarray(weights["assignment"]).shape[1])
        w.pca_dim = int(np.asarray(weights["wpca_bias"]).shape[0])
        self._check(self._L.sf_netvlad_load(self._h, C.byref(w)))

    def netvlad_infer_device(self, d_image_rgb, width, height, d_out, n_out):
        self._check(self._L.sf_netvlad_infer_device(self._h, C.c_void_p(d_image_rgb), width, height, C.c_void_p(d_out), n_out))

    def netvlad_infer_batch_device(self, d_images_rgb, n_images, width, height, d_out, n_out):
        """n_images images [H][W][3] float32 back to back on the device -> d_out [n_images][n_out] (data_handler.py:149-156)."""
        self._check(self._L.sf_netvlad_infer_batch_device(self._h, C.c_void_p(d_images_rgb), n_images, width, height,
                                                          C.c_void_p(d_out), n_out))

    # -- the camera's own images (rgb8 / bgr8 / mono8: _abi.SF_IMAGE_*) -----------------------------------------------
    def image_set_gray_rule(self, rule):
        """Coefficients of the colour-to-gray conversion: _abi.GRAY_RULE_OPENCV3 (a fresh handle) or GRAY_RULE_OPENCV4."""
        self._check(self._L.sf_image_set_gray_rule(self._h, int(rule)))

    def image_get_gray_rule(self):
        r = C.c_int32()
        self._check(self._L.sf_image_get_gray_rule(self._h, C.byref(r)))
        return r.value

    def image_to_gray_device(self, d_src, fmt, width, height, src_pitch, src_stride, n_images, d_dst, dst_pitch,
                             dst_stride):
        """cv2.cvtColor(..., COLOR_RGB2GRAY) of n_images device images (raw pointers) in one launch; asynchronous."""
        self._check(self._L.sf_image_to_gray_device(self._h, C.c_void_p(d_src), int(fmt), width, height, src_pitch,
                                                    int(src_stride), n_images, C.c_void_p(d_dst), dst_pitch,
                                                    int(dst_stride)))

    def netvlad_infer_u8_batch_device(self, d_images, fmt, n_images, width, height, pitch, image_stride, d_out, n_out):
        """netvlad_infer_batch_device on 8-bit device images (rows of `pitch` bytes, images image_stride bytes apart)."""
        self._check(self._L.sf_netvlad_infer_u8_batch_device(self._h, C.c_void_p(d_images), int(fmt), n_images, width,
                                                             height, pitch, int(image_stride), C.c_void_p(d_out), n_out))

    def netvlad_u8(self, images, fmt=_abi.SF_IMAGE_RGB8, n_out=None):
        """NetVLAD descriptors of host images of one size (a sequence of uint8 arrays in `fmt`): uploads the bytes, runs
        the network on them, returns [n, n_out] float32 (n_out None: params.netvlad_dimensions)."""
        imgs = [np.ascontiguousarray(_camera_image(im, fmt)[0]) for im in images]
        n_out = self.params.netvlad_dimensions if n_out is None else int(n_out)
        if not imgs:
            return np.zeros((0, n_out), np.float32)
        batch = np.stack(imgs)
        h, w = batch.shape[1], batch.shape[2]
        import torch
        d_in = upload(batch, self.device)
        d_out = torch.zeros((len(imgs), n_out), dtype=torch.float32, device=d_in.device)
        torch.cuda.current_stream(d_in.device).synchronize()       # (the handle's stream may be another one)
        self.netvlad_infer_u8_batch_device(d_in.data_ptr(), fmt, len(imgs), w, h, batch.strides[1], batch.strides[0],
                                           d_out.data_ptr(), n_out)
        self.synchronize()
        return d_out.cpu().numpy()

    def get_features_and_descriptor_u8(self, left, right, fmt, cam, det=None, flow=None):
        """get_features_and_descriptor on the camera's images (host uint8, [h, w, 3] for rgb8 / bgr8, [h, w] for mono8):
        uploaded as they are, converted to gray on the device under the handle's gray rule."""
        left, w, h, pitch = _camera_image(left, fmt)
        right, w2, h2, pitch2 = _camera_image(right, fmt)
        if (w, h) != (w2, h2):
            raise ValueError("left / right must be images of one shape")
        if pitch != pitch2:
            left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
            pitch = left.strides[0]
        return self._host_keyframe(
            self._L.sf_get_features_and_descriptor_u8,
            (C.c_void_p(left.ctypes.data), C.c_void_p(right.ctypes.data), int(fmt), w, h, pitch), w, h, cam, det,
            C.byref(flow) if flow is not None else None)

    def add_keyframes_u8_batch_device(self, d_left, d_right, d_rgb, fmt, n_keyframes, width, height, pitch, image_stride,
                                      cam, det=None, flow=None, d_rows_out=None, d_desc_out=None, d_xyz_out=None,
                                      d_kpts_out=None, _call="sf_add_keyframes_u8_batch_device"):
        """n keyframes from the camera's device images (raw pointers; d_rgb None = the left images) to n store slots and n
        local NN rows in one launch sequence, no host wait.  Returns (first slot, first local NN row)."""
        first, row = C.c_int32(-1), C.c_int32(-1)
        self._check(getattr(self._L, _call)(
            self._h, C.c_void_p(d_left), C.c_void_p(d_right), C.c_void_p(d_rgb), int(fmt), n_keyframes, width, height,
            pitch, int(image_stride), C.byref(cam), C.byref(det) if det is not None else None,
            C.byref(flow) if flow is not None else None, C.byref(first), C.byref(row), C.c_void_p(d_rows_out),
            C.c_void_p(d_desc_out), C.c_void_p(d_xyz_out), C.c_void_p(d_kpts_out)))
        return first.value, row.value

    def add_keyframes_orb_u8_batch_device(self, *args, **kw):
        """add_keyframes_u8_batch_device on a handle of Vis/FeatureType 2 (set_feature_type_orb): same arguments, same
        return value; slot i holds what get_features_and_descriptor_u8 gives for pair i."""
        return self.add_keyframes_u8_batch_device(*args, _call="sf_add_keyframes_orb_u8_batch_device", **kw)

    def add_keyframes_surf_u8_batch_device(self, *args, **kw):
        """add_keyframes_u8_batch_device on a handle of Vis/FeatureType 0 (set_feature_type_surf): same arguments, same
        return value; slot i holds what get_features_and_descriptor_u8 gives for pair i (surf_batch_status: overflow)."""
        return self.add_keyframes_u8_batch_device(*args, _call="sf_add_keyframes_surf_u8_batch_device", **kw)

    def add_keyframes_sift_u8_batch_device(self, *args, **kw):
        """add_keyframes_u8_batch_device on a handle of Vis/FeatureType 1 (set_feature_type_sift): same arguments, same
        return value; slot i holds what get_features_and_descriptor_u8 gives for pair i (sift_batch_status: overflow)."""
        return self.add_keyframes_u8_batch_device(*args, _call="sf_add_keyframes_sift_u8_batch_device", **kw)

    def set_feature_type_orb(self, det=None, orb=None):
        """Vis/FeatureType 2, ORB on a pyramid: det (_abi.OrbDetectorParams; None = rtabmap's ORB/ defaults) drives the
        detector, orb (_abi.OrbParams; None = defaults, edge_threshold 16 .. 64) the border and the descriptors."""
        self._check(self._L.sf_set_feature_type_orb(self._h, C.byref(det) if det is not None else None,
                                                    C.byref(orb) if orb is not None else None))

    def get_orb_detector(self):
        p = _abi.OrbDetectorParams()
        self._check(self._L.sf_get_orb_detector(self._h, C.byref(p)))
        return p

    def detect_orb_device(self, d_image, width, height, pitch, max_features, d_kpts_out, cap, det=None, orb=None):
        """cv::ORB::detect + rtabmap's limitKeypoints on the device (det / orb None = the handle's); returns the number
        of keypoints of the result (<= cap are written)."""
        n = C.c_int32()
        self._check(self._L.sf_detect_orb_device(self._h, C.c_void_p(d_image), width, height, pitch, max_features,
                                                 C.byref(det) if det is not None else None,
                                                 C.byref(orb) if orb is not None else None,
                                                 C.c_void_p(d_kpts_out), cap, C.byref(n)))
        return n.value

    def fast_set_params(self, params):
        """The handle's FAST parameters (_abi.FastParams): what feature type 4 detects with."""
        self._check(self._L.sf_fast_set_params(self._h, C.byref(params)))

    def fast_get_params(self):
        p = _abi.FastParams()
        self._check(self._L.sf_fast_get_params(self._h, C.byref(p)))
        return p

    def detect_fast_device(self, d_image, width, height, pitch, max_features, d_kpts_out, cap, params=None):
        """FAST-9/16 + rtabmap's limitKeypoints on the device (params None = the handle's); returns the number of
        keypoints of the result (<= cap are written)."""
        n = C.c_int32()
        self._check(self._L.sf_detect_fast_device(self._h, C.c_void_p(d_image), width, height, pitch, max_features,
                                                  C.byref(params) if params is not None else None,
                                                  C.c_void_p(d_kpts_out), cap, C.byref(n)))
        return n.value

    def gftt_set_params(self, params):
        """The handle's GFTT response parameters (_abi.GfttParams: block size, Harris or minimum eigenvalue, k): what
        detect_corners_device and the extraction calls under feature types 5, 6 and 8 detect with; (3, 0, 0.04) on a
        fresh handle."""
        self._check(self._L.sf_gftt_set_params(self._h, C.byref(params)))

    def gftt_get_params(self):
        p = _abi.GfttParams()
        self._check(self._L.sf_gftt_get_params(self._h, C.byref(p)))
        return p

    def front_set_params(self, params):
        """The handle's _abi.FrontParams: the ROI every detector sees (Vis/RoiRatios) and cv::cornerSubPix on the kept
        corners (Vis/SubPix*), applied by the keyframe extraction calls; both off on a fresh handle."""
        self._check(self._L.sf_front_set_params(self._h, C.byref(params)))

    def front_get_params(self):
        p = _abi.FrontParams()
        self._check(self._L.sf_front_get_params(self._h, C.byref(p)))
        return p

    def compute_roi(self, width, height, ratios):
        """sf_compute_roi (pure host code): (x, y, w, h); what _abi.compute_roi restates."""
        r = (C.c_float * 4)(*ratios)
        out = (C.c_int32 * 4)()
        rc = self._L.sf_compute_roi(width, height, r, out)
        if rc != _abi.SF_OK:
            raise SepfinderError(rc, "Vis/RoiRatios %s on a %d x %d image" % (list(ratios), width, height))
        return tuple(out)

    def grid_set_params(self, params):
        """The handle's _abi.GridParams: Vis/GridRows x Vis/GridCols, the detector per cell of the ROI in the keyframe
        extraction calls (feature types 4, 6, 8); 1 x 1 on a fresh handle.  Under a grid the batch calls' per-keyframe
        outputs and the store's rows are rows_cap of compute_grid apart, not max_features."""
        self._check(self._L.sf_grid_set_params(self._h, C.byref(params)))

    def grid_get_params(self):
        p = _abi.GridParams()
        self._check(self._L.sf_grid_get_params(self._h, C.byref(p)))
        return p

    def compute_grid(self, width, height, roi_ratios, grid_rows, grid_cols, max_features):
        """sf_compute_grid (pure host code): (x, y, col_size, row_size, quota, rows_cap); what _abi.compute_grid restates."""
        r = (C.c_float * 4)(*roi_ratios)
        g = _abi.grid_params(grid_rows, grid_cols)
        out = (C.c_int32 * 6)()
        rc = self._L.sf_compute_grid(width, height, r, C.byref(g), max_features, out)
        if rc != _abi.SF_OK:
            raise SepfinderError(rc, "a grid of %d x %d with %d features, Vis/RoiRatios %s, on a %d x %d image"
                                 % (grid_rows, grid_cols, max_features, list(roi_ratios), width, height))
        return tuple(out)

    def corner_subpix_device(self, d_image, width, height, pitch, d_kpts, n, win, iterations, eps):
        """cv::cornerSubPix on n 28-byte keypoint records of a device image, in place (x and y only), asynchronous on the
        handle's stream; device pointers (ints)."""
        self._check(self._L.sf_corner_subpix_device(self._h, C.c_void_p(d_image), width, height, pitch, C.c_void_p(d_kpts),
                                                    n, win, iterations, eps))

    def detect_corners_device(self, d_image, width, height, pitch, max_corners, quality_level, min_distance,
                              d_kpts_out, cap):
        """cv::goodFeaturesToTrack on the device; returns the number of corners found (<= cap are written)."""
        n = C.c_int32()
        self._check(self._L.sf_detect_corners_device(self._h, C.c_void_p(d_image), width, height, pitch, max_corners,
                                                     float(quality_level), float(min_distance), C.c_void_p(d_kpts_out),
                                                     cap, C.byref(n)))
        return n.value

    def stereo_correspondences_device(self, d_left, d_right, width, height, pitch, d_kpts, n, d_right_xy, d_status,
                                      d_right_x=None, d_err=None, params=None):
        """cv::calcOpticalFlowPyrLK + rtabmap's disparity gate on the device (asynchronous); device pointers (ints)."""
        self._check(self._L.sf_stereo_correspondences_device(
            self._h, C.c_void_p(d_left), C.c_void_p(d_right), width, height, pitch, C.c_void_p(d_kpts), n,
            C.byref(params) if params is not None else None, C.c_void_p(d_right_xy), C.c_void_p(d_status),
            C.c_void_p(d_right_x), C.c_void_p(d_err)))

    def stereo_set_params(self, params):
        """The handle's _abi.StereoParams: which stereo correspondence the keyframe extraction calls run (Stereo/OpticalFlow:
        pyramidal LK or block matching) and block matching's score (Stereo/SSD); LK on a fresh handle."""
        self._check(self._L.sf_stereo_set_params(self._h, C.byref(params)))

    def stereo_get_params(self):
        p = _abi.StereoParams()
        self._check(self._L.sf_stereo_get_params(self._h, C.byref(p)))
        return p

    def stereo_block_match_device(self, d_left, d_right, width, height, pitch, d_kpts, n, d_right_xy, d_status,
                                  d_right_x=None, d_score=None, params=None, ssd=1):
        """rtabmap's block-matching stereo correspondence (Stereo/OpticalFlow false) on the device (asynchronous); device
        pointers (ints)."""
        self._check(self._L.sf_stereo_block_match_device(
            self._h, C.c_void_p(d_left), C.c_void_p(d_right), width, height, pitch, C.c_void_p(d_kpts), n,
            C.byref(params) if params is not None else None, ssd, C.c_void_p(d_right_xy), C.c_void_p(d_status),
            C.c_void_p(d_right_x), C.c_void_p(d_score)))

    def _rows_cap(self, width, height, max_features):
        """The rows a keyframe of the single extraction calls can hold: max_features, or under a grid its R C quota
        (compute_grid), which can be more.  What the call itself refuses is left to the call."""
        g = self.grid_get_params()
        if (g.grid_rows, g.grid_cols) == (1, 1):
            return max_features
        try:
            return max(max_features, _abi.compute_grid(width, height, list(self.front_get_params().roi_ratios), g.grid_rows,
                                                       g.grid_cols, max_features)[5])
        except (ValueError, OverflowError):
            return max_features

    def _host_keyframe(self, fn, images, w, h, cam, det, *flow):
        """The three host keyframe calls behind their images: the outputs for the rows a keyframe can hold, the call
        fn(handle, *images, cam, det, *flow, outputs...), the rows it kept."""
        cap = self._rows_cap(w, h, det.max_features if det is not None else 1000)
        desc = np.zeros((cap, self.descriptor_bytes()), np.uint8)
        xyz = np.zeros((cap, 3), np.float32)
        kp = np.zeros(cap, _abi.KEYPOINT_DTYPE)
        rows, slot = C.c_int32(), C.c_int32()
        self._check(fn(self._h, *images, C.byref(cam), C.byref(det) if det is not None else None, *flow,
                       C.c_void_p(desc.ctypes.data), C.c_void_p(xyz.ctypes.data), C.c_void_p(kp.ctypes.data), cap,
                       C.byref(rows), C.byref(slot)))
        n = min(rows.value, cap)
        return desc[:n].copy(), xyz[:n].copy(), kp[:n].copy(), slot.value

    def get_features_and_descriptor(self, left, right, cam, det=None, flow=None):
        """GetFeatsAndDesc on host images (uint8 [h, w], same row stride): returns (descriptors [rows, bytes] uint8,
        kpts3D [rows, 3] float32, kpts [rows] KEYPOINT_DTYPE, slot of the keyframe in the device-resident store)."""
        left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
        if left.ndim != 2 or left.shape != right.shape or left.strides != right.strides or left.strides[1] != 1:
            raise ValueError("left / right must be 2-D uint8 images of one shape and row stride")
        h, w = left.shape
        return self._host_keyframe(
            self._L.sf_get_features_and_descriptor,
            (C.c_void_p(left.ctypes.data), C.c_void_p(right.ctypes.data), w, h, left.strides[0]), w, h, cam, det,
            C.byref(flow) if flow is not None else None)

    def get_features_and_descriptor_batch_device(self, d_left, d_right, n_keyframes, width, height, pitch, image_stride,
                                                 cam, det=None, flow=None, d_rows_out=None, d_desc_out=None,
                                                 d_xyz_out=None, d_kpts_out=None,
                                                 _call="sf_get_features_and_descriptor_batch_device"):
        """n keyframes from device images (raw pointers) to n store slots in one launch sequence, no host wait; optional
        device outputs sized for n_keyframes x max_features rows -- under a grid (grid_set_params) n_keyframes x rows_cap of
        compute_grid, the stride of the keyframes' blocks.  Returns the first slot."""
        first = C.c_int32()
        self._check(getattr(self._L, _call)(
            self._h, C.c_void_p(d_left), C.c_void_p(d_right), n_keyframes, width, height, pitch, int(image_stride),
            C.byref(cam), C.byref(det) if det is not None else None, C.byref(flow) if flow is not None else None,
            C.byref(first), C.c_void_p(d_rows_out), C.c_void_p(d_desc_out), C.c_void_p(d_xyz_out), C.c_void_p(d_kpts_out)))
        return first.value

    def get_features_and_descriptor_orb_batch_device(self, *args, **kw):
        """get_features_and_descriptor_batch_device on a handle of Vis/FeatureType 2 (set_feature_type_orb): same arguments,
        same return value; per keyframe the bytes of get_features_and_descriptor under type 2."""
        return self.get_features_and_descriptor_batch_device(*args, _call="sf_get_features_and_descriptor_orb_batch_device",
                                                             **kw)

    def get_features_and_descriptor_surf_batch_device(self, *args, **kw):
        """get_features_and_descriptor_batch_device on a handle of Vis/FeatureType 0 (set_feature_type_surf): same arguments,
        same return value; per keyframe the bytes of get_features_and_descriptor under type 0, float32 rows."""
        return self.get_features_and_descriptor_batch_device(*args, _call="sf_get_features_and_descriptor_surf_batch_device",
                                                             **kw)

    def surf_batch_status(self, check=True):
        """sf_surf_batch_status: waits for the stream; the number of keyframes of the most recent SURF batch call that had
        more maxima than their key capacity (they hold no rows).  check: raise SepfinderError (SF_ERANGE) when it is not 0."""
        n = C.c_int32()
        rc = self._L.sf_surf_batch_status(self._h, C.byref(n))
        if check or rc not in (_abi.SF_OK, _abi.SF_ERANGE):
            self._check(rc)
        return n.value

    def get_features_and_descriptor_sift_batch_device(self, *args, **kw):
        """get_features_and_descriptor_batch_device on a handle of Vis/FeatureType 1 (set_feature_type_sift): same arguments,
        same return value; per keyframe the bytes of get_features_and_descriptor under type 1, 128 float32 per row."""
        return self.get_features_and_descriptor_batch_device(*args, _call="sf_get_features_and_descriptor_sift_batch_device",
                                                             **kw)

    def sift_batch_status(self, check=True):
        """sf_sift_batch_status: waits for the stream; the number of keyframes of the most recent SIFT batch call that had
        more extrema or keypoints than an image holds (they hold no rows).  check: raise SepfinderError (SF_ERANGE) when it
        is not 0."""
        n = C.c_int32()
        rc = self._L.sf_sift_batch_status(self._h, C.byref(n))
        if check or rc not in (_abi.SF_OK, _abi.SF_ERANGE):
            self._check(rc)
        return n.value

    def debug_sift_batch_chunk(self, batch_chunk=0):
        """sf_debug_sift_batch_chunk (include/sf_experimental.h): the images per chunk of the SIFT batch forms, for tests on
        small shapes; 0 = what the workspace allows."""
        self._check(self._L.sf_debug_sift_batch_chunk(self._h, batch_chunk))

    def debug_surf_limits(self, candidate_cap=0, batch_chunk=0):
        """sf_debug_surf_limits (include/sf_experimental.h): the candidate capacity per image and the images per chunk of
        the SURF detector, for tests on small shapes; 0 = the default."""
        self._check(self._L.sf_debug_surf_limits(self._h, candidate_cap, batch_chunk))

    def extract_keyframe_device(self, d_left, width, height, pitch, d_kpts, d_right_x, d_status, n, cam,
                                d_desc_out=None, d_xyz_out=None, d_kpts_out=None, want_rows=True):
        """Device pointers (ints).  Returns (slot, rows kept or None)."""
        slot, rows = C.c_int32(), C.c_int32()
        self._check(self._L.sf_extract_keyframe_device(
            self._h, C.c_void_p(d_left), width, height, pitch, C.c_void_p(d_kpts), C.c_void_p(d_right_x),
            C.c_void_p(d_status), n, C.byref(cam), C.byref(slot), C.byref(rows) if want_rows else None,
            C.c_void_p(d_desc_out), C.c_void_p(d_xyz_out), C.c_void_p(d_kpts_out)))
        return slot.value, (rows.value if want_rows else None)

    # -- depth keyframes (RGB-D): 3D points from a registered depth image, Vis/DepthAsMask -----------------------------
    def depth_set_params(self, params):
        """The handle's _abi.DepthParams: Vis/DepthAsMask, whether the detector of the depth keyframe calls sees the mask
        of the depth image (types 3, 4, 5, 6, 8; types 0, 1, 2 need 0); 1 on a fresh handle."""
        self._check(self._L.sf_depth_set_params(self._h, C.byref(params)))

    def depth_get_params(self):
        p = _abi.DepthParams()
        self._check(self._L.sf_depth_get_params(self._h, C.byref(p)))
        return p

    def depth_set_size(self, size=None):
        """The handle's _abi.DepthSize: the depth images' own size in every depth call, whose width and height stay the
        image's (a decimated depth image); None or {0, 0}, a fresh handle's: the image's size."""
        self._check(self._L.sf_depth_set_size(self._h, C.byref(size) if size is not None else None))

    def depth_get_size(self):
        s = _abi.DepthSize()
        self._check(self._L.sf_depth_get_size(self._h, C.byref(s)))
        return s

    def depth_interpolate_device(self, d_depth, depth_format, depth_width, depth_height, depth_pitch, depth_stride, n_images,
                                 factor, d_out, out_pitch, out_stride):
        """util2d::interpolate of n_images device depth images (asynchronous): each enlarged by the integer factor, in its
        own format, to d_out; device pointers (ints), pitches and strides in bytes."""
        self._check(self._L.sf_depth_interpolate_device(self._h, C.c_void_p(d_depth), depth_format, depth_width, depth_height,
                                                        depth_pitch, int(depth_stride), n_images, factor, C.c_void_p(d_out),
                                                        out_pitch, int(out_stride)))

    def depth_register_device(self, reg, d_depth, depth_format, depth_pitch, depth_stride, n_images, d_out, out_pitch,
                              out_stride):
        """sf_depth_register_device: n_images device depth images of the depth camera registered to the colour camera
        under an _abi.DepthRegistration (asynchronous), each to a reg.width x reg.height image of its own format at d_out;
        device pointers (ints), pitches and strides in bytes."""
        self._check(self._L.sf_depth_register_device(self._h, C.byref(reg), C.c_void_p(d_depth), depth_format, depth_pitch,
                                                     int(depth_stride), n_images, C.c_void_p(d_out), out_pitch, int(out_stride)))

    def depth_fill_holes_device(self, d_depth, depth_format, width, height, depth_pitch, depth_stride, n_images, fill_vertical,
                                fill_horizontal, d_out, out_pitch, out_stride):
        """sf_depth_fill_holes_device: the hole filling of the registration alone, out of place, on n_images device images
        registered elsewhere (asynchronous)."""
        self._check(self._L.sf_depth_fill_holes_device(self._h, C.c_void_p(d_depth), depth_format, width, height, depth_pitch,
                                                       int(depth_stride), n_images, int(fill_vertical), int(fill_horizontal),
                                                       C.c_void_p(d_out), out_pitch, int(out_stride)))

    def debug_depth_register_limits(self, batch_chunk=0, stages=0):
        """sf_debug_depth_register_limits: the images per chunk and the stages (1 init, 2 scatter, 4 resolve; 0 = all) of
        depth_register_device, for the tests and the latency tool."""
        self._check(self._L.sf_debug_depth_register_limits(self._h, int(batch_chunk), int(stages)))

    def depth_register(self, depth, reg):
        """A host depth image ([depth_height, depth_width] uint16 millimetres or float32 metres) registered on the device:
        uploads it, runs sf_depth_register_device once, returns the registered [height, width] host image of the same dtype."""
        depth = np.ascontiguousarray(depth)
        fmt = _abi.depth_format_of(depth)
        if depth.ndim != 2 or depth.shape != (reg.depth_height, reg.depth_width):
            raise ValueError("the block registers depth images of %d x %d, not of shape %s" % (reg.depth_width, reg.depth_height,
                                                                                              depth.shape))
        import torch
        d_in = upload(depth.view(np.uint8), self.device)
        d_out = torch.zeros((max(reg.height, 1), max(reg.width, 1) * depth.itemsize), dtype=torch.uint8, device=d_in.device)
        torch.cuda.current_stream(d_in.device).synchronize()        # (the handle's stream may be another one)
        self.depth_register_device(reg, d_in.data_ptr(), fmt, depth.strides[0], 0, 1, d_out.data_ptr(), reg.width * depth.itemsize, 0)
        self.synchronize()
        return d_out.cpu().numpy().view(depth.dtype)

    def depth_mask_device(self, d_depth, depth_format, width, height, depth_pitch, depth_stride, n_images, min_depth,
                          max_depth, d_mask, mask_pitch, mask_stride):
        """The detector masks of n_images device depth images (asynchronous); device pointers (ints), pitches and strides
        in bytes."""
        self._check(self._L.sf_depth_mask_device(self._h, C.c_void_p(d_depth), depth_format, width, height, depth_pitch,
                                                 int(depth_stride), n_images, min_depth, max_depth, C.c_void_p(d_mask),
                                                 mask_pitch, int(mask_stride)))

    def depth_points_device(self, d_depth, depth_format, width, height, depth_pitch, d_kpts, n, cam, d_xyz_out,
                            d_valid_out=None):
        """The 3D points of n device keypoints from a device depth image (asynchronous): d_xyz_out [n][3] float32,
        d_valid_out [n] uint8 (optional)."""
        self._check(self._L.sf_depth_points_device(self._h, C.c_void_p(d_depth), depth_format, width, height, depth_pitch,
                                                   C.c_void_p(d_kpts), n, C.byref(cam), C.c_void_p(d_xyz_out),
                                                   C.c_void_p(d_valid_out)))

    def detect_corners_masked_device(self, d_image, width, height, pitch, d_mask, mask_pitch, max_corners, quality_level,
                                     min_distance, d_kpts_out, cap):
        """detect_corners_device as cv::goodFeaturesToTrack(image, ..., mask): d_mask a uint8 plane of the image's size."""
        n = C.c_int32()
        self._check(self._L.sf_detect_corners_masked_device(
            self._h, C.c_void_p(d_image), width, height, pitch, C.c_void_p(d_mask), mask_pitch, max_corners,
            float(quality_level), float(min_distance), C.c_void_p(d_kpts_out), cap, C.byref(n)))
        return n.value

    def detect_fast_masked_device(self, d_image, width, height, pitch, d_mask, mask_pitch, max_features, d_kpts_out, cap,
                                  params=None):
        """detect_fast_device as FastFeatureDetector::detect(image, keypoints, mask)."""
        n = C.c_int32()
        self._check(self._L.sf_detect_fast_masked_device(
            self._h, C.c_void_p(d_image), width, height, pitch, C.c_void_p(d_mask), mask_pitch, max_features,
            C.byref(params) if params is not None else None, C.c_void_p(d_kpts_out), cap, C.byref(n)))
        return n.value

    def extract_keyframe_depth_device(self, d_left, width, height, pitch, d_kpts, d_depth, depth_format, depth_pitch, n, cam,
                                      d_desc_out=None, d_xyz_out=None, d_kpts_out=None, want_rows=True):
        """extract_keyframe_device with the keyframe's depth image in place of d_right_x / d_status.  Returns (slot, rows
        kept or None)."""
        slot, rows = C.c_int32(), C.c_int32()
        self._check(self._L.sf_extract_keyframe_depth_device(
            self._h, C.c_void_p(d_left), width, height, pitch, C.c_void_p(d_kpts), C.c_void_p(d_depth), depth_format,
            depth_pitch, n, C.byref(cam), C.byref(slot), C.byref(rows) if want_rows else None, C.c_void_p(d_desc_out),
            C.c_void_p(d_xyz_out), C.c_void_p(d_kpts_out)))
        return slot.value, (rows.value if want_rows else None)

    def get_features_and_descriptor_depth(self, image, depth, cam, det=None, image_format=_abi.SF_IMAGE_MONO8):
        """GetFeatsAndDesc for a SensorData(rgb, depth, model) caller, on host arrays: image uint8 [h, w] (mono8) or
        [h, w, 3] (rgb8 / bgr8), depth uint16 [h, w] millimetres or float32 [h, w] metres, registered to the image -- after
        depth_set_size an array of that size.  Returns what get_features_and_descriptor returns."""
        image, w, h, image_pitch = _camera_image(image, image_format)
        depth = np.asarray(depth)
        fmt = _abi.depth_format_of(depth)
        size = self.depth_get_size()
        want = (size.depth_height or h, size.depth_width or w)
        if depth.shape != want or depth.strides[1] != depth.itemsize:
            raise ValueError("depth must be a 2-D array of %d rows and %d columns (%s) with contiguous rows, not of shape %s"
                             % (want + ("depth_set_size" if size.depth_width else "the image's height and width", depth.shape)))
        return self._host_keyframe(
            self._L.sf_get_features_and_descriptor_depth,
            (C.c_void_p(image.ctypes.data), image_format, C.c_void_p(depth.ctypes.data), fmt, w, h, image_pitch,
             depth.strides[0]), w, h, cam, det)

    def get_features_and_descriptor_depth_batch_device(self, d_images, d_depth, depth_format, n_keyframes, width, height,
                                                       image_pitch, image_stride, depth_pitch, depth_stride, cam, det=None,
                                                       d_rows_out=None, d_desc_out=None, d_xyz_out=None, d_kpts_out=None):
        """n depth keyframes from device MONO8 planes and depth planes to n store slots in one launch sequence, no host
        wait, under every feature type; outputs as get_features_and_descriptor_batch_device.  Returns the first slot."""
        first = C.c_int32()
        self._check(self._L.sf_get_features_and_descriptor_depth_batch_device(
            self._h, C.c_void_p(d_images), C.c_void_p(d_depth), depth_format, n_keyframes, width, height, image_pitch,
            int(image_stride), depth_pitch, int(depth_stride), C.byref(cam), C.byref(det) if det is not None else None,
            C.byref(first), C.c_void_p(d_rows_out), C.c_void_p(d_desc_out), C.c_void_p(d_xyz_out), C.c_void_p(d_kpts_out)))
        return first.value

    def add_keyframes_depth_batch_device(self, d_images, image_format, d_depth, depth_format, n_keyframes, width, height,
                                         image_pitch, image_stride, depth_pitch, depth_stride, cam, det=None,
                                         d_rows_out=None, d_desc_out=None, d_xyz_out=None, d_kpts_out=None):
        """add_keyframes_u8_batch_device for depth keyframes: the colour images feed the network and, as gray planes, the
        depth stages.  Returns (first store slot, first local NN row)."""
        first, row = C.c_int32(), C.c_int32()
        self._check(self._L.sf_add_keyframes_depth_batch_device(
            self._h, C.c_void_p(d_images), image_format, C.c_void_p(d_depth), depth_format, n_keyframes, width, height,
            image_pitch, int(image_stride), depth_pitch, int(depth_stride), C.byref(cam),
            C.byref(det) if det is not None else None, C.byref(first), C.byref(row), C.c_void_p(d_rows_out),
            C.c_void_p(d_desc_out), C.c_void_p(d_xyz_out), C.c_void_p(d_kpts_out)))
        return first.value, row.value

    def store_size(self):
        n = C.c_int32()
        self._check(self._L.sf_store_size(self._h, C.byref(n)))
        return n.value

    def store_clear(self):
        self._check(self._L.sf_store_clear(self._h))

    # -- raw camera images: rectification plans (include/sepfinder.h: sf_camera_info) -----------------
    def rectify_plan_create(self, info):
        """sf_rectify_plan_create: validates an _abi.CameraInfo and stores its plan; returns the plan id (1, 2, ..)."""
        pid = C.c_int32()
        self._check(self._L.sf_rectify_plan_create(self._h, C.byref(info), C.byref(pid)))
        return pid.value

    def rectify_plan_from_maps(self, mapx, mapy, src_width, src_height):
        """sf_rectify_plan_from_maps: a plan from the caller's float32 maps [out_h, out_w] (host arrays) into a source of
        src_width x src_height; returns the plan id."""
        mx, my = np.ascontiguousarray(mapx, np.float32), np.ascontiguousarray(mapy, np.float32)
        if mx.ndim != 2 or mx.shape != my.shape:
            raise ValueError("mapx / mapy must be two [out_h, out_w] arrays of one shape")
        pid = C.c_int32()
        self._check(self._L.sf_rectify_plan_from_maps(self._h, C.c_void_p(mx.ctypes.data), C.c_void_p(my.ctypes.data), mx.shape[1],
                                                      mx.shape[0], mx.strides[0], int(src_width), int(src_height), C.byref(pid)))
        return pid.value

    def rectify_plan_count(self):
        n = C.c_int32()
        self._check(self._L.sf_rectify_plan_count(self._h, C.byref(n)))
        return n.value

    def rectify_plan_get(self, plan):
        """sf_rectify_plan_get: (the _abi.CameraInfo the plan was created from, whether it is a plan of caller maps)."""
        info, from_maps = _abi.CameraInfo(), C.c_int32()
        self._check(self._L.sf_rectify_plan_get(self._h, int(plan), C.byref(info), C.byref(from_maps)))
        return info, bool(from_maps.value)

    def rectify_plan_clear(self):
        self._check(self._L.sf_rectify_plan_clear(self._h))

    def rectify_maps_device(self, plan, d_mapx, d_mapy, pitch_bytes):
        """sf_rectify_maps_device: a computed plan's float32 maps into device arrays (raw pointers); asynchronous."""
        self._check(self._L.sf_rectify_maps_device(self._h, int(plan), C.c_void_p(d_mapx), C.c_void_p(d_mapy), int(pitch_bytes)))

    def image_rectify_device(self, plan_a, d_src_a, plan_b, d_src_b, fmt, out_fmt, n_images, src_pitch, src_stride, d_dst_a,
                             d_dst_b, dst_pitch, dst_stride):
        """sf_image_rectify_device: n_images raw device images under plan_a and (d_src_b not None) as many under plan_b in one
        launch, to images in out_fmt (fmt, or SF_IMAGE_MONO8 from a colour format: the fused gray); asynchronous."""
        self._check(self._L.sf_image_rectify_device(self._h, int(plan_a), C.c_void_p(d_src_a), int(plan_b), C.c_void_p(d_src_b),
                                                    int(fmt), int(out_fmt), int(n_images), int(src_pitch), int(src_stride),
                                                    C.c_void_p(d_dst_a), C.c_void_p(d_dst_b), int(dst_pitch), int(dst_stride)))

    def rectify_pair(self, left, right, fmt, plan_left, plan_right, out_fmt=None):
        """A raw host pair ([h, w, 3] rgb8 / bgr8 or [h, w] mono8) rectified on the device under two plans: uploads both
        images, runs sf_image_rectify_device once, returns the two rectified host images in out_fmt (None: fmt)."""
        out_fmt = fmt if out_fmt is None else out_fmt
        left, w, h, pitch = _camera_image(left, fmt)
        right, w2, h2, pitch2 = _camera_image(right, fmt)
        if (w, h) != (w2, h2):
            raise ValueError("left / right must be images of one shape")
        info = self.rectify_plan_get(plan_left)[0]
        if (info.width, info.height) != (w, h):
            raise ValueError("plan %d rectifies %d x %d images, not %d x %d" % (plan_left, info.width, info.height, w, h))
        ow, oh = info.out_width or info.width, info.out_height or info.height
        import torch
        d_l, d_r = upload(np.ascontiguousarray(left), self.device), upload(np.ascontiguousarray(right), self.device)
        shape = (oh, ow) if out_fmt == _abi.SF_IMAGE_MONO8 else (oh, ow, 3)
        d_out = torch.zeros((2,) + shape, dtype=torch.uint8, device=d_l.device)
        torch.cuda.current_stream(d_l.device).synchronize()        # (the handle's stream may be another one)
        row = ow * (1 if out_fmt == _abi.SF_IMAGE_MONO8 else 3)
        self.image_rectify_device(plan_left, d_l.data_ptr(), plan_right, d_r.data_ptr(), fmt, out_fmt, 1,
                                  w * (1 if fmt == _abi.SF_IMAGE_MONO8 else 3), 0, d_out[0].data_ptr(), d_out[1].data_ptr(), row, 0)
        self.synchronize()
        out = d_out.cpu().numpy()
        return out[0], out[1]

    # -- a camera model per keyframe (include/sepfinder.h: sf_camera_model) ---------------------------
    def camera_add(self, model):
        """sf_camera_add: adds an _abi.CameraModel to the handle's table; returns its id (1, 2, ..)."""
        cid = C.c_int32()
        self._check(self._L.sf_camera_add(self._h, C.byref(model), C.byref(cid)))
        return cid.value

    def camera_get(self, cam_id):
        """sf_camera_get: the model behind an id (0: the handle's sf_params camera)."""
        m = _abi.CameraModel()
        self._check(self._L.sf_camera_get(self._h, int(cam_id), C.byref(m)))
        return m

    def camera_count(self):
        n = C.c_int32()
        self._check(self._L.sf_camera_count(self._h, C.byref(n)))
        return n.value

    def camera_select(self, cam_id):
        """sf_camera_select: slots appended from now on carry this id."""
        self._check(self._L.sf_camera_select(self._h, int(cam_id)))

    def store_set_camera(self, first_slot, n, cam_id):
        self._check(self._L.sf_store_set_camera(self._h, int(first_slot), int(n), int(cam_id)))

    def store_get_camera(self, slot):
        cid = C.c_int32()
        self._check(self._L.sf_store_get_camera(self._h, int(slot), C.byref(cid)))
        return cid.value

    # -- store slots as bytes (include/sepfinder.h: sf_kfblob_header) ---------------------------------
    def export_plan(self, first_slot, n):
        """sf_store_export_plan: (total bytes, largest row count) of the blob of slots [first_slot, first_slot + n); waits
        for the stream."""
        total, max_rows = C.c_uint64(), C.c_int32()
        self._check(self._L.sf_store_export_plan(self._h, int(first_slot), int(n), C.byref(total), C.byref(max_rows)))
        return total.value, max_rows.value

    def export_keyframes_device(self, first_slot, n, d_blob, cap_bytes):
        """sf_store_export_keyframes_device: the blob of slots [first_slot, first_slot + n) into device memory (a raw,
        16-byte aligned pointer and its length); asynchronous on the handle's stream.  A blob that does not fit is
        reported by wire_status, not written."""
        self._check(self._L.sf_store_export_keyframes_device(self._h, int(first_slot), int(n), C.c_void_p(d_blob),
                                                             int(cap_bytes)))

    def import_keyframes_device(self, d_blob, nbytes, n, max_rows, cols):
        """sf_store_import_keyframes_device: appends the n keyframes of the blob in device memory (a raw, 16-byte aligned
        pointer and its length); asynchronous, always n slots.  Returns the first slot; wire_status says what was refused."""
        first = C.c_int32()
        self._check(self._L.sf_store_import_keyframes_device(self._h, C.c_void_p(d_blob), int(nbytes), int(n), int(max_rows),
                                                             int(cols), C.byref(first)))
        return first.value

    def wire_status(self, check=True):
        """sf_store_wire_status: waits for the stream; [bits, emptied slots, first emptied keyframe or -1, 0] of the most
        recent export or import (bits: _abi.WIRE_*).  check: raise SepfinderError (SF_ERANGE) when a bit is set."""
        out = (C.c_int32 * 4)()
        rc = self._L.sf_store_wire_status(self._h, out)
        if check or rc not in (_abi.SF_OK, _abi.SF_ERANGE):
            self._check(rc)
        return list(out)

    def _wire_staging(self, nbytes):
        import torch
        return torch.empty(max(int(nbytes), 32), dtype=torch.uint8, device=torch.device("cuda:%d" % self.device))

    def export_keyframes(self, first_slot, n):
        """Slots [first_slot, first_slot + n) as the bytes of one blob: what a robot sends for a GetFeatsAndDesc request.
        Staged through a torch tensor on the handle's device."""
        total, _ = self.export_plan(first_slot, n)
        t = self._wire_staging(total)
        self.export_keyframes_device(first_slot, n, t.data_ptr(), total)
        self.wire_status()
        return t[:total].cpu().numpy().tobytes()

    def import_keyframes(self, blob, check=True):
        """Appends the keyframes of a blob received as bytes; n, max_rows and the descriptor width are read from its header
        and table HERE, on the host, and checked again on the device.  Returns (first slot, n); check: raise when the
        device refused the header or an entry (the slots exist either way, empty)."""
        import torch
        raw = np.frombuffer(bytes(blob), np.uint8)
        if raw.size < 32:
            raise ValueError("a keyframe blob has at least 32 bytes, not %d" % raw.size)
        hdr = raw[:32].view(_abi.KFBLOB_HEADER_DTYPE)[0]
        n, max_rows = int(hdr["n_keyframes"]), int(hdr["max_rows"])
        if not 0 <= n <= 65535 or raw.size < 32 + 32 * n or max_rows < 0:
            raise ValueError("keyframe blob of %d bytes states %d keyframes of up to %d rows" % (raw.size, n, max_rows))
        table = raw[32: 32 + 32 * n].view(_abi.KFBLOB_ENTRY_DTYPE)
        cols = int(table["cols"].max()) if n else max(1, self.params.desc_bytes)
        t = self._wire_staging(raw.size)
        t[:raw.size].copy_(torch.from_numpy(raw.copy()))
        torch.cuda.current_stream(t.device).synchronize()      # (the handle's stream is not torch's)
        first = self.import_keyframes_device(t.data_ptr(), raw.size, n, max_rows, cols)
        self.wire_status(check=check)       # (waits: the staging tensor may go)
        return first, n

    # -- verification -----------------------------------------------------------------------------
    def estimate_transform(self, f_from, f_to):
        res = np.zeros(1, dtype=_abi.RESULT_DTYPE)
        a, b = f_from.c_struct(), f_to.c_struct()
        self._check(self._L.sf_estimate_transform(self._h, C.byref(a), C.byref(b), res.ctypes.data))
        return res[0]

    def estimate_transform_batch(self, feats_from, feats_to):
        n = len(feats_from)
        res = np.zeros(n, dtype=_abi.RESULT_DTYPE)
        if n == 0:
            return res
        fa, ta = _abi.features_array(feats_from), _abi.features_array(feats_to)
        self._check(self._L.sf_estimate_transform_batch(self._h, fa, ta, n, res.ctypes.data))
        return res

    def verify_pairs(self, from_slots, to_slots):
        f = np.ascontiguousarray(from_slots, dtype=np.int32)
        t = np.ascontiguousarray(to_slots, dtype=np.int32)
        res = np.zeros(f.size, dtype=_abi.RESULT_DTYPE)
        self._check(self._L.sf_verify_pairs(self._h, _ptr(f), _ptr(t), f.size, _ptr(res)))
        return res

    def verify_pairs_device(self, d_from, d_to, n, d_out):
        self._check(self._L.sf_verify_pairs_device(self._h, C.c_void_p(d_from), C.c_void_p(d_to), n,
                                                   C.c_void_p(d_out)))

    def verify_matches_device(self, matches, slot_base_other, slot_base_local, d_out):
        """Verify the candidates of an NN query (structured array of MATCH_DTYPE, host) -> d_out (device)."""
        m = np.ascontiguousarray(matches, dtype=_abi.MATCH_DTYPE)
        self._check(self._L.sf_verify_matches_device(self._h, _ptr(m), m.size, slot_base_other, slot_base_local,
                                                     C.c_void_p(d_out)))
        return m.size

    def find_matches_and_verify_device(self, slot_base_other, slot_base_local, d_out, cap=None):
        """nn_find_matches + verify_matches_device as one call (speculative verification of the NN candidates
        while the host walks them, when the walk may return every local row); returns the matches, their
        results are written to d_out (device) asynchronously."""
        n_l, _ = self.nn_sizes()
        if cap is None:
            cap = max(1, min(max(n_l, 1), self.params.netvlad_max_matches_nb))
        out = np.zeros(max(cap, 1), dtype=_abi.MATCH_DTYPE)
        n = C.c_int32()
        self._check(self._L.sf_find_matches_and_verify_device(self._h, slot_base_other, slot_base_local, _ptr(out), cap,
                                                              C.byref(n), C.c_void_p(d_out) if d_out else None))
        return out[: n.value]

    # -- the caller's loop body as a begin / retire pair (find_separators.py:59-133) ----------------------------------
    def step_issue(self, slot_base_other, slot_base_local):
        """Queue one find-and-verify step (NN search, walk, verification of every returned candidate, all on the
        device); does not wait for any of it.  At most SF_OPT_STEP_DEPTH (default 6) steps in flight; with a mirror set
        (step_mirror / step_mirror_pair) as many as the mirror has buffers."""
        self._check(self._L.sf_step_issue(self._h, int(slot_base_other), int(slot_base_local)))

    def step_retire(self, copy=False):
        """The oldest step in flight: (matches, record_of_match, records, info).  The arrays are VIEWS of memory the
        handle owns (valid until the next step_retire) unless copy=True; records[record_of_match[i]] is the
        accepted result of match i, record_of_match[i] = -1 means its estimation failed."""
        r = _abi.StepResult()
        self._check(self._L.sf_step_retire(self._h, C.byref(r)))
        n, nr = r.n_matches, r.n_records

        def view(ptr, count, dtype):
            if not ptr or count <= 0:
                return np.zeros(0, dtype=dtype)
            buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            a = np.frombuffer(buf, dtype=dtype, count=count)
            return a.copy() if copy else a
        return (view(r.matches, n, _abi.MATCH_DTYPE), view(r.record_of_match, n, np.int32),
                view(r.records, nr, _abi.RESULT_DTYPE),
                {"n_matches": n, "n_records": nr, "n_accepted": r.n_accepted, "streamed": bool(r.streamed),
                 "d_records": r.d_records or 0})

    def memcpy_device_async(self, d_dst, d_src, nbytes, stream=None):
        """Device-to-device copy (raw pointers) on `stream` (a hipStream_t as an integer; None: the handle's stream), e.g. a
        retired step's d_records -> a send buffer."""
        self._check(self._L.sf_memcpy_device_async(self._h, C.c_void_p(d_dst), C.c_void_p(d_src), int(nbytes),
                                                   C.c_void_p(stream) if stream else None))

    def step_mirror(self, d_records2, d_counter, cap):
        """Second (device) destination of every accepted record + the caller's slot counter; (None, None, 0) removes it."""
        self._check(self._L.sf_step_mirror(self._h, C.c_void_p(d_records2) if d_records2 else None,
                                           C.c_void_p(d_counter) if d_counter else None, int(cap)))

    def step_mirror_pair(self, even, odd, cap):
        """Two alternating mirrors, (d_records2, d_counter) each: the first step issued after this call writes `even`."""
        self._check(self._L.sf_step_mirror_pair(self._h, C.c_void_p(even[0]), C.c_void_p(even[1]),
                                                C.c_void_p(odd[0]), C.c_void_p(odd[1]), int(cap)))

    def step_mirror_streams(self):
        """(stream_even, stream_odd) as integers: after step_mirror_pair, odd steps move to the handle's second stream."""
        a, b = C.c_void_p(), C.c_void_p()
        self._check(self._L.sf_step_mirror_streams(self._h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def last_match_results(self):
        """(d_results pointer, index pointer or None, n) of the last find_matches_and_verify_device call."""
        r, ix, n = C.c_void_p(), C.c_void_p(), C.c_int32()
        self._check(self._L.sf_last_match_results(self._h, C.byref(r), C.byref(ix), C.byref(n)))
        return r.value, ix.value, n.value

    def compact_accepted_indexed_device_async(self, d_results, index, n, d_accepted, d_flags, d_count):
        self._check(self._L.sf_compact_accepted_indexed_device_async(
            self._h, C.c_void_p(d_results), C.c_void_p(index), n, C.c_void_p(d_accepted),
            C.c_void_p(d_flags) if d_flags else None, C.c_void_p(d_count)))

    def accept_stream_set(self, which, records, index, flags, cap, d_records2=None, d_counter=None):
        """Register block `which` (0 / 1) of the accepted-result stream: pinned host pointers (ints); optionally a
        second (device) destination of every record and a caller-owned device counter."""
        self._check(self._L.sf_accept_stream_set(self._h, which, C.c_void_p(records), C.c_void_p(index),
                                                 C.c_void_p(flags) if flags else None, cap,
                                                 C.c_void_p(d_records2) if d_records2 else None,
                                                 C.c_void_p(d_counter) if d_counter else None))

    def accept_stream_select(self, which):
        self._check(self._L.sf_accept_stream_select(self._h, which))

    def accept_stream_status(self):
        """(streamed, pairs) of the last sf_find_matches_and_verify_device."""
        s, n = C.c_int32(), C.c_int32()
        self._check(self._L.sf_accept_stream_status(self._h, C.byref(s), C.byref(n)))
        return bool(s.value), n.value

    def compact_accepted_indexed_mirrored_device_async(self, d_results, index, n, d_accepted, d_flags, d_count, d_accepted2,
                                                       d_flags2, d_count2):
        self._check(self._L.sf_compact_accepted_indexed_mirrored_device_async(
            self._h, C.c_void_p(d_results), C.c_void_p(index), n, C.c_void_p(d_accepted),
            C.c_void_p(d_flags) if d_flags else None, C.c_void_p(d_count), C.c_void_p(d_accepted2),
            C.c_void_p(d_flags2) if d_flags2 else None, C.c_void_p(d_count2)))

    def compact_accepted_device(self, d_results, n, d_accepted, d_flags=None):
        """Ordered device-side compaction of the accepted results; returns their number."""
        k = C.c_int32()
        self._check(self._L.sf_compact_accepted_device(self._h, C.c_void_p(d_results), n, C.c_void_p(d_accepted),
                                                       C.c_void_p(d_flags) if d_flags else None, C.byref(k)))
        return k.value

    def compact_accepted_device_async(self, d_results, n, d_accepted, d_flags, d_count):
        """The same without the synchronisation: the count (int32) is left on the device at d_count."""
        self._check(self._L.sf_compact_accepted_device_async(self._h, C.c_void_p(d_results), n, C.c_void_p(d_accepted),
                                                             C.c_void_p(d_flags) if d_flags else None, C.c_void_p(d_count)))

    def debug_pass_state(self, pair, which_pass):
        """(T [3][4] float32, is_null, inliers, matches) of one pass of pair `pair` of the last verification."""
        T = np.zeros(12, dtype=np.float32)
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.sf_debug_pass_state(self._h, pair, which_pass, T.ctypes.data, C.byref(a), C.byref(b), C.byref(c)))
        return T.reshape(3, 4), a.value, b.value, c.value

    def debug_knn2_u8(self, slot_from, slot_to, rows_to):
        """sf_debug_knn2_u8 (include/sf_experimental.h; a handle with desc_type 2): the kNN-2 scan of the uint8 L2 matcher
        for one pair of store slots -> (d_best, d_second, i_best), int32 [rows_to]: per row of the "to" keyframe (rows_to =
        its rows) the smallest and second smallest squared distance to the "from" rows (2^31 - 1: none) and the lowest
        "from" row at the smallest (-1: none).  The integers a desc_type 1 handle computes in float32 on the float twin
        (rows.astype(float32)) -- which is how the oracle, which knows desc_type 0 and 1 only, is asked about such rows:
        desc_type 1, desc_bytes 512, the rows as float32."""
        d1 = np.zeros(max(rows_to, 1), np.int32); d2 = np.zeros_like(d1); i1 = np.zeros_like(d1)
        self._check(self._L.sf_debug_knn2_u8(self._h, slot_from, slot_to, d1.ctypes.data, d2.ctypes.data, i1.ctypes.data))
        return d1[:rows_to], d2[:rows_to], i1[:rows_to]

    def debug_guided_points(self, pair, kcap=4096):
        a = np.zeros(kcap, dtype=np.uint64); b = np.zeros(kcap, dtype=np.uint64)
        k = C.c_int32()
        self._check(self._L.sf_debug_guided_points(self._h, pair, a.ctypes.data, b.ctypes.data, C.byref(k)))
        return a[: k.value].copy(), b[: k.value].copy()

    def debug_counters(self, n=8):
        out = np.zeros(n, dtype=np.uint64)
        self._check(self._L.sf_debug_counters(self._h, out.ctypes.data, n))
        return out

    def debug_correspondences(self, pair, which_pass, cap=4096):
        cf = np.zeros(cap, dtype=np.uint16)
        ct = np.zeros(cap, dtype=np.uint16)
        n = C.c_int32()
        self._check(self._L.sf_debug_correspondences(self._h, pair, which_pass, cf.ctypes.data,
                                                     ct.ctypes.data, cap, C.byref(n)))
        return cf[: n.value].copy(), ct[: n.value].copy()

    # -- multi-GPU exchange (RCCL through the C-ABI) --------------------------------------------------
    def comm_init(self, unique_id, rank, world):
        uid = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
        self._check(self._L.sf_comm_init(self._h, uid.ctypes.data, rank, world))

    def comm_destroy(self):
        self._check(self._L.sf_comm_destroy(self._h))

    def allgather_separators(self, d_local, n_local, d_all, cap_per_rank, world):
        counts = np.zeros(world, dtype=np.int32)
        self._check(self._L.sf_allgather_separators(self._h, C.c_void_p(d_local), n_local, C.c_void_p(d_all),
                                                    cap_per_rank, counts.ctypes.data))
        return counts

    # -- measurement ------------------------------------------------------------------------------
    def allgather_separators_device(self, d_send, d_all, cap_per_rank):
        """One-collective exchange on device buffers with a device-stamped count (see include/sepfinder.h)."""
        self._check(self._L.sf_allgather_separators_device(self._h, C.c_void_p(d_send), C.c_void_p(d_all), cap_per_rank))

    def prof_enable(self, on=True):
        self._check(self._L.sf_prof_enable(self._h, int(on)))

    def prof_select(self, names=None):
        """Bracket only the named kernels (sf_kernel_name strings) while profiling is on; None = all."""
        mask = 0xFFFFFFFF
        if names is not None:
            mask = 0
            for k in range(_abi.SF_K_COUNT):
                if self._L.sf_kernel_name(k).decode() in names:
                    mask |= 1 << k
        self._check(self._L.sf_prof_select(self._h, mask))

    def stream_placement(self):
        """One line on where the step pipeline's streams sit on the dispatch pipes (include/sf_experimental.h)."""
        buf = C.create_string_buffer(512)
        self._check(self._L.sf_stream_placement(self._h, buf, 512))
        return buf.value.decode()

    def streams_prepare(self):
        """Run the stream placement measurement now (60-100 ms; otherwise inside the first overlapped step)."""
        self._check(self._L.sf_streams_prepare(self._h))

    def prof_reset(self):
        self._check(self._L.sf_prof_reset(self._h))

    def prof_get(self):
        """{kernel name: (launches, total_ms)} measured with hipEvents on the handle's stream."""
        out = {}
        for k in range(_abi.SF_K_COUNT):
            n, ms = C.c_int64(), C.c_double()
            self._check(self._L.sf_prof_get(self._h, k, C.byref(n), C.byref(ms)))
            out[self._L.sf_kernel_name(k).decode()] = (n.value, ms.value)
        return out


def comm_unique_id():
    """ncclUniqueId bytes (created by one rank, distributed by the host side)."""
    L = load()
    out = np.zeros(128, dtype=np.uint8)
    rc = L.sf_comm_unique_id(out.ctypes.data, 128)
    if rc != 0:
        raise SepfinderError(rc, "sf_comm_unique_id (is librccl.so loadable?)")
    return out.tobytes()


def pack_separators(results, robot_from, robot_to, kf_from, kf_to, frame_from, frame_to):
    """ReceiveSeparators.srv rows (one per result) as a structured array of SEPARATOR_DTYPE."""
    L = load()
    res = np.ascontiguousarray(results, dtype=_abi.RESULT_DTYPE)
    n = res.size
    arrs = [np.ascontiguousarray(a, dtype=np.int16) for a in (kf_from, kf_to, frame_from, frame_to)]
    for a in arrs:
        if a.size != n:
            raise ValueError("id arrays must have one entry per result")
    for v in (robot_from, robot_to):
        if not -128 <= int(v) <= 127:
            raise ValueError("robot ids are int8 on the wire (ReceiveSeparators.srv:1-2)")
    out = np.zeros(n, dtype=_abi.SEPARATOR_DTYPE)
    rc = L.sf_pack_separators(_ptr(res), n, int(robot_from), int(robot_to), _ptr(arrs[0]), _ptr(arrs[1]),
                              _ptr(arrs[2]), _ptr(arrs[3]), _ptr(out))
    if rc != 0:
        raise SepfinderError(rc, "sf_pack_separators")
    return out
