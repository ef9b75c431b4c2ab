"""ctypes binding of liborbfe.so (the HIP product library) and the host-side mirror of the
reference interface for the hot path:

* :class:`ORBextractor` mirrors ``ORB_SLAM2::ORBextractor`` (include/ORBextractor.h:50-119):
  same ctor arguments, ``__call__(image, mask)`` for ``operator()`` and the six getters; the
  frame-side steps that read its outputs hang off it too (``ComputeStereoMatches``,
  ``ComputeStereoFromRGBD`` with ``depth_buffer``);
* :class:`ORBmatcher` mirrors the hot subset of ``ORB_SLAM2::ORBmatcher``
  (include/ORBmatcher.h:38-110): ``DescriptorDistance``, ``SearchForInitialization`` and the two
  tracking ``SearchByProjection`` overloads, the search of ``Fuse`` (``FuseSearch``,
  ``fuse_search_batch_device``), ``SearchForTriangulation`` (and
  ``search_for_triangulation_batch_device``), the loop-closing matchers
  (``SearchByBoWKeyFrames``, ``SearchBySim3``, ``SearchByProjectionSim3``), plus the brute-force
  match of config 3 and the close-point rule of the RGB-D / stereo tracking loops
  (``ClosePoints``).

There is no CPU fallback: importing works anywhere, but constructing an extractor or matcher
needs the built library and a gfx950 device, and raises otherwise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .abi import (KEYPOINT_DTYPE, ORBFE_ERR_CAPACITY, ORBFE_ERR_UNSUPPORTED, ORBFE_OK, Camera, Frame, FrameView,
                  MapPoints, MapPointView, OrbfeError, Params, ptr)

_HERE = os.path.dirname(os.path.abspath(__file__))
# ORBFE_LIB selects another build of the same library (A/B runs of build variants)
LIB_PATH = os.environ.get("ORBFE_LIB") or os.path.join(_HERE, "lib", "liborbfe.so")
_lib: C.CDLL | None = None

# every symbol include/orbfe.h declares (checked by tests/test_abi.py)
EXPORTED = [
    "orbfe_create", "orbfe_destroy", "orbfe_get_levels", "orbfe_get_scale_factor",
    "orbfe_get_scale_tables", "orbfe_get_features_per_level", "orbfe_keypoint_capacity",
    "orbfe_keypoint_capacity_for", "orbfe_keypoint_capacity_params", "orbfe_set_arithmetic", "orbfe_get_arithmetic",
    "orbfe_get_reference_constants",
    "orbfe_extract", "orbfe_input_buffer", "orbfe_extract_staged", "orbfe_staged_outputs",
    "orbfe_extract_color", "orbfe_human_mask_rect", "orbfe_extract_batch",
    "orbfe_extract_batch_device", "orbfe_extract_color_batch_device", "orbfe_set_stream",
    "orbfe_synchronize", "orbfe_compute_stereo_matches", "orbfe_compute_stereo_matches_device",
    "orbfe_stereo_status", "orbfe_profile", "orbfe_profile_read", "orbfe_pyramid_path", "orbfe_pyramid_tail", "orbfe_describe_blur_fragments", "orbfe_debug_replay", "orbfe_set_stage_mask", "orbfe_get_level", "orbfe_get_blurred_level", "orbfe_get_fast_keys",
    "orbfe_matcher_create", "orbfe_matcher_destroy", "orbfe_matcher_set_stream",
    "orbfe_matcher_profile", "orbfe_matcher_profile_read", "orbfe_matcher_profile_read_stages", "orbfe_hamming",
    "orbfe_bf_match", "orbfe_bf_match_batch_device", "orbfe_search_for_initialization",
    "orbfe_search_by_projection_local", "orbfe_search_by_projection_last",
    "orbfe_search_by_projection_keyframe", "orbfe_fuse_search",
    "orbfe_fuse_search_batch_device", "orbfe_distinctive_descriptors",
    "orbfe_distinctive_descriptors_device", "orbfe_search_local_points_device",
    "orbfe_search_by_projection_local_device",
    "orbfe_matcher_last_rounds", "orbfe_matcher_capacity_retries", "orbfe_features_in_area", "orbfe_is_in_frustum", "orbfe_vocabulary_load_text",
    "orbfe_vocabulary_create", "orbfe_vocabulary_destroy", "orbfe_vocabulary_info",
    "orbfe_vocabulary_set_stream", "orbfe_bow_transform", "orbfe_bow_transform_batch_device",
    "orbfe_search_by_bow", "orbfe_search_by_bow_batch_device",
    "orbfe_search_by_bow_keyframes", "orbfe_search_by_bow_keyframes_batch_device",
    "orbfe_search_by_projection_sim3", "orbfe_search_by_sim3",
    "orbfe_search_for_triangulation", "orbfe_search_for_triangulation_batch_device",
    "orbfe_vocabulary_set_arithmetic", "orbfe_vocabulary_score",
    "orbfe_vocabulary_score_batch_device",
    "orbfe_kfdb_create", "orbfe_kfdb_destroy", "orbfe_kfdb_set_stream", "orbfe_kfdb_size",
    "orbfe_kfdb_add", "orbfe_kfdb_add_device", "orbfe_kfdb_erase", "orbfe_kfdb_clear",
    "orbfe_kfdb_set_covisibility", "orbfe_kfdb_set_scores", "orbfe_kfdb_get_state",
    "orbfe_kfdb_detect_loop_candidates", "orbfe_kfdb_detect_relocalization_candidates",
    "orbfe_kfdb_detect_loop_candidates_device",
    "orbfe_kfdb_detect_relocalization_candidates_device",
    "orbfe_map_create", "orbfe_map_destroy", "orbfe_map_set_stream", "orbfe_map_clear",
    "orbfe_map_size", "orbfe_map_add_keyframe", "orbfe_map_set_keyframe_points",
    "orbfe_map_set_keyframe_bad", "orbfe_map_set_covisibility", "orbfe_map_set_children",
    "orbfe_map_set_parent", "orbfe_map_add_points", "orbfe_map_set_points_bad",
    "orbfe_map_add_observations", "orbfe_map_erase_observations", "orbfe_map_set_stamps",
    "orbfe_map_get_stamps", "orbfe_map_set_local_keyframes", "orbfe_map_get_local_keyframes",
    "orbfe_map_update_local", "orbfe_map_update_local_device", "orbfe_map_local_points_device",
    "orbfe_map_get_local_points", "orbfe_map_gather_points_device",
    "orbfe_map_update_connections", "orbfe_map_add_connection", "orbfe_map_erase_connection",
    "orbfe_map_update_best_covisibles", "orbfe_map_erase_keyframe_connections",
    "orbfe_map_set_connections", "orbfe_map_set_ordered_connections",
    "orbfe_map_set_first_connection", "orbfe_map_get_connections",
    "orbfe_map_get_ordered_connections", "orbfe_map_get_spanning_tree",
    "orbfe_map_set_keyframe_features", "orbfe_map_get_keyframe_features",
    "orbfe_map_add_observations_idx", "orbfe_map_erase_observation",
    "orbfe_map_set_point_bad_flag", "orbfe_map_set_point_counters",
    "orbfe_map_get_point_counters", "orbfe_map_increase_counters",
    "orbfe_map_increase_counters_device", "orbfe_map_cull_points",
    "orbfe_map_tracked_map_points", "orbfe_map_get_keyframe_points",
    "orbfe_map_get_observations", "orbfe_map_get_bad_flags",
    "orbfe_map_set_not_erase", "orbfe_map_get_erase_flags", "orbfe_map_set_keyframe_bad_flag",
    "orbfe_map_set_erase", "orbfe_map_cull_keyframes",
    "orbfe_map_set_scale_factors", "orbfe_map_get_scale_factors",
    "orbfe_map_set_keyframe_centers", "orbfe_map_get_keyframe_centers",
    "orbfe_map_set_keyframe_descriptors", "orbfe_map_set_keyframe_descriptors_device",
    "orbfe_map_get_keyframe_descriptors", "orbfe_map_set_point_ref_keyframes",
    "orbfe_map_get_point_ref_keyframes", "orbfe_map_refresh_points",
    "orbfe_map_refresh_points_device", "orbfe_map_refresh_keyframe_points",
    "orbfe_map_process_new_keyframe",
    "orbfe_archive_mat_bytes",
    "orbfe_archive_write_keypoints_device", "orbfe_archive_read_keypoints_device",
    "orbfe_archive_write_descriptors_device", "orbfe_archive_read_descriptors_device",
    "orbfe_compute_stereo_from_rgbd", "orbfe_depth_buffer",
    "orbfe_compute_stereo_from_rgbd_device", "orbfe_rgbd_status",
    "orbfe_close_points", "orbfe_close_points_batch_device",
]

DEPTH_U16, DEPTH_F32 = 0, 1            # ORBFE_DEPTH_*
CLOSE_SORTED, CLOSE_ALL = 0, 1         # ORBFE_CLOSE_*
CLOSE_MAX_KEPT = 8192                  # ORBFE_CLOSE_MAX_KEPT
_DEPTH_DTYPES = {DEPTH_U16: np.dtype(np.uint16), DEPTH_F32: np.dtype(np.float32)}


def _depth_type(dtype) -> int:
    for t, d in _DEPTH_DTYPES.items():
        if np.dtype(dtype) == d:
            return t
    raise ValueError(f"depth images are uint16 or float32, not {dtype}")


def lib() -> C.CDLL:
    """Load liborbfe.so; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with "
                               "`python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        L.orbfe_create.restype = C.c_void_p
        L.orbfe_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.orbfe_destroy.argtypes = [C.c_void_p]
        L.orbfe_get_scale_factor.restype = C.c_float
        for fn in ("orbfe_get_levels", "orbfe_get_scale_factor", "orbfe_keypoint_capacity",
                   "orbfe_synchronize"):
            getattr(L, fn).argtypes = [C.c_void_p]
        L.orbfe_pyramid_path.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "orbfe_pyramid_tail"):  # an older build selected with ORBFE_LIB has none
            L.orbfe_pyramid_tail.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "orbfe_matcher_create"):
            L.orbfe_matcher_create.restype = C.c_void_p
            L.orbfe_matcher_create.argtypes = [C.c_int, C.c_void_p]
            L.orbfe_matcher_destroy.argtypes = [C.c_void_p]
        if hasattr(L, "orbfe_vocabulary_load_text"):
            L.orbfe_vocabulary_load_text.restype = C.c_void_p
            L.orbfe_vocabulary_load_text.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
            L.orbfe_vocabulary_create.restype = C.c_void_p
            L.orbfe_vocabulary_destroy.argtypes = [C.c_void_p]
        if hasattr(L, "orbfe_kfdb_create"):
            vp, i, u64, f = C.c_void_p, C.c_int, C.c_uint64, C.c_float
            L.orbfe_vocabulary_set_arithmetic.argtypes = [vp, i]
            L.orbfe_vocabulary_score.argtypes = [vp, vp, vp, i, vp, vp, i, vp]
            L.orbfe_vocabulary_score_batch_device.argtypes = [vp, i, vp, vp, i, vp, vp, vp, vp]
            L.orbfe_kfdb_create.restype = vp
            L.orbfe_kfdb_create.argtypes = [vp, i, i, vp]
            L.orbfe_kfdb_destroy.restype = None
            L.orbfe_kfdb_destroy.argtypes = [vp]
            L.orbfe_kfdb_set_stream.argtypes = [vp, vp]
            L.orbfe_kfdb_size.argtypes = [vp]
            L.orbfe_kfdb_add.argtypes = [vp, vp, vp, i, vp]
            L.orbfe_kfdb_add_device.argtypes = [vp, vp, vp, vp, vp]
            L.orbfe_kfdb_erase.argtypes = [vp, i]
            L.orbfe_kfdb_clear.argtypes = [vp]
            L.orbfe_kfdb_set_covisibility.argtypes = [vp, i, i, vp]
            L.orbfe_kfdb_set_scores.argtypes = [vp, i, f, f]
            L.orbfe_kfdb_get_state.argtypes = [vp, i, vp]
            L.orbfe_kfdb_detect_loop_candidates.argtypes = [vp, u64, vp, vp, i, i, vp, f, vp, i, vp]
            L.orbfe_kfdb_detect_relocalization_candidates.argtypes = [vp, u64, vp, vp, i, vp, i, vp]
            L.orbfe_kfdb_detect_loop_candidates_device.argtypes = [vp, u64, vp, vp, vp, i, vp, f,
                                                                   vp, i, vp]
            L.orbfe_kfdb_detect_relocalization_candidates_device.argtypes = [vp, u64, vp, vp, vp,
                                                                             vp, i, vp]
        if hasattr(L, "orbfe_map_create"):
            vp, i, u64 = C.c_void_p, C.c_int, C.c_uint64
            L.orbfe_map_create.restype = vp
            L.orbfe_map_create.argtypes = [i, i, i, vp]
            L.orbfe_map_destroy.restype = None
            L.orbfe_map_destroy.argtypes = [vp]
            L.orbfe_map_set_stream.argtypes = [vp, vp]
            L.orbfe_map_clear.argtypes = [vp]
            L.orbfe_map_size.argtypes = [vp, vp, vp]
            L.orbfe_map_add_keyframe.argtypes = [vp, u64, i, vp, vp]
            L.orbfe_map_set_keyframe_points.argtypes = [vp, i, i, i, vp]
            L.orbfe_map_set_keyframe_bad.argtypes = [vp, i, i]
            L.orbfe_map_set_covisibility.argtypes = [vp, i, i, vp]
            L.orbfe_map_set_children.argtypes = [vp, i, i, vp]
            L.orbfe_map_set_parent.argtypes = [vp, i, i]
            L.orbfe_map_add_points.argtypes = [vp, i, vp]
            L.orbfe_map_set_points_bad.argtypes = [vp, i, vp, i]
            L.orbfe_map_add_observations.argtypes = [vp, i, vp, vp]
            L.orbfe_map_erase_observations.argtypes = [vp, i, vp, vp]
            L.orbfe_map_set_stamps.argtypes = [vp, i, i, vp, vp]
            L.orbfe_map_get_stamps.argtypes = [vp, i, i, vp, vp]
            L.orbfe_map_set_local_keyframes.argtypes = [vp, i, vp, i]
            L.orbfe_map_get_local_keyframes.argtypes = [vp, vp, i, vp, vp]
            L.orbfe_map_update_local.argtypes = [vp, u64, i, vp, vp, i, vp, vp, vp, i, vp]
            L.orbfe_map_update_local_device.argtypes = [vp, u64, i, vp, vp, i, vp, vp, vp]
            L.orbfe_map_local_points_device.argtypes = [vp, vp, vp]
            L.orbfe_map_get_local_points.argtypes = [vp, vp, i, vp]
            L.orbfe_map_gather_points_device.argtypes = [vp, i, vp, vp, vp]
        if hasattr(L, "orbfe_map_update_connections"):
            vp, i = C.c_void_p, C.c_int
            L.orbfe_map_update_connections.argtypes = [vp, i, vp, vp, vp, vp]
            L.orbfe_map_add_connection.argtypes = [vp, i, i, i]
            L.orbfe_map_erase_connection.argtypes = [vp, i, i]
            L.orbfe_map_update_best_covisibles.argtypes = [vp, i]
            L.orbfe_map_erase_keyframe_connections.argtypes = [vp, i]
            L.orbfe_map_set_connections.argtypes = [vp, i, i, vp, vp]
            L.orbfe_map_set_ordered_connections.argtypes = [vp, i, i, vp, vp]
            L.orbfe_map_set_first_connection.argtypes = [vp, i, i]
            L.orbfe_map_get_connections.argtypes = [vp, i, vp, vp, i, vp]
            L.orbfe_map_get_ordered_connections.argtypes = [vp, i, vp, vp, i, vp]
            L.orbfe_map_get_spanning_tree.argtypes = [vp, i, vp, vp, vp, i, vp]
        if hasattr(L, "orbfe_map_cull_points"):
            vp, i, f = C.c_void_p, C.c_int, C.c_float
            L.orbfe_map_set_keyframe_features.argtypes = [vp, i, i, vp, vp, vp, f]
            L.orbfe_map_get_keyframe_features.argtypes = [vp, i, i, vp, vp, vp, vp, vp]
            L.orbfe_map_add_observations_idx.argtypes = [vp, i, vp, vp, vp]
            L.orbfe_map_erase_observation.argtypes = [vp, i, i, vp]
            L.orbfe_map_set_point_bad_flag.argtypes = [vp, i, vp]
            L.orbfe_map_set_point_counters.argtypes = [vp, i, vp, vp, vp, vp, vp]
            L.orbfe_map_get_point_counters.argtypes = [vp, i, vp, vp, vp, vp, vp]
            L.orbfe_map_increase_counters.argtypes = [vp, i, i, vp, vp]
            L.orbfe_map_increase_counters_device.argtypes = [vp, i, i, vp, vp]
            L.orbfe_map_cull_points.argtypes = [vp, C.c_int64, i, vp, i, vp, vp, vp]
            L.orbfe_map_tracked_map_points.argtypes = [vp, i, i, vp]
            L.orbfe_map_get_keyframe_points.argtypes = [vp, i, vp, i, vp]
            L.orbfe_map_get_observations.argtypes = [vp, i, vp, vp, i, vp]
            L.orbfe_map_get_bad_flags.argtypes = [vp, i, i, vp, vp]
            L.orbfe_map_set_not_erase.argtypes = [vp, i, i]
            L.orbfe_map_get_erase_flags.argtypes = [vp, i, vp, vp]
            L.orbfe_map_set_keyframe_bad_flag.argtypes = [vp, i, i, vp, vp, i, vp, vp, i, vp]
            L.orbfe_map_set_erase.argtypes = [vp, i, i, i, vp, vp, i, vp, vp, i, vp]
            L.orbfe_map_cull_keyframes.argtypes = [vp, i, i, vp, i, i, vp, i, vp, vp, i, vp, vp, i, vp]
        if hasattr(L, "orbfe_map_refresh_points"):
            vp, i = C.c_void_p, C.c_int
            L.orbfe_map_set_scale_factors.argtypes = [vp, i, vp]
            L.orbfe_map_get_scale_factors.argtypes = [vp, vp, i, vp]
            L.orbfe_map_set_keyframe_centers.argtypes = [vp, i, vp, vp]
            L.orbfe_map_get_keyframe_centers.argtypes = [vp, i, vp, vp]
            L.orbfe_map_set_keyframe_descriptors.argtypes = [vp, i, i, vp]
            L.orbfe_map_set_keyframe_descriptors_device.argtypes = [vp, i, i, vp]
            L.orbfe_map_get_keyframe_descriptors.argtypes = [vp, i, i, vp, vp, vp]
            L.orbfe_map_set_point_ref_keyframes.argtypes = [vp, i, vp, vp]
            L.orbfe_map_get_point_ref_keyframes.argtypes = [vp, i, vp, vp]
            L.orbfe_map_refresh_points.argtypes = [vp, i, i, vp, vp, vp]
            L.orbfe_map_refresh_points_device.argtypes = [vp, i, i, vp, vp, vp]
            L.orbfe_map_refresh_keyframe_points.argtypes = [vp, i, i, vp, vp]
            L.orbfe_map_process_new_keyframe.argtypes = [vp, i, vp, vp, i, vp]
        if hasattr(L, "orbfe_archive_mat_bytes"):
            L.orbfe_archive_mat_bytes.restype = C.c_int64
            sz, vp, i = C.c_size_t, C.c_void_p, C.c_int
            L.orbfe_archive_write_keypoints_device.argtypes = [i, vp, sz, vp, i, vp, sz, vp]
            L.orbfe_archive_read_keypoints_device.argtypes = [i, vp, sz, vp, i, vp, sz, vp]
            L.orbfe_archive_write_descriptors_device.argtypes = [i, vp, sz, vp, i, i, vp, sz, vp, vp]
            L.orbfe_archive_read_descriptors_device.argtypes = [i, vp, sz, i, vp, sz, vp, vp, vp]
        if hasattr(L, "orbfe_close_points"):
            sz, vp, i, f = C.c_size_t, C.c_void_p, C.c_int, C.c_float
            L.orbfe_compute_stereo_from_rgbd.argtypes = [vp, vp, i, i, i, sz, f, vp, vp, i, f, vp, vp]
            L.orbfe_depth_buffer.argtypes = [vp, i, i, i, vp, vp]
            L.orbfe_compute_stereo_from_rgbd_device.argtypes = [vp, i, vp, i, i, i, sz, sz, f, vp,
                                                                vp, vp, i, f, vp, vp]
            L.orbfe_rgbd_status.argtypes = [vp]
            L.orbfe_close_points.argtypes = [vp, i, vp, vp, vp, i, vp, vp, f, i, vp, i, vp, vp, vp,
                                             vp, vp, vp, vp, vp]
            L.orbfe_close_points_batch_device.argtypes = [vp, i, i, vp, vp, vp, vp, i, vp, vp, f, i,
                                                          vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


# hipStreamLegacy (hip_runtime_api.h): the device's legacy default stream as an explicit handle
HIP_STREAM_LEGACY = 1


def _stream_arg(stream_handle: int | None):
    """set_stream's argument: None = the handle's own stream; 0 (torch's default stream, the
    legacy null stream) = hipStreamLegacy, since a NULL hip_stream selects the handle's own
    stream in the C ABI; anything else is a hipStream_t as is."""
    if stream_handle is None:
        return None
    return C.c_void_p(HIP_STREAM_LEGACY if stream_handle == 0 else stream_handle)


def _check_results(fn: str, st: int, results):
    """_check for the calls that write valid results next to ORBFE_ERR_UNSUPPORTED (a predicted
    level outside the pyramid skips that point only): the error carries them as ``.results``."""
    if st != ORBFE_OK:
        e = OrbfeError(fn, st)
        e.results = results() if st == ORBFE_ERR_UNSUPPORTED else None
        raise e
    return results()


def _check(fn: str, st: int) -> None:
    if st != ORBFE_OK:
        raise OrbfeError(fn, st)


def reference_constants() -> dict:
    """The reference's compile-time constants as the HIP library uses them
    (orbfe_get_reference_constants: ORBextractor.cc:71-73, ORBmatcher.cc:37-39); no device."""
    out = (C.c_int32 * 6)()
    _check("orbfe_get_reference_constants", lib().orbfe_get_reference_constants(out))
    return dict(zip(("PATCH_SIZE", "HALF_PATCH_SIZE", "EDGE_THRESHOLD", "TH_HIGH", "TH_LOW",
                     "HISTO_LENGTH"), list(out)))


def keypoint_capacity(nfeatures: int, scaleFactor: float, nlevels: int, iniThFAST: int,
                      minThFAST: int, w: int, h: int) -> int:
    """Per-frame keypoint capacity at w x h for these extractor parameters, without a handle or
    a device (orbfe_keypoint_capacity_params): the slab rows an extraction can fill."""
    p = Params(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
    c = lib().orbfe_keypoint_capacity_params(C.byref(p), int(w), int(h))
    _check("orbfe_keypoint_capacity_params", min(c, 0))
    return c


def describe_blur_fragments(nfeatures: int, scaleFactor: float, nlevels: int, iniThFAST: int,
                            minThFAST: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Describe's matrix-core window blur as the host builds it, without a device
    (orbfe_describe_blur_fragments): the 7 taps, the fragments as int8 [6, 64, 16] (H_0..H_2,
    V_0..V_2; lane; byte) and the spare K slots' constant bytes as int8 [2, 2, 4]
    (plane hi / lo; reading scalar / x86; byte i <-> slot j = 12 + i)."""
    p = Params(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
    taps = np.zeros(7, np.int32)
    frags = np.zeros(384 * 16, np.uint8)
    pads = np.zeros(4, np.uint32)
    _check("orbfe_describe_blur_fragments",
           lib().orbfe_describe_blur_fragments(C.byref(p), ptr(taps), ptr(frags), ptr(pads)))
    return taps, frags.view(np.int8).reshape(6, 64, 16), pads.view(np.int8).reshape(2, 2, 4)


# ORBFE_PIX_* (include/orbfe.h): the cvtColor codes of Tracking::GrabImage*
PIX_GRAY, PIX_RGB, PIX_BGR, PIX_RGBA, PIX_BGRA = range(5)
PIX_CHANNELS = {PIX_GRAY: 1, PIX_RGB: 3, PIX_BGR: 3, PIX_RGBA: 4, PIX_BGRA: 4}


def human_mask_rect(joints: np.ndarray, w: int, h: int) -> tuple[int, int, int, int]:
    """OpDetector::SkeletonSquareMask's zeroed rectangle from (n, 3) joints
    (DetectHumanPose.cpp:453-489), via orbfe_human_mask_rect."""
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, 3)
    out = (C.c_int32 * 4)()
    _check("orbfe_human_mask_rect", lib().orbfe_human_mask_rect(ptr(j), len(j), w, h, out))
    return tuple(out)


class ORBextractor:
    """``ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)`` on a gfx950 GPU
    (ORBextractor.cc:409-469).  One instance is not reentrant; use one per thread."""

    def __init__(self, nfeatures: int, scaleFactor: float, nlevels: int, iniThFAST: int,
                 minThFAST: int, device: int = 0, max_width: int = 0, max_height: int = 0,
                 max_batch: int = 1):
        self._p = Params(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
        st = C.c_int(0)
        h = lib().orbfe_create(C.byref(self._p), device, max_width, max_height, max_batch,
                               C.byref(st))
        if not h:
            raise OrbfeError("orbfe_create", st.value)
        self._h = C.c_void_p(h)
        self.nlevels = nlevels

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().orbfe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- getters (ORBextractor.h:68-88)
    def GetLevels(self) -> int:
        return lib().orbfe_get_levels(self._h)

    def GetScaleFactor(self) -> float:
        return lib().orbfe_get_scale_factor(self._h)

    def _tables(self):
        t = [np.zeros(self.nlevels, np.float32) for _ in range(4)]
        _check("orbfe_get_scale_tables", lib().orbfe_get_scale_tables(self._h, *map(ptr, t)))
        return t

    def GetScaleFactors(self) -> np.ndarray:
        return self._tables()[0]

    def GetInverseScaleFactors(self) -> np.ndarray:
        return self._tables()[1]

    def GetScaleSigmaSquares(self) -> np.ndarray:
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self) -> np.ndarray:
        return self._tables()[3]

    def features_per_level(self) -> np.ndarray:
        out = np.zeros(self.nlevels, np.int32)
        _check("orbfe_get_features_per_level", lib().orbfe_get_features_per_level(self._h, ptr(out)))
        return out

    ARITH_SCALAR, ARITH_X86_SIMD = 0, 1

    def set_arithmetic(self, mode: int) -> None:
        """orbfe_set_arithmetic: ARITH_X86_SIMD (the default: the SSE2 resize / blur bodies and
        FMA-contracted rotation of the reference's x86-64 build) or ARITH_SCALAR (OpenCV's
        portable scalar paths)."""
        _check("orbfe_set_arithmetic", lib().orbfe_set_arithmetic(self._h, int(mode)))

    def capacity(self, w: int | None = None, h: int | None = None) -> int:
        """Keypoints per frame that can never overflow: for a w x h input when given
        (orbfe_keypoint_capacity_for), else for every supported size."""
        if w is None or h is None:
            return lib().orbfe_keypoint_capacity(self._h)
        c = lib().orbfe_keypoint_capacity_for(self._h, int(w), int(h))
        _check("orbfe_keypoint_capacity_for", min(c, 0))
        return c

    # ---- operator() (ORBextractor.cc:1042-1108)
    def __call__(self, image: np.ndarray, mask: np.ndarray | None = None):
        """Returns (keypoints[KEYPOINT_DTYPE], descriptors uint8 (n, 32)); an empty image
        returns (None, None) like the reference, which leaves its outputs untouched."""
        image = np.asarray(image)
        if image.size == 0:
            return None, None
        # a row-strided u8 view (a cv::Mat ROI: step > cols) is passed as is, with its stride
        if not (image.dtype == np.uint8 and image.ndim == 2 and image.strides[1] == 1 and
                image.strides[0] >= image.shape[1]):
            image = np.ascontiguousarray(image, np.uint8)
        h, w = image.shape
        stride = image.strides[0]
        m = None if mask is None or np.size(mask) == 0 else np.ascontiguousarray(mask, np.uint8)
        cap = self.capacity(w, h)
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        _check("orbfe_extract", lib().orbfe_extract(
            self._h, C.c_void_p(image.ctypes.data), w, h, C.c_size_t(stride), ptr(m),
            C.c_size_t(w), ptr(kps), cap, ptr(desc), C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def input_buffer(self, w: int, h: int) -> np.ndarray:
        """The handle's pinned staging buffer as a writable (h, w) uint8 view
        (orbfe_input_buffer): write the gray frame into it (as GrabImageMonocular's cvtColor
        would), then call :meth:`extract_staged`."""
        buf = C.POINTER(C.c_uint8)()
        stride = C.c_size_t(0)
        _check("orbfe_input_buffer", lib().orbfe_input_buffer(self._h, w, h, C.byref(buf),
                                                              C.byref(stride)))
        flat = np.ctypeslib.as_array(buf, shape=(h * stride.value,))
        return np.lib.stride_tricks.as_strided(flat, (h, w), (stride.value, 1))

    def extract_staged(self, w: int, h: int, copy_out: bool = True):
        """operator() on the staged frame (orbfe_extract_staged).  copy_out=False leaves the
        outputs in the handle's pinned buffers (kps_cap 0) and returns views of them
        (orbfe_staged_outputs), valid until the next call."""
        n = C.c_int(0)
        if copy_out:
            cap = self.capacity(w, h)
            kps = np.zeros(cap, KEYPOINT_DTYPE)
            desc = np.zeros((cap, 32), np.uint8)
            _check("orbfe_extract_staged", lib().orbfe_extract_staged(
                self._h, w, h, ptr(kps), cap, ptr(desc), C.byref(n)))
            return kps[:n.value].copy(), desc[:n.value].copy()
        _check("orbfe_extract_staged", lib().orbfe_extract_staged(self._h, w, h, None, 0, None,
                                                                  C.byref(n)))
        return self.staged_outputs()

    def staged_outputs(self):
        """Views of the last single-frame call's outputs in handle-owned memory."""
        k = C.c_void_p()
        d = C.c_void_p()
        n = C.c_int(0)
        _check("orbfe_staged_outputs", lib().orbfe_staged_outputs(self._h, C.byref(k), C.byref(d),
                                                                  C.byref(n)))
        if not k.value or n.value == 0:
            return np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
        kb = (C.c_uint8 * (n.value * KEYPOINT_DTYPE.itemsize)).from_address(k.value)
        db = (C.c_uint8 * (n.value * 32)).from_address(d.value)
        return (np.frombuffer(kb, KEYPOINT_DTYPE, n.value),
                np.frombuffer(db, np.uint8).reshape(n.value, 32))

    def extract_color(self, image: np.ndarray, pix: int, mask: np.ndarray | None = None,
                      rect: tuple[int, int, int, int] | None = None):
        """``cvtColor(image, gray, CV_*2GRAY)`` (Tracking.cc:409-422) fused with
        ``operator()(gray, mask)``; `pix` is one of PIX_*; `rect` = (x0, y0, x1, y1) zeroed
        rectangle of the human mask (DetectHumanPose.cpp:484-489)."""
        image = np.ascontiguousarray(image, np.uint8)
        if image.size == 0:
            return None, None
        h, w = image.shape[:2]
        cn = 1 if image.ndim == 2 else image.shape[2]
        if cn != PIX_CHANNELS[pix]:
            raise ValueError(f"pix {pix} needs {PIX_CHANNELS[pix]} channels, image has {cn}")
        m = None if mask is None or np.size(mask) == 0 else np.ascontiguousarray(mask, np.uint8)
        r = None if rect is None else (C.c_int32 * 4)(*rect)
        cap = self.capacity(w, h)
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        _check("orbfe_extract_color", lib().orbfe_extract_color(
            self._h, ptr(image), pix, w, h, C.c_size_t(w * cn), ptr(m), C.c_size_t(w),
            r, ptr(kps), cap, ptr(desc), C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_color_batch_device(self, d_imgs: int, pix: int, n: int, w: int, h: int,
                                   stride: int, frame_pitch: int, d_kps: int, kps_cap: int,
                                   d_desc: int, d_n_out: int, d_masks: int | None = None,
                                   mask_stride: int = 0, mask_frame_pitch: int = 0,
                                   d_rects: int | None = None) -> None:
        """Device-resident colour batch (orbfe_extract_color_batch_device); async."""
        _check("orbfe_extract_color_batch_device", lib().orbfe_extract_color_batch_device(
            self._h, C.c_void_p(d_imgs), pix, n, w, h, C.c_size_t(stride),
            C.c_size_t(frame_pitch), C.c_void_p(d_masks) if d_masks else None,
            C.c_size_t(mask_stride), C.c_size_t(mask_frame_pitch),
            C.c_void_p(d_rects) if d_rects else None, C.c_void_p(d_kps), kps_cap,
            C.c_void_p(d_desc), C.c_void_p(d_n_out)))

    def ComputeStereoMatches(self, right: "ORBextractor", kl: np.ndarray, dl: np.ndarray,
                             kr: np.ndarray, dr: np.ndarray, bf: float, b: float,
                             frame: int = 0):
        """Frame::ComputeStereoMatches (Frame.cc:584-756) with this handle as
        mpORBextractorLeft and `right` as mpORBextractorRight (their last extractions' pyramids).
        Returns (mvuRight, mvDepth) float32 arrays of len(kl)."""
        kl = np.ascontiguousarray(kl, KEYPOINT_DTYPE)
        kr = np.ascontiguousarray(kr, KEYPOINT_DTYPE)
        dl = np.ascontiguousarray(dl, np.uint8)
        dr = np.ascontiguousarray(dr, np.uint8)
        ur = np.full(len(kl), -1, np.float32)
        dp = np.full(len(kl), -1, np.float32)
        _check("orbfe_compute_stereo_matches", lib().orbfe_compute_stereo_matches(
            self._h, right._h, frame, ptr(kl), ptr(dl), len(kl), ptr(kr), ptr(dr), len(kr),
            C.c_float(bf), C.c_float(b), ptr(ur), ptr(dp)))
        return ur, dp

    def compute_stereo_matches_device(self, right: "ORBextractor", n: int, d_kl: int, d_dl: int,
                                      d_nl: int, d_kr: int, d_dr: int, d_nr: int, kps_cap: int,
                                      bf: float, b: float, d_ur: int, d_dp: int) -> None:
        """Batched device form (orbfe_compute_stereo_matches_device); async."""
        _check("orbfe_compute_stereo_matches_device", lib().orbfe_compute_stereo_matches_device(
            self._h, right._h, n, C.c_void_p(d_kl), C.c_void_p(d_dl), C.c_void_p(d_nl),
            C.c_void_p(d_kr), C.c_void_p(d_dr), C.c_void_p(d_nr), kps_cap, C.c_float(bf),
            C.c_float(b), C.c_void_p(d_ur), C.c_void_p(d_dp)))

    def stereo_status(self) -> None:
        _check("orbfe_stereo_status", lib().orbfe_stereo_status(self._h))

    def depth_buffer(self, w: int, h: int, dtype=np.uint16) -> np.ndarray:
        """The handle's pinned depth buffer as a writable (h, w) view of `dtype` (uint16 or
        float32; orbfe_depth_buffer): the grabber writes the raw depth image into it and
        :meth:`ComputeStereoFromRGBD`, given this array, gathers from it in place."""
        t = _depth_type(dtype)
        buf = C.c_void_p()
        stride = C.c_size_t(0)
        _check("orbfe_depth_buffer", lib().orbfe_depth_buffer(self._h, w, h, t, C.byref(buf),
                                                              C.byref(stride)))
        raw = (C.c_uint8 * (h * stride.value)).from_address(buf.value)
        return np.frombuffer(raw, _DEPTH_DTYPES[t]).reshape(h, -1)[:, :w]

    def ComputeStereoFromRGBD(self, imDepth: np.ndarray, depth_factor: float, keys: np.ndarray,
                              bf: float, keys_un: np.ndarray | None = None, results: bool = False):
        """Frame::ComputeStereoFromRGBD (Frame.cc:759-780) on the raw depth image (uint16 or
        float32, rows may be padded) with ``convertTo(CV_32F, depth_factor)`` (Tracking.cc:368)
        fused.  keys = mvKeys, keys_un = mvKeysUn (None: the same).  Returns (mvuRight, mvDepth);
        with results=True an out-of-image keypoint does not raise and the status comes third."""
        t = _depth_type(imDepth.dtype)
        assert imDepth.ndim == 2 and imDepth.strides[1] == imDepth.itemsize and imDepth.strides[0] > 0
        h, w = imDepth.shape
        keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
        ku = None if keys_un is None else np.ascontiguousarray(keys_un, KEYPOINT_DTYPE)
        assert ku is None or len(ku) == len(keys)
        ur = np.full(len(keys), -1, np.float32)
        dp = np.full(len(keys), -1, np.float32)
        st = lib().orbfe_compute_stereo_from_rgbd(
            self._h, imDepth.ctypes.data, t, w, h, imDepth.strides[0], depth_factor, ptr(keys),
            ptr(ku), len(keys), bf, ptr(ur), ptr(dp))
        if results and st in (ORBFE_OK, ORBFE_ERR_UNSUPPORTED):
            return ur, dp, st
        _check("orbfe_compute_stereo_from_rgbd", st)
        return ur, dp

    def compute_stereo_from_rgbd_device(self, n_frames: int, d_depth: int, depth_type: int, w: int,
                                        h: int, stride: int, frame_pitch: int,
                                        depth_factor: float, d_keys: int, d_n: int, kps_cap: int,
                                        bf: float, d_ur: int, d_dp: int,
                                        d_keys_un: int | None = None) -> None:
        """Batched device form (orbfe_compute_stereo_from_rgbd_device) over the slabs
        :meth:`extract_batch_device` writes; async, :meth:`rgbd_status` reports afterwards."""
        _check("orbfe_compute_stereo_from_rgbd_device", lib().orbfe_compute_stereo_from_rgbd_device(
            self._h, n_frames, d_depth, depth_type, w, h, stride, frame_pitch, depth_factor,
            d_keys, d_keys_un, d_n, kps_cap, bf, d_ur, d_dp))

    def rgbd_status(self) -> None:
        _check("orbfe_rgbd_status", lib().orbfe_rgbd_status(self._h))

    def extract_batch(self, images: np.ndarray, masks: np.ndarray | None = None):
        """Host batch: (n, h, w) uint8 -> (kps (n, cap), desc (n, cap, 32), counts (n,))."""
        images = np.ascontiguousarray(images, np.uint8)
        n, h, w = images.shape
        cap = self.capacity(w, h)
        kps = np.zeros((n, cap), KEYPOINT_DTYPE)
        desc = np.zeros((n, cap, 32), np.uint8)
        cnt = np.zeros(n, np.int32)
        arr = (C.c_void_p * n)(*[images[i].ctypes.data for i in range(n)])
        marr = None
        if masks is not None:
            masks = np.ascontiguousarray(masks, np.uint8)
            marr = (C.c_void_p * n)(*[masks[i].ctypes.data for i in range(n)])
        _check("orbfe_extract_batch", lib().orbfe_extract_batch(
            self._h, arr, n, w, h, C.c_size_t(w), marr, C.c_size_t(w), ptr(kps), cap, ptr(desc),
            ptr(cnt)))
        return kps, desc, cnt

    def extract_batch_device(self, d_imgs: int, n: int, w: int, h: int, stride: int,
                             frame_pitch: int, d_kps: int, kps_cap: int, d_desc: int,
                             d_n_out: int, d_masks: int | None = None) -> None:
        """Device-resident batch (raw device pointers, e.g. torch ``data_ptr()``); async."""
        _check("orbfe_extract_batch_device", lib().orbfe_extract_batch_device(
            self._h, C.c_void_p(d_imgs), n, w, h, C.c_size_t(stride), C.c_size_t(frame_pitch),
            C.c_void_p(d_masks) if d_masks else None, C.c_void_p(d_kps), kps_cap,
            C.c_void_p(d_desc), C.c_void_p(d_n_out)))

    def set_stream(self, stream_handle: int | None) -> None:
        _check("orbfe_set_stream", lib().orbfe_set_stream(
            self._h, _stream_arg(stream_handle)))

    def synchronize(self) -> None:
        _check("orbfe_synchronize", lib().orbfe_synchronize(self._h))

    STAGES = ("mask", "resize", "fast", "octree", "blur", "describe")

    def profile(self, enable: bool, stages=None) -> None:
        """Record a HIP event pair around every kernel launch (orbfe_profile), or only around
        the launches of the named stages (e.g. ("fast",))."""
        mode = int(bool(enable))
        if enable and stages is not None:
            mode = 0
            for st in stages:
                mode |= 2 << self.STAGES.index(st)
        _check("orbfe_profile", lib().orbfe_profile(self._h, mode))

    def set_stages(self, stages=None) -> None:
        """orbfe_set_stage_mask: later extraction calls run only the named stages (None: all)."""
        mask = 0
        for st in stages or ():
            mask |= 1 << self.STAGES.index(st)
        _check("orbfe_set_stage_mask", lib().orbfe_set_stage_mask(self._h, C.c_uint(mask)))

    def replay(self, stages, reps: int = 1) -> None:
        """orbfe_debug_replay: relaunch the named stages of the last extraction reps times."""
        mask = 0
        for st in stages:
            mask |= 1 << self.STAGES.index(st)
        _check("orbfe_debug_replay", lib().orbfe_debug_replay(self._h, C.c_uint(mask), int(reps)))

    def profile_read(self) -> dict:
        """{stage: (total_ms, launches)} since the previous read (orbfe_profile_read)."""
        ms = np.zeros(len(self.STAGES), np.float64)
        n = np.zeros(len(self.STAGES), np.int32)
        _check("orbfe_profile_read", lib().orbfe_profile_read(self._h, ptr(ms), ptr(n)))
        return {s: (float(ms[i]), int(n[i])) for i, s in enumerate(self.STAGES)}

    PYR_PATHS = ("per_level", "bands")

    def pyramid_path(self, nframes: int) -> str:
        """The pyramid kernel an extraction of `nframes` frames at the last extracted size takes
        (orbfe_pyramid_path): "per_level" or "bands"."""
        r = lib().orbfe_pyramid_path(self._h, int(nframes))
        _check("orbfe_pyramid_path", r if r < 0 else 0)
        return self.PYR_PATHS[r]

    PYR_TAILS = ("none", "gather", "table")

    def pyramid_tail(self, nframes: int) -> str:
        """How that extraction makes the small top levels (orbfe_pyramid_tail): "none" (no
        resize_tail_kernel launch), "gather" (byte gathers) or "table" (column-group tables)."""
        r = lib().orbfe_pyramid_tail(self._h, int(nframes))
        _check("orbfe_pyramid_tail", r if r < 0 else 0)
        return self.PYR_TAILS[r]

    # ---- probes of the last extraction
    def _level(self, fn, frame: int, level: int) -> np.ndarray:
        w, h = C.c_int(0), C.c_int(0)
        _check(fn.__name__, fn(self._h, frame, level, None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _check(fn.__name__, fn(self._h, frame, level, ptr(out), C.byref(w), C.byref(h)))
        return out

    def get_level(self, level: int, frame: int = 0) -> np.ndarray:
        """mvImagePyramid[level] of the last extraction (ORBextractor.h:90)."""
        return self._level(lib().orbfe_get_level, frame, level)

    @property
    def mvImagePyramid(self) -> list[np.ndarray]:
        return [self.get_level(l) for l in range(self.nlevels)]

    def get_blurred_level(self, level: int, frame: int = 0) -> np.ndarray:
        return self._level(lib().orbfe_get_blurred_level, frame, level)

    def get_fast_keys(self, level: int, frame: int = 0) -> np.ndarray:
        cap = 65536
        while True:
            out = np.zeros(cap, KEYPOINT_DTYPE)
            n = C.c_int(0)
            st = lib().orbfe_get_fast_keys(self._h, frame, level, ptr(out), cap, C.byref(n))
            if st == ORBFE_ERR_CAPACITY:
                cap = n.value
                continue
            _check("orbfe_get_fast_keys", st)
            return out[:n.value].copy()


def archive_mat_bytes(rows: int, cols: int = 32, elem_size: int = 1) -> int:
    """Bytes of one cv::Mat archive record (MapPoint.h:215-247)."""
    return int(lib().orbfe_archive_mat_bytes(rows, cols, elem_size))


def archive_write_keypoints_device(n_frames: int, d_keys: int, keys_pitch: int, d_n: int,
                                   cap: int, d_out: int, out_pitch: int, stream=None) -> None:
    """Keypoint records (serialize(Archive&, cv::KeyPoint&), MapPoint.h:196-209) from HBM."""
    _check("orbfe_archive_write_keypoints_device", lib().orbfe_archive_write_keypoints_device(
        n_frames, d_keys, keys_pitch, d_n, cap, d_out, out_pitch, stream))


def archive_read_keypoints_device(n_frames: int, d_in: int, in_pitch: int, d_n: int, cap: int,
                                  d_keys: int, keys_pitch: int, stream=None) -> None:
    _check("orbfe_archive_read_keypoints_device", lib().orbfe_archive_read_keypoints_device(
        n_frames, d_in, in_pitch, d_n, cap, d_keys, keys_pitch, stream))


def archive_write_descriptors_device(n_mats: int, d_desc: int, desc_pitch: int, d_rows,
                                     rows_fixed: int, cap: int, d_out: int, out_pitch: int,
                                     d_len=None, stream=None) -> None:
    """rows x 32 CV_8UC1 cv::Mat records (MapPoint.h:215-229) from HBM descriptors."""
    _check("orbfe_archive_write_descriptors_device", lib().orbfe_archive_write_descriptors_device(
        n_mats, d_desc, desc_pitch, d_rows, rows_fixed, cap, d_out, out_pitch, d_len, stream))


def archive_read_descriptors_device(n_mats: int, d_in: int, in_pitch: int, cap: int,
                                    d_desc: int, desc_pitch: int, d_rows, d_status: int,
                                    stream=None) -> None:
    _check("orbfe_archive_read_descriptors_device", lib().orbfe_archive_read_descriptors_device(
        n_mats, d_in, in_pitch, cap, d_desc, desc_pitch, d_rows, d_status, stream))


class Vocabulary:
    """ORBVocabulary (DBoW2 TemplatedVocabulary<FORB>) held in HBM: loadFromTextFile and
    transform (Frame::ComputeBoW)."""

    def __init__(self, path: str, device: int = 0):
        st = C.c_int(0)
        h = lib().orbfe_vocabulary_load_text(path.encode(), device, C.byref(st))
        if not h:
            raise OrbfeError("orbfe_vocabulary_load_text", st.value)
        self._adopt(h)

    def _adopt(self, h: int) -> None:
        self._h = C.c_void_p(h)
        info = np.zeros(6, np.int32)
        _check("orbfe_vocabulary_info", lib().orbfe_vocabulary_info(self._h, ptr(info)))
        self.k, self.L, self.scoring, self.weighting, self.nodes, self.words = map(int, info)

    @classmethod
    def from_arrays(cls, k: int, L: int, scoring: int, weighting: int, parent, is_word, desc,
                    weight, device: int = 0) -> "Vocabulary":
        """The vocabulary from node arrays in insertion order (orbfe_vocabulary_create): node 0
        is the root, parent[i] < i, word ids are handed out to the flagged nodes in order."""
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        n = len(par)
        word = np.ascontiguousarray(is_word, np.uint8).reshape(-1)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        w = np.ascontiguousarray(weight, np.float64).reshape(-1)
        if not (len(word) == len(d) == len(w) == n):
            raise ValueError("from_arrays: parent, is_word, desc and weight must describe the same nodes")
        st = C.c_int(0)
        h = lib().orbfe_vocabulary_create(k, L, scoring, weighting, n, ptr(par), ptr(word), ptr(d),
                                          ptr(w), device, C.byref(st))
        if not h:
            raise OrbfeError("orbfe_vocabulary_create", st.value)
        self = cls.__new__(cls)
        self._adopt(h)
        return self

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().orbfe_vocabulary_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transform(self, desc: np.ndarray, levelsup: int = 4):
        """-> (word_ids, values, node_ids, node_off, feat) = BowVector + FeatureVector."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        cap = max(n, 1)
        wid = np.zeros(cap, np.int32)
        val = np.zeros(cap, np.float64)
        nid = np.zeros(cap, np.int32)
        off = np.zeros(cap + 1, np.int32)
        feat = np.zeros(cap, np.int32)
        nw, nn = C.c_int32(0), C.c_int32(0)
        _check("orbfe_bow_transform", lib().orbfe_bow_transform(
            self._h, ptr(d), n, levelsup, ptr(wid), ptr(val), C.byref(nw), ptr(nid), ptr(off),
            ptr(feat), C.byref(nn)))
        return (wid[:nw.value].copy(), val[:nw.value].copy(), nid[:nn.value].copy(),
                off[:nn.value + 1].copy(), feat[:off[nn.value]].copy())

    def transform_batch_device(self, nframes: int, d_desc: int, d_n: int, cap: int,
                               levelsup: int, d_wid: int, d_val: int, d_nw: int, d_nid: int,
                               d_noff: int, d_feat: int, d_nn: int) -> None:
        _check("orbfe_bow_transform_batch_device", lib().orbfe_bow_transform_batch_device(
            self._h, nframes, C.c_void_p(d_desc), C.c_void_p(d_n), cap, levelsup,
            C.c_void_p(d_wid), C.c_void_p(d_val), C.c_void_p(d_nw), C.c_void_p(d_nid),
            C.c_void_p(d_noff), C.c_void_p(d_feat), C.c_void_p(d_nn)))

    def set_stream(self, stream_handle: int | None) -> None:
        _check("orbfe_vocabulary_set_stream", lib().orbfe_vocabulary_set_stream(
            self._h, _stream_arg(stream_handle)))

    def set_arithmetic(self, mode: int) -> None:
        """ORBFE_ARITH_X86_SIMD (1, default): the L2 / dot-product sums contracted to fma as the
        reference's -march=native build; ORBFE_ARITH_SCALAR (0): uncontracted."""
        _check("orbfe_vocabulary_set_arithmetic",
               lib().orbfe_vocabulary_set_arithmetic(self._h, mode))

    def score(self, ids1, vals1, ids2, vals2) -> float:
        """ORBVocabulary::score(v1, v2) with the vocabulary's scoring (ScoringObject.cpp:23-311)."""
        i1, v1 = np.ascontiguousarray(ids1, np.int32), np.ascontiguousarray(vals1, np.float64)
        i2, v2 = np.ascontiguousarray(ids2, np.int32), np.ascontiguousarray(vals2, np.float64)
        out = C.c_double(0.0)
        _check("orbfe_vocabulary_score", lib().orbfe_vocabulary_score(
            self._h, ptr(i1), ptr(v1), len(i1), ptr(i2), ptr(v2), len(i2), C.byref(out)))
        return out.value

    def score_batch_device(self, n_pairs: int, d_pair_a: int, d_pair_b: int, cap: int,
                           d_wid: int, d_val: int, d_nw: int, d_score: int) -> None:
        _check("orbfe_vocabulary_score_batch_device", lib().orbfe_vocabulary_score_batch_device(
            self._h, n_pairs, C.c_void_p(d_pair_a), C.c_void_p(d_pair_b), cap, C.c_void_p(d_wid),
            C.c_void_p(d_val), C.c_void_p(d_nw), C.c_void_p(d_score)))


class KfdbState(C.Structure):
    """orbfe_kfdb_state: the six fields of KeyFrame.h:166-171 and which scores were written."""
    _fields_ = [("loop_query", C.c_uint64), ("reloc_query", C.c_uint64),
                ("loop_words", C.c_int32), ("reloc_words", C.c_int32),
                ("loop_score", C.c_float), ("reloc_score", C.c_float),
                ("scores_set", C.c_int32), ("reserved", C.c_int32)]


class KeyFrameDatabase:
    """KeyFrameDatabase (KeyFrameDatabase.cc:115-389) over device slots.  Keyframes are named by
    the slot ``add`` returns.  The two queries return ``(candidates, status)``: status is
    ORBFE_OK, or ORBFE_ERR_UNSUPPORTED when the reference would have read a score it never wrote
    (the candidates are then computed with 0.0f); other errors raise."""

    def __init__(self, voc: Vocabulary, cap: int = 4096, slots_hint: int = 0):
        st = C.c_int(0)
        h = lib().orbfe_kfdb_create(voc._h, cap, slots_hint, C.byref(st))
        if not h:
            raise OrbfeError("orbfe_kfdb_create", st.value)
        self._h = C.c_void_p(h)
        self._voc = voc  # the vocabulary must outlive the database
        self.cap = cap

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().orbfe_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return lib().orbfe_kfdb_size(self._h)

    def set_stream(self, stream_handle: int | None) -> None:
        _check("orbfe_kfdb_set_stream", lib().orbfe_kfdb_set_stream(
            self._h, _stream_arg(stream_handle)))

    def add(self, word_ids, values) -> int:
        ids = np.ascontiguousarray(word_ids, np.int32)
        val = np.ascontiguousarray(values, np.float64)
        slot = C.c_int32(-1)
        _check("orbfe_kfdb_add", lib().orbfe_kfdb_add(self._h, ptr(ids), ptr(val), len(ids),
                                                      C.byref(slot)))
        return slot.value

    def add_device(self, d_wid: int, d_val: int, d_nw: int) -> int:
        slot = C.c_int32(-1)
        _check("orbfe_kfdb_add_device", lib().orbfe_kfdb_add_device(
            self._h, C.c_void_p(d_wid), C.c_void_p(d_val), C.c_void_p(d_nw), C.byref(slot)))
        return slot.value

    def erase(self, slot: int) -> None:
        _check("orbfe_kfdb_erase", lib().orbfe_kfdb_erase(self._h, slot))

    def clear(self) -> None:
        _check("orbfe_kfdb_clear", lib().orbfe_kfdb_clear(self._h))

    def set_covisibility(self, slot: int, neigh_slots) -> None:
        n = np.ascontiguousarray(neigh_slots, np.int32)
        _check("orbfe_kfdb_set_covisibility", lib().orbfe_kfdb_set_covisibility(
            self._h, slot, len(n), ptr(n)))

    def set_scores(self, slot: int, loop_score: float, reloc_score: float) -> None:
        _check("orbfe_kfdb_set_scores", lib().orbfe_kfdb_set_scores(
            self._h, slot, loop_score, reloc_score))

    def get_state(self, slot: int) -> KfdbState:
        s = KfdbState()
        _check("orbfe_kfdb_get_state", lib().orbfe_kfdb_get_state(self._h, slot, C.byref(s)))
        return s

    @staticmethod
    def _result(fn: str, st: int, cand: np.ndarray, n: int):
        if st not in (ORBFE_OK, ORBFE_ERR_UNSUPPORTED):
            raise OrbfeError(fn, st)
        return cand[:n].copy(), st

    def DetectLoopCandidates(self, query_id: int, word_ids, values, conn_slots, min_score: float,
                             cand_cap: int = 4096):
        ids = np.ascontiguousarray(word_ids, np.int32)
        val = np.ascontiguousarray(values, np.float64)
        conn = np.ascontiguousarray(conn_slots, np.int32)
        cand = np.zeros(max(cand_cap, 1), np.int32)
        n = C.c_int32(0)
        st = lib().orbfe_kfdb_detect_loop_candidates(
            self._h, query_id, ptr(ids), ptr(val), len(ids), len(conn), ptr(conn), min_score,
            ptr(cand), cand_cap, C.byref(n))
        return self._result("orbfe_kfdb_detect_loop_candidates", st, cand, n.value)

    def DetectRelocalizationCandidates(self, frame_id: int, word_ids, values,
                                       cand_cap: int = 4096):
        ids = np.ascontiguousarray(word_ids, np.int32)
        val = np.ascontiguousarray(values, np.float64)
        cand = np.zeros(max(cand_cap, 1), np.int32)
        n = C.c_int32(0)
        st = lib().orbfe_kfdb_detect_relocalization_candidates(
            self._h, frame_id, ptr(ids), ptr(val), len(ids), ptr(cand), cand_cap, C.byref(n))
        return self._result("orbfe_kfdb_detect_relocalization_candidates", st, cand, n.value)

    def detect_loop_candidates_device(self, query_id: int, d_wid: int, d_val: int, d_nw: int,
                                      n_conn: int, d_conn: int, min_score: float, d_cand: int,
                                      cand_cap: int):
        """-> (n_cand, status); the candidates stay in d_cand."""
        n = C.c_int32(0)
        st = lib().orbfe_kfdb_detect_loop_candidates_device(
            self._h, query_id, C.c_void_p(d_wid), C.c_void_p(d_val), C.c_void_p(d_nw), n_conn,
            C.c_void_p(d_conn), min_score, C.c_void_p(d_cand), cand_cap, C.byref(n))
        if st not in (ORBFE_OK, ORBFE_ERR_UNSUPPORTED):
            raise OrbfeError("orbfe_kfdb_detect_loop_candidates_device", st)
        return n.value, st

    def detect_relocalization_candidates_device(self, frame_id: int, d_wid: int, d_val: int,
                                                d_nw: int, d_cand: int, cand_cap: int):
        n = C.c_int32(0)
        st = lib().orbfe_kfdb_detect_relocalization_candidates_device(
            self._h, frame_id, C.c_void_p(d_wid), C.c_void_p(d_val), C.c_void_p(d_nw),
            C.c_void_p(d_cand), cand_cap, C.byref(n))
        if st not in (ORBFE_OK, ORBFE_ERR_UNSUPPORTED):
            raise OrbfeError("orbfe_kfdb_detect_relocalization_candidates_device", st)
        return n.value, st


class MapPointArrays(C.Structure):
    """orbfe_map_point_arrays: device pointers of map-point data (map-wide or gathered)."""
    _fields_ = [(k, C.c_void_p) for k in ("xyz", "normal", "min_dist", "max_dist", "desc", "n_obs",
                                          "skip", "mp_ids", "bad")]


MAP_KEYFRAMES, MAP_POINTS = 0, 1       # ORBFE_MAP_KEYFRAMES / ORBFE_MAP_POINTS
MAP_MAX_VOTED, MAP_MAX_KF_SLOTS = 4096, 8192
MAP_FOUND, MAP_VISIBLE = 0, 1          # ORBFE_MAP_FOUND / ORBFE_MAP_VISIBLE
MAP_BAD_NOTHING, MAP_BAD_DEFERRED, MAP_BAD_DONE = 0, 1, 2      # ORBFE_MAP_BAD_*
MAP_CULL_KEPT, MAP_CULL_CULLED, MAP_CULL_DEFERRED = 0, 1, 2    # ORBFE_MAP_CULL_*
MAP_MAX_CULL_LIST = 4096
MAP_REFRESH_NORMAL_DEPTH, MAP_REFRESH_DESCRIPTOR, MAP_REFRESH_UNSUPPORTED = 1, 2, 4  # ORBFE_MAP_REFRESH_*
MAP_MAX_REFRESH_OBS = 1024


class LocalMap:
    """Tracking::UpdateLocalMap (Tracking.cc:1455-1599) over a device mirror of the map graph
    (orbfe_map).  Keyframes and points are named by the slots ``add_keyframe`` / ``add_points``
    return.  The mutators carry the names of the reference methods they shadow; ``UpdateLocalMap``
    returns ``(mvpLocalKeyFrames, mpReferenceKF, mvpLocalMapPoints, frame_mp)`` as slots."""

    def __init__(self, device: int = 0, keyframes_hint: int = 0, points_hint: int = 0):
        st = C.c_int(0)
        h = lib().orbfe_map_create(device, keyframes_hint, points_hint, C.byref(st))
        if not h:
            raise OrbfeError("orbfe_map_create", st.value)
        self._h = C.c_void_p(h)
        self._children: dict[int, set] = {}

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().orbfe_map_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _i32(a) -> np.ndarray:
        return np.ascontiguousarray(a, np.int32).reshape(-1)

    def set_stream(self, stream_handle: int | None) -> None:
        _check("orbfe_map_set_stream", lib().orbfe_map_set_stream(self._h, _stream_arg(stream_handle)))

    def clear(self) -> None:
        _check("orbfe_map_clear", lib().orbfe_map_clear(self._h))
        self._children.clear()

    def size(self) -> tuple[int, int]:
        a, b = C.c_int32(0), C.c_int32(0)
        _check("orbfe_map_size", lib().orbfe_map_size(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def add_keyframe(self, order_key: int, n_slots: int, mp_slots=None) -> int:
        s = C.c_int32(-1)
        mp = None if mp_slots is None else self._i32(mp_slots)
        if mp is not None and len(mp) != n_slots:
            raise ValueError("mp_slots must hold n_slots entries")
        _check("orbfe_map_add_keyframe", lib().orbfe_map_add_keyframe(
            self._h, order_key, n_slots, None if mp is None else ptr(mp), C.byref(s)))
        return s.value

    def set_keyframe_points(self, slot: int, first: int, mp_slots) -> None:
        mp = self._i32(mp_slots)
        _check("orbfe_map_set_keyframe_points", lib().orbfe_map_set_keyframe_points(
            self._h, slot, first, len(mp), ptr(mp)))

    def AddMapPoint(self, kf: int, idx: int, mp: int) -> None:
        """KeyFrame::AddMapPoint(pMP, idx); mp = -1: EraseMapPointMatch(idx)."""
        self.set_keyframe_points(kf, idx, [mp])

    def set_keyframe_bad(self, kf: int, bad: bool = True) -> None:
        """mbBad of a keyframe alone."""
        _check("orbfe_map_set_keyframe_bad", lib().orbfe_map_set_keyframe_bad(self._h, kf, int(bad)))

    SetBadFlag = set_keyframe_bad   # the name this call had before SetKeyFrameBadFlag existed

    def UpdateBestCovisibles(self, kf: int, neigh_slots=None) -> None:
        """With ``neigh_slots``: GetBestCovisibilityKeyFrames(10) after KeyFrame::UpdateBestCovisibles,
        computed by the caller.  Without: KeyFrame::UpdateBestCovisibles itself, the ordered list
        re-sorted from the whole weight map on the device."""
        if neigh_slots is None:
            _check("orbfe_map_update_best_covisibles",
                   lib().orbfe_map_update_best_covisibles(self._h, kf))
            return
        n = self._i32(neigh_slots)
        _check("orbfe_map_set_covisibility", lib().orbfe_map_set_covisibility(
            self._h, kf, len(n), ptr(n)))

    def set_children(self, kf: int, child_slots) -> None:
        c = self._i32(child_slots)
        self._children[kf] = set(int(x) for x in c)
        _check("orbfe_map_set_children", lib().orbfe_map_set_children(self._h, kf, len(c), ptr(c)))

    def set_parent(self, kf: int, parent: int) -> None:
        """mpParent = parent (or -1) alone."""
        _check("orbfe_map_set_parent", lib().orbfe_map_set_parent(self._h, kf, parent))

    def AddChild(self, kf: int, child: int) -> None:
        """KeyFrame::AddChild: mspChildrens.insert(child)."""
        self.set_children(kf, sorted(self._children.get(kf, set()) | {child}))

    def EraseChild(self, kf: int, child: int) -> None:
        self.set_children(kf, sorted(self._children.get(kf, set()) - {child}))

    def ChangeParent(self, kf: int, parent: int) -> None:
        """KeyFrame::ChangeParent (KeyFrame.cc): mpParent = parent; parent->AddChild(this)."""
        self.set_parent(kf, parent)
        self.AddChild(parent, kf)

    def add_points(self, n: int) -> int:
        s = C.c_int32(-1)
        _check("orbfe_map_add_points", lib().orbfe_map_add_points(self._h, n, C.byref(s)))
        return s.value

    def SetBadFlagPoints(self, mp_slots, bad: bool = True) -> None:
        """MapPoint::SetBadFlag of every listed point."""
        p = self._i32(mp_slots)
        _check("orbfe_map_set_points_bad", lib().orbfe_map_set_points_bad(
            self._h, len(p), ptr(p), int(bad)))

    def AddObservation(self, mp_slots, kf_slots, idx=None) -> None:
        """MapPoint::AddObservation(pKF, idx), batched.  Without ``idx`` the index is recorded as
        unknown (-1) and nObs grows by 1."""
        p, k = self._i32(mp_slots), self._i32(kf_slots)
        if len(p) != len(k):
            raise ValueError("one keyframe per point")
        if idx is None:
            _check("orbfe_map_add_observations", lib().orbfe_map_add_observations(
                self._h, len(p), ptr(p), ptr(k)))
            return
        x = self._i32(idx)
        if len(x) != len(p):
            raise ValueError("one index per point")
        _check("orbfe_map_add_observations_idx", lib().orbfe_map_add_observations_idx(
            self._h, len(p), ptr(p), ptr(k), ptr(x)))

    def EraseObservation(self, mp_slots, kf_slots):
        """Two scalars: MapPoint::EraseObservation(pKF) in full, with its `nObs <= 2` rule
        -> whether the point went bad.  Sequences: the set erase alone, batched (nObs follows,
        no point is set bad)."""
        if np.isscalar(mp_slots) and np.isscalar(kf_slots):
            bad = C.c_int32(0)
            _check("orbfe_map_erase_observation", lib().orbfe_map_erase_observation(
                self._h, int(mp_slots), int(kf_slots), C.byref(bad)))
            return bool(bad.value)
        p, k = self._i32(mp_slots), self._i32(kf_slots)
        if len(p) != len(k):
            raise ValueError("one keyframe per point")
        _check("orbfe_map_erase_observations", lib().orbfe_map_erase_observations(
            self._h, len(p), ptr(p), ptr(k)))
        return None

    def set_stamps(self, kind: int, slots, stamps) -> None:
        s, v = self._i32(slots), np.ascontiguousarray(stamps, np.uint64).reshape(-1)
        if len(s) != len(v):
            raise ValueError("one stamp per slot")
        _check("orbfe_map_set_stamps", lib().orbfe_map_set_stamps(self._h, kind, len(s), ptr(s), ptr(v)))

    def get_stamps(self, kind: int, slots) -> np.ndarray:
        s = self._i32(slots)
        v = np.zeros(len(s), np.uint64)
        _check("orbfe_map_get_stamps", lib().orbfe_map_get_stamps(self._h, kind, len(s), ptr(s), ptr(v)))
        return v

    def set_local_keyframes(self, kf_slots, ref_kf: int) -> None:
        k = self._i32(kf_slots)
        _check("orbfe_map_set_local_keyframes", lib().orbfe_map_set_local_keyframes(
            self._h, len(k), ptr(k), ref_kf))

    def get_local_keyframes(self) -> tuple[np.ndarray, int]:
        out = np.zeros(MAP_MAX_VOTED + 8, np.int32)
        n, ref = C.c_int32(0), C.c_int32(-1)
        _check("orbfe_map_get_local_keyframes", lib().orbfe_map_get_local_keyframes(
            self._h, ptr(out), len(out), C.byref(n), C.byref(ref)))
        return out[:n.value].copy(), ref.value

    def UpdateLocalMap(self, frame_id: int, frame_mp, kf_cap: int = MAP_MAX_VOTED + 8,
                       mp_cap: int | None = None):
        """-> (local keyframes, reference keyframe, local points, updated frame_mp)."""
        f = self._i32(frame_mp).copy()
        if mp_cap is None:
            mp_cap = self.size()[1]
        kf = np.zeros(max(kf_cap, 1), np.int32)
        mp = np.zeros(max(mp_cap, 1), np.int32)
        nk, ref, nm = C.c_int32(0), C.c_int32(-1), C.c_int32(0)
        st = lib().orbfe_map_update_local(self._h, frame_id, len(f), ptr(f), ptr(kf), kf_cap,
                                          C.byref(nk), C.byref(ref), ptr(mp), mp_cap, C.byref(nm))
        if st != ORBFE_OK:
            e = OrbfeError("orbfe_map_update_local", st)
            e.counts = (nk.value, nm.value)
            e.frame_mp = f
            raise e
        return kf[:nk.value].copy(), ref.value, mp[:nm.value].copy(), f

    def update_local_device(self, frame_id: int, n: int, d_frame_mp: int,
                            kf_cap: int = MAP_MAX_VOTED + 8):
        """-> (local keyframes, reference keyframe, n_local_mp); the points stay on the device
        (``local_points_device``) and d_frame_mp is updated in place."""
        kf = np.zeros(max(kf_cap, 1), np.int32)
        nk, ref, nm = C.c_int32(0), C.c_int32(-1), C.c_int32(0)
        st = lib().orbfe_map_update_local_device(self._h, frame_id, n, C.c_void_p(d_frame_mp),
                                                 ptr(kf), kf_cap, C.byref(nk), C.byref(ref),
                                                 C.byref(nm))
        if st != ORBFE_OK:
            e = OrbfeError("orbfe_map_update_local_device", st)
            e.counts = (nk.value, nm.value)
            raise e
        return kf[:nk.value].copy(), ref.value, nm.value

    def local_points_device(self) -> tuple[int, int]:
        """-> (device pointer of the point list, its length)."""
        p, n = C.c_void_p(0), C.c_int32(0)
        _check("orbfe_map_local_points_device", lib().orbfe_map_local_points_device(
            self._h, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def get_local_points(self) -> np.ndarray:
        """mvpLocalMapPoints of the last successful query, copied to the host."""
        out = np.zeros(max(self.size()[1], 1), np.int32)
        n = C.c_int32(0)
        _check("orbfe_map_get_local_points", lib().orbfe_map_get_local_points(
            self._h, ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def gather_points_device(self, n: int, d_list: int, src: MapPointArrays,
                             dst: MapPointArrays) -> None:
        _check("orbfe_map_gather_points_device", lib().orbfe_map_gather_points_device(
            self._h, n, C.c_void_p(d_list), C.byref(src), C.byref(dst)))

    # ---- the covisibility graph (KeyFrame.cc:844-929, 1010-1100, 1188-1199, 1295-1309)
    def UpdateConnections(self, kf, allow_parent=None):
        """KeyFrame::UpdateConnections of one keyframe slot, or of a sequence of them in that
        order.  ``allow_parent`` is ``mnId != 0`` per keyframe (default: all true).
        -> (parents assigned by this call or -1, lengths of the ordered lists)."""
        k = self._i32([kf] if np.isscalar(kf) else kf)
        a = None if allow_parent is None else np.ascontiguousarray(
            [allow_parent] if np.isscalar(allow_parent) else allow_parent, np.uint8).reshape(-1)
        if a is not None and len(a) != len(k):
            raise ValueError("one allow_parent per keyframe")
        par, no = np.full(len(k), -1, np.int32), np.zeros(len(k), np.int32)
        _check("orbfe_map_update_connections", lib().orbfe_map_update_connections(
            self._h, len(k), ptr(k), ptr(a), ptr(par), ptr(no)))
        for c, p in zip(k, par):
            if p >= 0:
                self._children.setdefault(int(p), set()).add(int(c))
        return par, no

    def AddConnection(self, kf: int, other: int, weight: int) -> None:
        _check("orbfe_map_add_connection", lib().orbfe_map_add_connection(self._h, kf, other, weight))

    def EraseConnection(self, kf: int, other: int) -> None:
        _check("orbfe_map_erase_connection", lib().orbfe_map_erase_connection(self._h, kf, other))

    def erase_keyframe_connections(self, kf: int) -> None:
        """The connection part of KeyFrame::SetBadFlag (:1188-1189, :1198-1199)."""
        _check("orbfe_map_erase_keyframe_connections",
               lib().orbfe_map_erase_keyframe_connections(self._h, kf))

    def set_connections(self, kf: int, kf_slots, weights) -> None:
        s, w = self._i32(kf_slots), self._i32(weights)
        if len(s) != len(w):
            raise ValueError("one weight per keyframe")
        _check("orbfe_map_set_connections", lib().orbfe_map_set_connections(
            self._h, kf, len(s), ptr(s), ptr(w)))

    def set_ordered_connections(self, kf: int, kf_slots, weights) -> None:
        s, w = self._i32(kf_slots), self._i32(weights)
        if len(s) != len(w):
            raise ValueError("one weight per keyframe")
        _check("orbfe_map_set_ordered_connections", lib().orbfe_map_set_ordered_connections(
            self._h, kf, len(s), ptr(s), ptr(w)))

    def set_first_connection(self, kf: int, flag: bool) -> None:
        _check("orbfe_map_set_first_connection",
               lib().orbfe_map_set_first_connection(self._h, kf, int(flag)))

    def _connections(self, fn: str, kf: int):
        s, w = np.zeros(MAP_MAX_VOTED, np.int32), np.zeros(MAP_MAX_VOTED, np.int32)
        n = C.c_int32(0)
        _check(fn, getattr(lib(), fn)(self._h, kf, ptr(s), ptr(w), len(s), C.byref(n)))
        return s[:n.value].copy(), w[:n.value].copy()

    def get_connections(self, kf: int):
        """mConnectedKeyFrameWeights in pointer order -> (slots, weights)."""
        return self._connections("orbfe_map_get_connections", kf)

    def get_ordered_connections(self, kf: int):
        """mvpOrderedConnectedKeyFrames, mvOrderedWeights -> (slots, weights)."""
        return self._connections("orbfe_map_get_ordered_connections", kf)

    def get_spanning_tree(self, kf: int):
        """-> (mpParent or -1, mbFirstConnection, mspChildrens in pointer order)."""
        p, f, n = C.c_int32(-1), C.c_int32(0), C.c_int32(0)
        ch = np.zeros(max(self.size()[0], 1), np.int32)
        _check("orbfe_map_get_spanning_tree", lib().orbfe_map_get_spanning_tree(
            self._h, kf, C.byref(p), C.byref(f), ptr(ch), len(ch), C.byref(n)))
        return p.value, bool(f.value), ch[:n.value].copy()

    def GetConnectedKeyFrames(self, kf: int) -> set:
        return set(int(x) for x in self.get_connections(kf)[0])

    def GetVectorCovisibleKeyFrames(self, kf: int) -> np.ndarray:
        return self.get_ordered_connections(kf)[0]

    def GetBestCovisibilityKeyFrames(self, kf: int, n: int) -> np.ndarray:
        return self.get_ordered_connections(kf)[0][:max(n, 0)]

    def GetCovisiblesByWeight(self, kf: int, w: int) -> np.ndarray:
        """KeyFrame.cc:905-920 with its `it == end` quirk: when every weight is >= w the
        reference returns nothing."""
        s, ws = self.get_ordered_connections(kf)
        n = int(np.count_nonzero(ws >= w))  # upper_bound with a > b over descending weights
        return s[:0] if n == len(ws) else s[:n]

    def GetWeight(self, kf: int, other: int) -> int:
        s, w = self.get_connections(kf)
        hit = np.nonzero(s == other)[0]
        return int(w[hit[0]]) if len(hit) else 0

    def GetParent(self, kf: int) -> int:
        return self.get_spanning_tree(kf)[0]

    def GetChilds(self, kf: int) -> set:
        return set(int(x) for x in self.get_spanning_tree(kf)[2])

    # ---- culling (LocalMapping.cc:170-205, MapPoint.cc:339-409, KeyFrame.cc:971-996)
    def set_keyframe_features(self, kf: int, octaves=None, mvu_right=None, depth=None,
                              th_depth: float = 0.0) -> None:
        """mvKeysUn[i].octave, mvuRight (only ``>= 0`` is kept), mvDepth, mThDepth of a keyframe;
        every array holds one entry per slot (None: octave 0 / -1 / -1)."""
        arrs = [None if a is None else np.ascontiguousarray(a, t).reshape(-1)
                for a, t in ((octaves, np.int32), (mvu_right, np.float32), (depth, np.float32))]
        n = {len(a) for a in arrs if a is not None}
        if len(n) > 1:
            raise ValueError("one entry per slot in every array")
        n = n.pop() if n else len(self.get_keyframe_points(kf))
        _check("orbfe_map_set_keyframe_features", lib().orbfe_map_set_keyframe_features(
            self._h, kf, n, ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), float(th_depth)))

    def get_keyframe_features(self, kf: int):
        """-> (octaves, has_right, depth, th_depth)."""
        cap = MAP_MAX_KF_SLOTS
        o, r, d = np.zeros(cap, np.int32), np.zeros(cap, np.uint8), np.zeros(cap, np.float32)
        th, n = C.c_float(0), C.c_int32(0)
        _check("orbfe_map_get_keyframe_features", lib().orbfe_map_get_keyframe_features(
            self._h, kf, cap, ptr(o), ptr(r), ptr(d), C.byref(th), C.byref(n)))
        return o[:n.value].copy(), r[:n.value].astype(bool), d[:n.value].copy(), th.value

    def get_keyframe_points(self, kf: int) -> np.ndarray:
        """mvpMapPoints as point slots or -1."""
        out = np.zeros(MAP_MAX_KF_SLOTS, np.int32)
        n = C.c_int32(0)
        _check("orbfe_map_get_keyframe_points", lib().orbfe_map_get_keyframe_points(
            self._h, kf, ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def GetObservations(self, mp: int):
        """mObservations -> (keyframe slots ascending, feature indices or -1)."""
        cap = max(self.size()[0], 1)
        k, x = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = C.c_int32(0)
        _check("orbfe_map_get_observations", lib().orbfe_map_get_observations(
            self._h, mp, ptr(k), ptr(x), cap, C.byref(n)))
        return k[:n.value].copy(), x[:n.value].copy()

    def get_bad_flags(self, kind: int, slots) -> np.ndarray:
        s = self._i32(slots)
        out = np.zeros(len(s), np.uint8)
        _check("orbfe_map_get_bad_flags", lib().orbfe_map_get_bad_flags(
            self._h, kind, len(s), ptr(s), ptr(out)))
        return out.astype(bool)

    def set_point_counters(self, mp_slots, n_obs=None, found=None, visible=None, first_kf_id=None) -> None:
        s = self._i32(mp_slots)
        a = [None if v is None else np.ascontiguousarray(v, t).reshape(-1)
             for v, t in ((n_obs, np.int32), (found, np.int32), (visible, np.int32), (first_kf_id, np.int64))]
        if any(v is not None and len(v) != len(s) for v in a):
            raise ValueError("one value per point")
        _check("orbfe_map_set_point_counters", lib().orbfe_map_set_point_counters(
            self._h, len(s), ptr(s), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3])))

    def get_point_counters(self, mp_slots):
        """-> (nObs, mnFound, mnVisible, mnFirstKFid)."""
        s = self._i32(mp_slots)
        o, f, v = (np.zeros(len(s), np.int32) for _ in range(3))
        k = np.zeros(len(s), np.int64)
        _check("orbfe_map_get_point_counters", lib().orbfe_map_get_point_counters(
            self._h, len(s), ptr(s), ptr(o), ptr(f), ptr(v), ptr(k)))
        return o, f, v, k

    def _increase(self, kind: int, mp_slots, amounts) -> None:
        s = self._i32([mp_slots] if np.isscalar(mp_slots) else mp_slots)
        a = None if amounts is None else self._i32([amounts] if np.isscalar(amounts) else amounts)
        if a is not None and len(a) != len(s):
            raise ValueError("one amount per point")
        _check("orbfe_map_increase_counters", lib().orbfe_map_increase_counters(
            self._h, kind, len(s), ptr(s), ptr(a)))

    def IncreaseFound(self, mp_slots, n=None) -> None:
        self._increase(MAP_FOUND, mp_slots, n)

    def IncreaseVisible(self, mp_slots, n=None) -> None:
        self._increase(MAP_VISIBLE, mp_slots, n)

    def increase_counters_device(self, kind: int, n: int, d_mp_slots: int, d_mask: int | None = None) -> None:
        """By 1 for every entry >= 0 of the device array whose mask byte (if any) is set."""
        _check("orbfe_map_increase_counters_device", lib().orbfe_map_increase_counters_device(
            self._h, kind, n, C.c_void_p(d_mp_slots), C.c_void_p(d_mask or 0)))

    def Observations(self, mp: int) -> int:
        return int(self.get_point_counters([mp])[0][0])

    def GetFoundRatio(self, mp: int) -> float:
        _, f, v, _ = self.get_point_counters([mp])
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.float32(f[0]) / np.float32(v[0]))

    def SetMapPointBadFlag(self, mp_slots) -> None:
        """MapPoint::SetBadFlag in full: the flag, the observations cleared, EraseMapPointMatch on
        every former observer."""
        s = self._i32([mp_slots] if np.isscalar(mp_slots) else mp_slots)
        _check("orbfe_map_set_point_bad_flag", lib().orbfe_map_set_point_bad_flag(self._h, len(s), ptr(s)))

    def MapPointCulling(self, recent, current_kf_id: int, monocular: bool):
        """LocalMapping::MapPointCulling over mlpRecentAddedMapPoints -> (the list that remains,
        the points whose SetBadFlag ran)."""
        lst = self._i32(recent).copy()
        gone = np.zeros(max(len(lst), 1), np.int32)
        n, nc = C.c_int32(0), C.c_int32(0)
        _check("orbfe_map_cull_points", lib().orbfe_map_cull_points(
            self._h, int(current_kf_id), int(bool(monocular)), ptr(lst), len(lst), C.byref(n),
            ptr(gone), C.byref(nc)))
        return lst[:n.value].copy(), gone[:nc.value].copy()

    def SetNotErase(self, kf: int, flag: bool = True) -> None:
        _check("orbfe_map_set_not_erase", lib().orbfe_map_set_not_erase(self._h, kf, int(flag)))

    def get_erase_flags(self, kf: int) -> tuple[bool, bool]:
        """-> (mbNotErase, mbToBeErased)."""
        a, b = C.c_int32(0), C.c_int32(0)
        _check("orbfe_map_get_erase_flags", lib().orbfe_map_get_erase_flags(self._h, kf, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def _bad_flag_call(self, fn: str, *head):
        n_kf, n_mp = self.size()
        bad, pairs = np.zeros(max(n_mp, 1), np.int32), np.zeros(2 * max(n_kf, 1), np.int32)
        what, nb, npair = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(fn, getattr(lib(), fn)(self._h, *head, C.byref(what), ptr(bad), len(bad), C.byref(nb),
                                      ptr(pairs), len(pairs) // 2, C.byref(npair)))
        pr = pairs[:2 * npair.value].reshape(-1, 2).copy()
        self._refresh_children(pr)
        return what.value, bad[:nb.value].copy(), pr

    def _refresh_children(self, pairs) -> None:
        for k in list(self._children) + [int(x) for x in np.asarray(pairs).reshape(-1)]:
            self._children[k] = set(int(x) for x in self.get_spanning_tree(k)[2])

    def SetKeyFrameBadFlag(self, kf: int, is_first: bool = False):
        """KeyFrame::SetBadFlag in full -> (MAP_BAD_NOTHING | MAP_BAD_DEFERRED | MAP_BAD_DONE, the
        points that went bad, the (child, new parent) pairs)."""
        return self._bad_flag_call("orbfe_map_set_keyframe_bad_flag", kf, int(bool(is_first)))

    def SetErase(self, kf: int, has_loop_edges: bool = False, is_first: bool = False):
        """KeyFrame::SetErase -> as SetKeyFrameBadFlag."""
        return self._bad_flag_call("orbfe_map_set_erase", kf, int(bool(has_loop_edges)), int(bool(is_first)))

    def KeyFrameCulling(self, current_kf: int, monocular: bool, kf_slots=None, first_kf: int = -1):
        """LocalMapping::KeyFrameCulling over the ordered covisibility list of ``current_kf`` (or
        over ``kf_slots``) -> (the list, its results MAP_CULL_*, the points that went bad, the
        (child, new parent) pairs)."""
        n_kf, n_mp = self.size()
        k = None if kf_slots is None else self._i32(kf_slots)
        if k is None:
            lst = self.get_ordered_connections(current_kf)[0]
        else:
            lst = k.copy()
        res = np.zeros(max(len(lst), 1), np.int32)
        bad, pairs = np.zeros(max(n_mp, 1), np.int32), np.zeros(2 * max(n_kf, 1) * max(len(lst), 1), np.int32)
        nl, nb, npair = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check("orbfe_map_cull_keyframes", lib().orbfe_map_cull_keyframes(
            self._h, current_kf, -1 if k is None else len(k), ptr(k) if k is not None and len(k) else
            (None if k is None else ptr(np.zeros(1, np.int32))), first_kf, int(bool(monocular)), ptr(res), len(lst),
            C.byref(nl), ptr(bad), len(bad), C.byref(nb), ptr(pairs), len(pairs) // 2, C.byref(npair)))
        pr = pairs[:2 * npair.value].reshape(-1, 2).copy()
        self._refresh_children(pr)
        return lst, res[:nl.value].copy(), bad[:nb.value].copy(), pr

    def TrackedMapPoints(self, kf: int, min_obs: int) -> int:
        n = C.c_int32(0)
        _check("orbfe_map_tracked_map_points", lib().orbfe_map_tracked_map_points(
            self._h, kf, min_obs, C.byref(n)))
        return n.value

    # ---- MapPoint refresh (MapPoint.cc:483-548, 571-619; LocalMapping.cc:140-161)
    def SetScaleFactors(self, scale) -> None:
        """mvScaleFactors of the map's keyframes."""
        s = np.ascontiguousarray(scale, np.float32).reshape(-1)
        _check("orbfe_map_set_scale_factors", lib().orbfe_map_set_scale_factors(self._h, len(s), ptr(s)))

    def GetScaleFactors(self) -> np.ndarray:
        s, n = np.zeros(128, np.float32), C.c_int32(0)
        _check("orbfe_map_get_scale_factors", lib().orbfe_map_get_scale_factors(
            self._h, ptr(s), len(s), C.byref(n)))
        return s[:n.value].copy()

    def SetCameraCenter(self, kf_slots, ow) -> None:
        """GetCameraCenter() of one keyframe (three floats) or of a sequence (n x 3)."""
        k = self._i32([kf_slots] if np.isscalar(kf_slots) else kf_slots)
        o = np.ascontiguousarray(ow, np.float32).reshape(-1)
        if len(o) != 3 * len(k):
            raise ValueError("three floats per keyframe")
        _check("orbfe_map_set_keyframe_centers", lib().orbfe_map_set_keyframe_centers(
            self._h, len(k), ptr(k), ptr(o)))

    def GetCameraCenter(self, kf_slots) -> np.ndarray:
        k = self._i32([kf_slots] if np.isscalar(kf_slots) else kf_slots)
        o = np.zeros((len(k), 3), np.float32)
        _check("orbfe_map_get_keyframe_centers", lib().orbfe_map_get_keyframe_centers(
            self._h, len(k), ptr(k), ptr(o)))
        return o[0] if np.isscalar(kf_slots) else o

    def SetDescriptors(self, kf: int, desc=None, d_desc: int | None = None, n: int | None = None) -> None:
        """mDescriptors of a keyframe: an (n_slots, 32) uint8 array, or ``d_desc`` a device pointer
        to ``n`` rows (copied on the handle's stream)."""
        if d_desc is not None:
            _check("orbfe_map_set_keyframe_descriptors_device",
                   lib().orbfe_map_set_keyframe_descriptors_device(self._h, kf, int(n), C.c_void_p(d_desc)))
            return
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        _check("orbfe_map_set_keyframe_descriptors", lib().orbfe_map_set_keyframe_descriptors(
            self._h, kf, len(d), ptr(d)))

    def GetDescriptors(self, kf: int):
        """-> (descriptors (n_slots, 32), whether they were ever set)."""
        d = np.zeros((MAP_MAX_KF_SLOTS, 32), np.uint8)
        n, s = C.c_int32(0), C.c_int32(0)
        _check("orbfe_map_get_keyframe_descriptors", lib().orbfe_map_get_keyframe_descriptors(
            self._h, kf, len(d), ptr(d), C.byref(n), C.byref(s)))
        return d[:n.value].copy(), bool(s.value)

    def SetReferenceKeyFrame(self, mp_slots, kf_slots) -> None:
        """mpRefKF of the listed points: keyframe slots or -1."""
        p = self._i32([mp_slots] if np.isscalar(mp_slots) else mp_slots)
        k = self._i32([kf_slots] if np.isscalar(kf_slots) else kf_slots)
        if len(p) != len(k):
            raise ValueError("one keyframe per point")
        _check("orbfe_map_set_point_ref_keyframes", lib().orbfe_map_set_point_ref_keyframes(
            self._h, len(p), ptr(p), ptr(k)))

    def GetReferenceKeyFrame(self, mp_slots):
        p = self._i32([mp_slots] if np.isscalar(mp_slots) else mp_slots)
        k = np.full(len(p), -1, np.int32)
        _check("orbfe_map_get_point_ref_keyframes", lib().orbfe_map_get_point_ref_keyframes(
            self._h, len(p), ptr(p), ptr(k)))
        return int(k[0]) if np.isscalar(mp_slots) else k

    def RefreshPoints(self, what: int, mp_slots, arrays: MapPointArrays, d_list: int | None = None,
                      n: int | None = None, d_result: int | None = None):
        """UpdateNormalAndDepth (``what & 1``) and ComputeDistinctiveDescriptors (``what & 2``) of
        the listed points, written into the map-wide device ``arrays``.  Host list -> the masks of
        what was written per entry; with ``d_list`` (a device pointer to ``n`` slots) the masks go
        to ``d_result`` if given.  A refusal raises; ORBFE_ERR_UNSUPPORTED raises with ``e.result``
        holding the masks of the host form (everything else was written)."""
        if d_list is not None:
            _check("orbfe_map_refresh_points_device", lib().orbfe_map_refresh_points_device(
                self._h, what, int(n), C.c_void_p(d_list), C.byref(arrays), C.c_void_p(d_result or 0)))
            return None
        p = self._i32(mp_slots)
        res = np.zeros(len(p), np.uint8)
        st = lib().orbfe_map_refresh_points(self._h, what, len(p), ptr(p) if len(p) else None,
                                            C.byref(arrays), ptr(res) if len(p) else None)
        if st != ORBFE_OK:
            e = OrbfeError("orbfe_map_refresh_points", st)
            e.result = res
            raise e
        return res

    def UpdateNormalAndDepth(self, mp_slots, arrays: MapPointArrays):
        return self.RefreshPoints(MAP_REFRESH_NORMAL_DEPTH, [mp_slots] if np.isscalar(mp_slots) else mp_slots, arrays)

    def ComputeDistinctiveDescriptors(self, mp_slots, arrays: MapPointArrays):
        return self.RefreshPoints(MAP_REFRESH_DESCRIPTOR, [mp_slots] if np.isscalar(mp_slots) else mp_slots, arrays)

    def RefreshKeyFramePoints(self, kf: int, arrays: MapPointArrays,
                              what: int = MAP_REFRESH_NORMAL_DEPTH | MAP_REFRESH_DESCRIPTOR) -> int:
        """Both functions over the keyframe's mvpMapPoints where it lies (LocalMapping.cc:518-530)
        -> the number of entries refreshed."""
        n = C.c_int32(0)
        _check("orbfe_map_refresh_keyframe_points", lib().orbfe_map_refresh_keyframe_points(
            self._h, kf, what, C.byref(arrays), C.byref(n)))
        return n.value

    def ProcessNewKeyFrame(self, kf: int, arrays: MapPointArrays, recent_cap: int = MAP_MAX_KF_SLOTS):
        """The map-point loop of LocalMapping::ProcessNewKeyFrame (:140-161) -> the points to append
        to mlpRecentAddedMapPoints, in index order."""
        rec = np.zeros(max(recent_cap, 1), np.int32)
        n = C.c_int32(0)
        st = lib().orbfe_map_process_new_keyframe(self._h, kf, C.byref(arrays), ptr(rec), recent_cap, C.byref(n))
        if st != ORBFE_OK:
            e = OrbfeError("orbfe_map_process_new_keyframe", st)
            e.count = n.value
            raise e
        return rec[:n.value].copy()


class ORBmatcher:
    """``ORBmatcher(nnratio=0.6, checkOri=true)`` (ORBmatcher.cc:41-43), GPU-backed."""

    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30  # ORBmatcher.cc:37-39

    def __init__(self, nnratio: float = 0.6, checkOri: bool = True, device: int = 0):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        st = C.c_int(0)
        h = lib().orbfe_matcher_create(device, C.byref(st))
        if not h:
            raise OrbfeError("orbfe_matcher_create", st.value)
        self._h = C.c_void_p(h)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().orbfe_matcher_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def DescriptorDistance(self, a: np.ndarray, b: np.ndarray) -> np.ndarray | int:
        """Row-wise Hamming distance (ORBmatcher.cc:1650-1666)."""
        a2 = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
        b2 = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
        out = np.zeros(len(a2), np.int32)
        _check("orbfe_hamming", lib().orbfe_hamming(self._h, ptr(a2), ptr(b2), len(a2), ptr(out)))
        return int(out[0]) if np.ndim(a) == 1 else out

    def bf_match(self, q: np.ndarray, r: np.ndarray):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        r = np.ascontiguousarray(r, np.uint8).reshape(-1, 32)
        bi, bd, sd = (np.zeros(len(q), np.int32) for _ in range(3))
        _check("orbfe_bf_match", lib().orbfe_bf_match(self._h, ptr(q), len(q), ptr(r), len(r),
                                                      ptr(bi), ptr(bd), ptr(sd)))
        return bi, bd, sd

    def bf_match_batch_device(self, d_q: int, q_pitch: int, d_nq: int, nq_cap: int, d_r: int,
                              r_pitch: int, d_nr: int, nb: int, d_out: int) -> None:
        _check("orbfe_bf_match_batch_device", lib().orbfe_bf_match_batch_device(
            self._h, C.c_void_p(d_q), C.c_size_t(q_pitch), C.c_void_p(d_nq), nq_cap,
            C.c_void_p(d_r), C.c_size_t(r_pitch), C.c_void_p(d_nr), nb, C.c_void_p(d_out)))

    def profile(self, enable: bool) -> None:
        _check("orbfe_matcher_profile", lib().orbfe_matcher_profile(self._h, int(enable)))

    def profile_read(self) -> tuple[float, int]:
        """(total ms, launches) of the brute-force match kernels since the previous read."""
        ms = np.zeros(1, np.float64)
        n = np.zeros(1, np.int32)
        _check("orbfe_matcher_profile_read", lib().orbfe_matcher_profile_read(self._h, ptr(ms), ptr(n)))
        return float(ms[0]), int(n[0])

    def profile_read_stages(self) -> dict:
        """{"bf_match": (ms, launches), "bf_expand": (ms, launches)} since the previous read:
        the match kernels and the shared-reference expansion (orbfe_matcher_profile_read_stages)."""
        ms = np.zeros(2, np.float64)
        n = np.zeros(2, np.int32)
        _check("orbfe_matcher_profile_read_stages",
               lib().orbfe_matcher_profile_read_stages(self._h, ptr(ms), ptr(n)))
        return {"bf_match": (float(ms[0]), int(n[0])), "bf_expand": (float(ms[1]), int(n[1]))}

    def set_stream(self, stream_handle: int | None) -> None:
        _check("orbfe_matcher_set_stream", lib().orbfe_matcher_set_stream(
            self._h, _stream_arg(stream_handle)))

    def SearchForInitialization(self, F1: Frame, F2: Frame, vbPrevMatched: np.ndarray,
                                windowSize: int = 10):
        """Returns (vnMatches12, nmatches, updated vbPrevMatched) (ORBmatcher.cc:408-523)."""
        prev = np.ascontiguousarray(vbPrevMatched, np.float32).reshape(-1, 2).copy()
        m12 = np.zeros(F1.n, np.int32)
        nm = C.c_int32(0)
        v1, v2 = F1.view(), F2.view()
        _check("orbfe_search_for_initialization", lib().orbfe_search_for_initialization(
            self._h, C.c_float(self.mfNNratio), int(self.mbCheckOrientation), C.byref(v1),
            C.byref(v2), ptr(prev), windowSize, ptr(m12), C.byref(nm)))
        return m12, nm.value, prev

    def SearchByProjection(self, F: Frame, mps: MapPoints, th: float = 3.0, frame_mp=None,
                           frame_mp_obs=None, mp_ids=None):
        """Local-map overload (ORBmatcher.cc:45-129).  Returns (frame_mp, frame_mp_obs,
        nmatches): the MapPoint id held by each keypoint (-1 = none)."""
        fmp = (np.full(F.n, -1, np.int32) if frame_mp is None
               else np.ascontiguousarray(frame_mp, np.int32).copy())
        fobs = (np.zeros(F.n, np.int32) if frame_mp_obs is None
                else np.ascontiguousarray(frame_mp_obs, np.int32).copy())
        ids = None if mp_ids is None else np.ascontiguousarray(mp_ids, np.int32)
        nm = C.c_int32(0)
        fv, mv = F.view(), mps.view()
        return _check_results(
            "orbfe_search_by_projection_local", lib().orbfe_search_by_projection_local(
                self._h, C.c_float(self.mfNNratio), C.byref(fv), ptr(fmp), ptr(fobs), C.byref(mv),
                ptr(ids), C.c_float(th), C.byref(nm)), lambda: (fmp, fobs, nm.value))

    def SearchByProjectionLast(self, cur: Frame, tcw_cur, cam: Camera, last_keys, last_valid,
                               last_outlier, last_xyz, last_desc, last_nobs, tcw_last,
                               th: float, bMono: bool, frame_mp=None, frame_mp_obs=None,
                               last_ids=None):
        """Last-frame overload (ORBmatcher.cc:1331-1473)."""
        fmp = (np.full(cur.n, -1, np.int32) if frame_mp is None
               else np.ascontiguousarray(frame_mp, np.int32).copy())
        fobs = (np.zeros(cur.n, np.int32) if frame_mp_obs is None
                else np.ascontiguousarray(frame_mp_obs, np.int32).copy())
        a = [np.ascontiguousarray(tcw_cur, np.float32).reshape(12),
             np.ascontiguousarray(last_keys, KEYPOINT_DTYPE),
             np.ascontiguousarray(last_valid, np.uint8),
             np.ascontiguousarray(last_outlier, np.uint8),
             np.ascontiguousarray(last_xyz, np.float32).reshape(-1, 3),
             np.ascontiguousarray(last_desc, np.uint8).reshape(-1, 32),
             np.ascontiguousarray(last_nobs, np.int32),
             np.ascontiguousarray(tcw_last, np.float32).reshape(12)]
        ids = None if last_ids is None else np.ascontiguousarray(last_ids, np.int32)
        nm = C.c_int32(0)
        cv = cur.view()
        _check("orbfe_search_by_projection_last", lib().orbfe_search_by_projection_last(
            self._h, int(self.mbCheckOrientation), C.byref(cv), ptr(a[0]), C.byref(cam),
            ptr(fmp), ptr(fobs), len(a[1]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(a[4]),
            ptr(a[5]), ptr(a[6]), ptr(ids), ptr(a[7]), C.c_float(th), int(bMono),
            C.byref(nm)))
        return fmp, fobs, nm.value

    def SearchByProjectionKeyFrame(self, cur: Frame, tcw_cur, cam: Camera, log_scale: float,
                                   kf_angle, kf_valid, kf_bad, already_found, kf_xyz, kf_desc,
                                   kf_min_dist, kf_max_dist, th: float, ORBdist: int,
                                   frame_mp=None, kf_ids=None):
        """Relocalisation overload SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th,
        ORBdist) (ORBmatcher.cc:1475-1602).  Returns (frame_mp, nmatches)."""
        fmp = (np.full(cur.n, -1, np.int32) if frame_mp is None
               else np.ascontiguousarray(frame_mp, np.int32).copy())
        a = [np.ascontiguousarray(tcw_cur, np.float32).reshape(12),
             np.ascontiguousarray(kf_angle, np.float32),
             np.ascontiguousarray(kf_valid, np.uint8),
             np.ascontiguousarray(kf_bad, np.uint8),
             np.ascontiguousarray(already_found, np.uint8),
             np.ascontiguousarray(kf_xyz, np.float32).reshape(-1, 3),
             np.ascontiguousarray(kf_desc, np.uint8).reshape(-1, 32),
             np.ascontiguousarray(kf_min_dist, np.float32),
             np.ascontiguousarray(kf_max_dist, np.float32)]
        ids = None if kf_ids is None else np.ascontiguousarray(kf_ids, np.int32)
        nm = C.c_int32(0)
        cv = cur.view()
        return _check_results(
            "orbfe_search_by_projection_keyframe", lib().orbfe_search_by_projection_keyframe(
                self._h, int(self.mbCheckOrientation), C.byref(cv), ptr(a[0]), C.byref(cam),
                C.c_float(log_scale), ptr(fmp), len(a[1]), *(ptr(x) for x in a[1:]), ptr(ids),
                C.c_float(th), int(ORBdist), C.byref(nm)), lambda: (fmp, nm.value))

    FUSE_SE3, FUSE_SIM3 = 0, 1  # ORBFE_FUSE_*

    def FuseSearch(self, kf: Frame, tcw, cam: Camera, log_scale: float, inv_level_sigma2,
                   mp_xyz, mp_normal, mp_min_dist, mp_max_dist, mp_desc, th: float = 3.0,
                   mode: int = 0, skip=None):
        """The search half of ORBmatcher::Fuse (ORBmatcher.cc:828-978; mode FUSE_SIM3: the
        loop-closing overload, 980-1103, with the normalised [R|t]) for one keyframe
        (orbfe_fuse_search).  Returns (best_idx, best_dist, n_found): per point the keypoint to
        fuse into (-1: none) and the winning descriptor distance (256: no candidate).  A predicted
        level outside the pyramid raises OrbfeError(ORBFE_ERR_UNSUPPORTED) carrying the valid
        results of every other point as ``.results``."""
        a = [np.ascontiguousarray(tcw, np.float32).reshape(12),
             np.ascontiguousarray(inv_level_sigma2, np.float32),
             np.ascontiguousarray(mp_xyz, np.float32).reshape(-1, 3),
             np.ascontiguousarray(mp_normal, np.float32).reshape(-1, 3),
             np.ascontiguousarray(mp_min_dist, np.float32),
             np.ascontiguousarray(mp_max_dist, np.float32),
             np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)]
        n = len(a[2])
        assert len(a[1]) >= len(kf.scale_factors)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        bi = np.full(n, -1, np.int32)
        bd = np.full(n, 256, np.int32)
        nf = C.c_int32(0)
        kv = kf.view()
        st = lib().orbfe_fuse_search(
            self._h, C.byref(kv), ptr(a[0]), C.byref(cam), C.c_float(log_scale), ptr(a[1]), n,
            *(ptr(x) for x in a[2:]), ptr(sk), C.c_float(th), int(mode), ptr(bi), ptr(bd),
            C.byref(nf))
        if st != ORBFE_OK:
            e = OrbfeError("orbfe_fuse_search", st)
            e.results = (bi, bd, nf.value)
            raise e
        return bi, bd, nf.value

    def fuse_search_batch_device(self, n_kf: int, d_keys: int, keys_pitch: int, d_desc: int,
                                 desc_pitch: int, d_u_right: int | None, kp_cap: int, d_n: int,
                                 tcw, cam: Camera, bounds, scale_factors, inv_level_sigma2,
                                 log_scale: float, n_mp: int, d_xyz: int, d_normal: int,
                                 d_min: int, d_max: int, d_mdesc: int, d_skip: int | None,
                                 th: float, mode: int, d_best_idx: int,
                                 d_best_dist: int | None, d_status: int) -> None:
        """Fuse's search for n_kf keyframes against one shared point set, device-resident
        (orbfe_fuse_search_batch_device): raw device pointers, keys_pitch in keypoints,
        desc_pitch in bytes; tcw (n_kf, 3, 4) on the host; bounds = (min_x, max_x, min_y,
        max_y).  Asynchronous on the matcher's stream."""
        t = np.ascontiguousarray(tcw, np.float32).reshape(-1)
        assert len(t) == 12 * n_kf
        sf = np.ascontiguousarray(scale_factors, np.float32)
        isg = np.ascontiguousarray(inv_level_sigma2, np.float32)
        assert len(isg) >= len(sf)
        vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        _check("orbfe_fuse_search_batch_device", lib().orbfe_fuse_search_batch_device(
            self._h, n_kf, vp(d_keys), C.c_size_t(keys_pitch), vp(d_desc),
            C.c_size_t(desc_pitch), vp(d_u_right), kp_cap, vp(d_n), ptr(t), C.byref(cam),
            *(C.c_float(b) for b in bounds), ptr(sf), ptr(isg), len(sf), C.c_float(log_scale),
            n_mp, vp(d_xyz), vp(d_normal), vp(d_min), vp(d_max), vp(d_mdesc), vp(d_skip),
            C.c_float(th), int(mode), vp(d_best_idx), vp(d_best_dist), vp(d_status)))

    def ComputeDistinctiveDescriptors(self, obs_off: np.ndarray, obs_desc: np.ndarray):
        """MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:483-548) over a CSR of the
        points' observation descriptors -> (best row per point or -1, mDescriptor (n, 32))."""
        off = np.ascontiguousarray(obs_off, np.int32)
        d = np.ascontiguousarray(obs_desc, np.uint8).reshape(-1, 32)
        n = len(off) - 1
        best = np.zeros(n, np.int32)
        out = np.zeros((n, 32), np.uint8)
        _check("orbfe_distinctive_descriptors", lib().orbfe_distinctive_descriptors(
            self._h, n, ptr(off), ptr(d), ptr(best), ptr(out)))
        return best, out

    def search_local_points_device(self, n_kp: int, d_keys: int, d_desc: int,
                                   d_u_right: int | None, width: int, height: int,
                                   scale_factors: np.ndarray, tcw, cam: Camera,
                                   log_scale: float, cos_limit: float, n_mp: int, d_xyz: int,
                                   d_normal: int, d_min: int, d_max: int, d_mdesc: int,
                                   d_nobs: int, d_bad: int, d_skip: int | None,
                                   d_ids: int | None, nnratio: float, th: float, d_fmp: int,
                                   d_fobs: int, d_in_view: int) -> tuple[int, int]:
        """Tracking::SearchLocalPoints on device-resident frame + local map
        (orbfe_search_local_points_device) -> (nmatches, nToMatch)."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        gw = np.float32(64) / np.float32(width)
        gh = np.float32(48) / np.float32(height)
        fv = FrameView(n_kp, C.c_void_p(d_keys), C.c_void_p(d_desc),
                       C.c_void_p(d_u_right) if d_u_right else None, 0.0, float(width), 0.0,
                       float(height), float(gw), float(gh), ptr(sf), len(sf))
        t = np.ascontiguousarray(tcw, np.float32).reshape(12)
        counts = np.zeros(2, np.int32)
        vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        return _check_results(
            "orbfe_search_local_points_device", lib().orbfe_search_local_points_device(
                self._h, C.byref(fv), ptr(t), C.byref(cam), C.c_float(log_scale),
                C.c_float(cos_limit), n_mp, vp(d_xyz), vp(d_normal), vp(d_min), vp(d_max),
                vp(d_mdesc), vp(d_nobs), vp(d_bad), vp(d_skip), vp(d_ids), C.c_float(nnratio),
                C.c_float(th), vp(d_fmp), vp(d_fobs), vp(d_in_view), ptr(counts)),
            lambda: (int(counts[0]), int(counts[1])))

    def search_by_projection_local_device(self, n_kp: int, d_keys: int, d_desc: int,
                                          d_u_right: int | None, width: int, height: int,
                                          scale_factors: np.ndarray, n_mp: int,
                                          d_in_view: int, d_bad: int, d_px: int, d_py: int,
                                          d_pxr: int, d_lvl: int, d_vcos: int, d_mdesc: int,
                                          d_nobs: int, d_ids: int | None, nnratio: float,
                                          th: float, d_fmp: int, d_fobs: int) -> int:
        """SearchByProjection(F, vpLocalMapPoints, th) alone on device-resident isInFrustum
        outputs (orbfe_search_by_projection_local_device) -> nmatches."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        gw = np.float32(64) / np.float32(width)
        gh = np.float32(48) / np.float32(height)
        fv = FrameView(n_kp, C.c_void_p(d_keys), C.c_void_p(d_desc),
                       C.c_void_p(d_u_right) if d_u_right else None, 0.0, float(width), 0.0,
                       float(height), float(gw), float(gh), ptr(sf), len(sf))
        vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        mv = MapPointView(n_mp, vp(d_in_view), vp(d_bad), vp(d_px), vp(d_py), vp(d_pxr),
                          vp(d_lvl), vp(d_vcos), vp(d_mdesc), vp(d_nobs))
        nm = C.c_int32(0)
        return _check_results(
            "orbfe_search_by_projection_local_device",
            lib().orbfe_search_by_projection_local_device(
                self._h, C.c_float(nnratio), C.byref(fv), vp(d_fmp), vp(d_fobs), C.byref(mv),
                vp(d_ids), C.c_float(th), C.byref(nm)), lambda: nm.value)

    def last_rounds(self) -> int:
        return lib().orbfe_matcher_last_rounds(self._h)

    def GetFeaturesInArea(self, F: Frame, x, y, r, min_level=-1, max_level=-1, wave=False):
        """Frame::GetFeaturesInArea (Frame.cc:445-498) for arrays of queries on F's grid
        (orbfe_features_in_area).  Returns one int32 array of keypoint indices per query, in
        the reference's candidate order."""
        x = np.ascontiguousarray(np.atleast_1d(x), np.float32)
        nq = len(x)
        y = np.ascontiguousarray(np.broadcast_to(np.asarray(y, np.float32), (nq,)))
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r, np.float32), (nq,)))
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(min_level, np.int32), (nq,)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(max_level, np.int32), (nq,)))
        off = np.zeros(nq + 1, np.int32)
        fv = F.view()
        st = lib().orbfe_features_in_area(self._h, C.byref(fv), nq, ptr(x), ptr(y), ptr(r),
                                          ptr(lo), ptr(hi), int(bool(wave)), ptr(off), None, 0)
        items = np.zeros(max(int(off[nq]), 1), np.int32)
        if st == ORBFE_ERR_CAPACITY:
            st = lib().orbfe_features_in_area(self._h, C.byref(fv), nq, ptr(x), ptr(y), ptr(r),
                                              ptr(lo), ptr(hi), int(bool(wave)), ptr(off),
                                              ptr(items), len(items))
        _check("orbfe_features_in_area", st)
        return [items[off[q]:off[q + 1]].copy() for q in range(nq)]

    def capacity_retries(self) -> int:
        """Calls rerun because their candidates outgrew the device buffer (diagnostics)."""
        return lib().orbfe_matcher_capacity_retries(self._h)

    def SearchByBoW(self, kf_desc, kf_angle, kf_mp_ok, kf_fv, f_desc, f_angle, f_fv):
        """SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:159-291); *_fv are
        (node_ids, node_off, feat) FeatureVectors.  Returns (matches per frame feature, n)."""
        kd = np.ascontiguousarray(kf_desc, np.uint8).reshape(-1, 32)
        fd = np.ascontiguousarray(f_desc, np.uint8).reshape(-1, 32)
        ka = np.ascontiguousarray(kf_angle, np.float32)
        fa = np.ascontiguousarray(f_angle, np.float32)
        ok = np.ascontiguousarray(kf_mp_ok, np.uint8)
        kn, ko, kfe = (np.ascontiguousarray(x, np.int32) for x in kf_fv)
        fn, fo, ffe = (np.ascontiguousarray(x, np.int32) for x in f_fv)
        out = np.zeros(len(fd), np.int32)
        nm = C.c_int32(0)
        _check("orbfe_search_by_bow", lib().orbfe_search_by_bow(
            self._h, C.c_float(self.mfNNratio), int(self.mbCheckOrientation), len(kd), ptr(kd),
            ptr(ka), ptr(ok), len(kn), ptr(kn), ptr(ko), ptr(kfe), len(fd), ptr(fd), ptr(fa),
            len(fn), ptr(fn), ptr(fo), ptr(ffe), ptr(out), C.byref(nm)))
        return out, nm.value

    def search_by_bow_batch_device(self, n_pairs: int, d_pair_kf: int, d_pair_f: int,
                                   kf_cap: int, d_kf_desc: int, d_kf_angle: int, d_kf_mp_ok: int,
                                   d_kf_nn: int, d_kf_node_ids: int, d_kf_node_off: int,
                                   d_kf_feat: int, f_cap: int, d_f_desc: int, d_f_angle: int,
                                   d_f_nn: int, d_f_node_ids: int, d_f_node_off: int,
                                   d_f_feat: int, d_matches: int, d_nmatches: int,
                                   d_status: int) -> None:
        """SearchByBoW over n_pairs (keyframe slot, frame slot) pairs (Tracking::Relocalization's
        candidate loop, Tracking.cc:1636-1656); device pointers in the layout of
        Vocabulary.transform_batch_device.  Asynchronous on the matcher's stream."""
        v = C.c_void_p
        _check("orbfe_search_by_bow_batch_device", lib().orbfe_search_by_bow_batch_device(
            self._h, C.c_float(self.mfNNratio), int(self.mbCheckOrientation), n_pairs,
            v(d_pair_kf), v(d_pair_f), kf_cap, v(d_kf_desc), v(d_kf_angle), v(d_kf_mp_ok),
            v(d_kf_nn), v(d_kf_node_ids), v(d_kf_node_off), v(d_kf_feat), f_cap, v(d_f_desc),
            v(d_f_angle), v(d_f_nn), v(d_f_node_ids), v(d_f_node_off), v(d_f_feat),
            v(d_matches), v(d_nmatches), v(d_status)))

    def SearchByBoWKeyFrames(self, desc1, angle1, mp_ok1, fv1, desc2, angle2, mp_ok2, fv2):
        """SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (ORBmatcher.cc:525-658)
        through orbfe_search_by_bow_keyframes; mp_ok*: the feature holds a map point that is not
        bad; fv*: (node_ids, node_off, feat) FeatureVectors.  Returns (matches12, nmatches):
        per KF1 feature the KF2 feature whose map point it takes, or -1."""
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        a1 = np.ascontiguousarray(angle1, np.float32)
        a2 = np.ascontiguousarray(angle2, np.float32)
        ok1 = np.ascontiguousarray(mp_ok1, np.uint8)
        ok2 = np.ascontiguousarray(mp_ok2, np.uint8)
        n1, o1, f1 = (np.ascontiguousarray(x, np.int32) for x in fv1)
        n2, o2, f2 = (np.ascontiguousarray(x, np.int32) for x in fv2)
        out = np.full(len(d1), -1, np.int32)
        nm = C.c_int32(0)
        st = lib().orbfe_search_by_bow_keyframes(
            self._h, C.c_float(self.mfNNratio), int(self.mbCheckOrientation), len(d1), ptr(d1),
            ptr(a1), ptr(ok1), len(n1), ptr(n1), ptr(o1), ptr(f1), len(d2), ptr(d2), ptr(a2),
            ptr(ok2), len(n2), ptr(n2), ptr(o2), ptr(f2), ptr(out), C.byref(nm))
        if st != ORBFE_OK:
            e = OrbfeError("orbfe_search_by_bow_keyframes", st)
            e.results = (out, nm.value)
            raise e
        return out, nm.value

    def search_by_bow_keyframes_batch_device(self, n_pairs: int, d_pair_kf1: int,
                                             d_pair_kf2: int, cap: int, d_desc: int,
                                             d_angle: int, d_mp_ok: int, d_nn: int,
                                             d_node_ids: int, d_node_off: int, d_feat: int,
                                             d_matches12: int, d_nmatches: int,
                                             d_status: int) -> None:
        """SearchByBoW(pKF1, pKF2, ...) over n_pairs pairs of slots of one keyframe set
        (LoopClosing::ComputeSim3's candidate loop, LoopClosing.cc:266); device pointers in the
        layout of Vocabulary.transform_batch_device.  Asynchronous on the matcher's stream."""
        v = C.c_void_p
        _check("orbfe_search_by_bow_keyframes_batch_device",
               lib().orbfe_search_by_bow_keyframes_batch_device(
                   self._h, C.c_float(self.mfNNratio), int(self.mbCheckOrientation), n_pairs,
                   v(d_pair_kf1), v(d_pair_kf2), cap, v(d_desc), v(d_angle), v(d_mp_ok), v(d_nn),
                   v(d_node_ids), v(d_node_off), v(d_feat), v(d_matches12), v(d_nmatches),
                   v(d_status)))

    def SearchByProjectionSim3(self, kf: Frame, tcw, cam: Camera, log_scale: float, mp_xyz,
                               mp_normal, mp_min_dist, mp_max_dist, mp_desc, th: int = 10,
                               skip=None, mp_ids=None, kf_matched=None):
        """Loop-closing SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
        (ORBmatcher.cc:293-406) through orbfe_search_by_projection_sim3, with the normalised
        [R|t] of Scw.  skip: isBad() || spAlreadyFound.count(pMP) per point; kf_matched: the
        keyframe's slots before the call (ids, -1 = NULL).  Returns (kf_matched, nmatches).  A
        predicted level outside the pyramid raises OrbfeError(ORBFE_ERR_UNSUPPORTED) carrying
        the valid results of every other point as ``.results``."""
        a = [np.ascontiguousarray(tcw, np.float32).reshape(12),
             np.ascontiguousarray(mp_xyz, np.float32).reshape(-1, 3),
             np.ascontiguousarray(mp_normal, np.float32).reshape(-1, 3),
             np.ascontiguousarray(mp_min_dist, np.float32),
             np.ascontiguousarray(mp_max_dist, np.float32),
             np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)]
        n = len(a[1])
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        ids = None if mp_ids is None else np.ascontiguousarray(mp_ids, np.int32)
        km = (np.full(kf.n, -1, np.int32) if kf_matched is None
              else np.ascontiguousarray(kf_matched, np.int32).copy())
        nm = C.c_int32(0)
        kv = kf.view()
        st = lib().orbfe_search_by_projection_sim3(
            self._h, C.byref(kv), ptr(a[0]), C.byref(cam), C.c_float(log_scale), n,
            *(ptr(x) for x in a[1:]), ptr(sk), ptr(ids), int(th), ptr(km), C.byref(nm))
        if st != ORBFE_OK:
            e = OrbfeError("orbfe_search_by_projection_sim3", st)
            e.results = (km, nm.value)
            raise e
        return km, nm.value

    def SearchBySim3(self, kf1: Frame, kf2: Frame, cam1: Camera, t1w, t2w, s12, s21,
                     log_scale1: float, log_scale2: float, pts1, pts2, th: float = 7.5):
        """SearchBySim3 (ORBmatcher.cc:1105-1329) through orbfe_search_by_sim3.  s12 / s21: the
        3 x 4 [sR12|t12] and [sR21|t21] of lines 1122-1124; pts*: per keyframe a tuple
        (search, xyz, min_dist, max_dist, desc) over its features, search[i] != 0 <=> the
        feature holds a point that is not bad and is not already matched.  Returns (match12,
        vnMatch1, vnMatch2, nFound).  A predicted level outside the target's pyramid raises
        OrbfeError(ORBFE_ERR_UNSUPPORTED) carrying the other results as ``.results``."""
        mats = [np.ascontiguousarray(x, np.float32).reshape(12) for x in (t1w, t2w, s12, s21)]
        p = []
        for kf, (search, xyz, mind, maxd, desc) in ((kf1, pts1), (kf2, pts2)):
            q = [np.ascontiguousarray(search, np.uint8),
                 np.ascontiguousarray(xyz, np.float32).reshape(-1, 3),
                 np.ascontiguousarray(mind, np.float32), np.ascontiguousarray(maxd, np.float32),
                 np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)]
            assert all(len(x) == kf.n for x in q)
            p += q
        m12 = np.full(kf1.n, -1, np.int32)
        vn1 = np.full(kf1.n, -1, np.int32)
        vn2 = np.full(kf2.n, -1, np.int32)
        nf = C.c_int32(0)
        v1, v2 = kf1.view(), kf2.view()
        st = lib().orbfe_search_by_sim3(
            self._h, C.byref(v1), C.byref(v2), C.byref(cam1), *(ptr(x) for x in mats),
            C.c_float(log_scale1), C.c_float(log_scale2), *(ptr(x) for x in p), C.c_float(th),
            ptr(m12), ptr(vn1), ptr(vn2), C.byref(nf))
        if st != ORBFE_OK:
            e = OrbfeError("orbfe_search_by_sim3", st)
            e.results = (m12, vn1, vn2, nf.value)
            raise e
        return m12, vn1, vn2, nf.value

    def SearchForTriangulation(self, KF1: Frame, has_mp1, fv1, KF2: Frame, has_mp2, fv2, F12,
                               epipole, level_sigma2, bOnlyStereo: bool = False,
                               block_matched2: bool = False):
        """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)
        (ORBmatcher.cc:660-826) through orbfe_search_for_triangulation.  has_mp*:
        GetMapPoint(i) != NULL per feature; fv*: (node_ids, node_off, feat) FeatureVectors; F12
        3 x 3; epipole (ex, ey) of lines 667-673; level_sigma2 = pKF2->mvLevelSigma2.
        block_matched2=False is the reference as written (vbMatched2 is never set, DESIGN.md
        H13), True its evident intent.  Returns (vMatchedPairs (n, 2) int32, nmatches);
        ``self.vMatches12`` keeps the per-feature array.  A node over 256 keyframe-2 features or
        an octave outside the pyramid raises OrbfeError carrying the valid results of everything
        else as ``.results``."""
        mp1 = np.ascontiguousarray(has_mp1, np.uint8)
        mp2 = np.ascontiguousarray(has_mp2, np.uint8)
        n1, o1, f1 = (np.ascontiguousarray(x, np.int32) for x in fv1)
        n2, o2, f2 = (np.ascontiguousarray(x, np.int32) for x in fv2)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        ep = np.ascontiguousarray(epipole, np.float32).reshape(2)
        sg = np.ascontiguousarray(level_sigma2, np.float32)
        assert len(mp1) == KF1.n and len(mp2) == KF2.n and len(sg) >= len(KF2.scale_factors)
        m12 = np.full(KF1.n, -1, np.int32)
        nm = C.c_int32(0)
        v1, v2 = KF1.view(), KF2.view()
        st = lib().orbfe_search_for_triangulation(
            self._h, int(self.mbCheckOrientation), int(bool(block_matched2)),
            int(bool(bOnlyStereo)), C.byref(v1), ptr(mp1), len(n1), ptr(n1), ptr(o1), ptr(f1),
            C.byref(v2), ptr(mp2), len(n2), ptr(n2), ptr(o2), ptr(f2), ptr(F), ptr(ep), ptr(sg),
            ptr(m12), C.byref(nm))
        self.vMatches12 = m12
        i1 = np.flatnonzero(m12 >= 0)
        pairs = np.stack([i1, m12[i1]], axis=1).astype(np.int32).reshape(-1, 2)
        if st != ORBFE_OK:
            e = OrbfeError("orbfe_search_for_triangulation", st)
            e.results = (pairs, nm.value)
            raise e
        return pairs, nm.value

    def search_for_triangulation_batch_device(self, cap: int, d_keys: int, d_desc: int,
                                              d_u_right: int | None, d_has_mp: int, d_n: int,
                                              d_nn: int, d_node_ids: int, d_node_off: int,
                                              d_feat: int, n_pairs: int, d_pair_1: int,
                                              d_pair_2: int, d_f12: int, d_epipole: int,
                                              scale_factors, level_sigma2, d_matches12: int,
                                              d_nmatches: int, d_status: int,
                                              bOnlyStereo: bool = False,
                                              block_matched2: bool = False) -> None:
        """SearchForTriangulation over n_pairs (keyframe-1 slot, keyframe-2 slot) pairs
        (CreateNewMapPoints' neighbour loop, LocalMapping.cc:215-268): device pointers in the
        layout of Vocabulary.transform_batch_device plus keypoint, mvuRight and map-point-flag
        slabs (orbfe_search_for_triangulation_batch_device); scale_factors / level_sigma2 on the
        host.  Asynchronous on the matcher's stream."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        sg = np.ascontiguousarray(level_sigma2, np.float32)
        assert len(sg) >= len(sf)
        vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        _check("orbfe_search_for_triangulation_batch_device",
               lib().orbfe_search_for_triangulation_batch_device(
                   self._h, int(self.mbCheckOrientation), int(bool(block_matched2)),
                   int(bool(bOnlyStereo)), cap, vp(d_keys), vp(d_desc), vp(d_u_right),
                   vp(d_has_mp), vp(d_n), vp(d_nn), vp(d_node_ids), vp(d_node_off), vp(d_feat),
                   n_pairs, vp(d_pair_1), vp(d_pair_2), vp(d_f12), vp(d_epipole), ptr(sf),
                   ptr(sg), len(sf), vp(d_matches12), vp(d_nmatches), vp(d_status)))

    def is_in_frustum(self, xyz, normal, min_dist, max_dist, tcw, cam: Camera, bounds,
                      log_scale: float, cos_limit: float = 0.5, out=None):
        """Frame::isInFrustum + MapPoint::PredictScale over all map points (Frame.cc:387).
        out: the six output arrays (in_view u8, proj_x, proj_y, proj_xr f32, pred_level i32,
        view_cos f32) to write into; in_view is written for every point, the other five only
        for a point in view -- a rejected point keeps what they held, as mTrackProj* do."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        normal = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        mn = np.ascontiguousarray(min_dist, np.float32)
        mx = np.ascontiguousarray(max_dist, np.float32)
        t = np.ascontiguousarray(tcw, np.float32).reshape(12)
        if out is not None:
            inv, px, py, pxr, pl, vc = out
            for o, dt in zip(out, (np.uint8, np.float32, np.float32, np.float32, np.int32,
                                   np.float32)):
                assert o.dtype == dt and o.shape == (n,) and o.flags["C_CONTIGUOUS"]
        else:
            inv = np.zeros(n, np.uint8)
            px, py, pxr, vc = (np.zeros(n, np.float32) for _ in range(4))
            pl = np.zeros(n, np.int32)
        _check("orbfe_is_in_frustum", lib().orbfe_is_in_frustum(
            self._h, n, ptr(xyz), ptr(normal), ptr(mn), ptr(mx), ptr(t), C.byref(cam),
            *(C.c_float(b) for b in bounds), C.c_float(log_scale), C.c_float(cos_limit),
            ptr(inv), ptr(px), ptr(py), ptr(pxr), ptr(pl), ptr(vc)))
        return inv, px, py, pxr, pl, vc

    def ClosePoints(self, mode: int, keys_un, depth, has_point, cam: Camera, rwc_ow,
                    th_depth: float, scale_factors=None, min_points: int = 100, out=None,
                    results: bool = False):
        """The close-point rule over mvDepth with Frame::UnprojectStereo (orbfe_close_points):
        mode CLOSE_SORTED is the loop of Tracking::UpdateLastFrame / CreateNewKeyFrame
        (Tracking.cc:1059-1111, 1333-1392), CLOSE_ALL is StereoInitialization (764-779).
        has_point[i] = mvpMapPoints[i] && Observations() >= 1; rwc_ow = mRwc (row-major) then
        mOw.  scale_factors None leaves the MapPoint distances out.  Returns a dict: order,
        create, xyz (n_visited rows), max_dist / min_dist (or None), n_visited, n_total, n_map,
        status.  out: the five arrays (order i32, create u8, xyz f32 (n, 3), max_dist, min_dist
        f32) to write into; the call touches only their first n_visited entries."""
        keys_un = np.ascontiguousarray(keys_un, KEYPOINT_DTYPE)
        n = len(keys_un)
        depth = np.ascontiguousarray(depth, np.float32)
        hp = None if has_point is None else np.ascontiguousarray(has_point, np.uint8)
        assert len(depth) == n and (hp is None or len(hp) == n)
        pose = np.ascontiguousarray(rwc_ow, np.float32).reshape(12)
        sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, np.float32)
        if out is not None:
            order, create, xyz, mx, mn = out
        else:
            order = np.zeros(n, np.int32)
            create = np.zeros(n, np.uint8)
            xyz = np.zeros((n, 3), np.float32)
            mx = None if sf is None else np.zeros(n, np.float32)
            mn = None if sf is None else np.zeros(n, np.float32)
        cnt = np.zeros(3, np.int32)
        st = lib().orbfe_close_points(
            self._h, mode, ptr(keys_un), ptr(depth), ptr(hp), n, C.addressof(cam), ptr(pose),
            th_depth, min_points, ptr(sf), 0 if sf is None else len(sf), ptr(order),
            cnt[0:].ctypes.data, ptr(create), ptr(xyz), ptr(mx), ptr(mn), cnt[1:].ctypes.data,
            cnt[2:].ctypes.data)
        if not (results and st in (ORBFE_ERR_UNSUPPORTED, ORBFE_ERR_CAPACITY)):
            _check("orbfe_close_points", st)
        v = int(cnt[0])
        return {"order": order[:v], "create": create[:v], "xyz": xyz[:v],
                "max_dist": None if mx is None else mx[:v],
                "min_dist": None if mn is None else mn[:v], "n_visited": v,
                "n_total": int(cnt[1]), "n_map": int(cnt[2]), "status": st}

    def close_points_batch_device(self, mode: int, n_frames: int, d_keys_un: int, d_depth: int,
                                  d_has_point: int | None, d_n: int, kps_cap: int, cam: Camera,
                                  d_rwc_ow: int, th_depth: float, min_points: int, scale_factors,
                                  d_order: int, d_n_visited: int, d_create: int, d_xyz: int,
                                  d_max_dist: int | None, d_min_dist: int | None, d_n_total: int,
                                  d_n_map: int, d_status: int) -> None:
        """Batched device form (orbfe_close_points_batch_device): slabs of kps_cap entries per
        frame, a pose per frame, outputs left on the device; async."""
        sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, np.float32)
        _check("orbfe_close_points_batch_device", lib().orbfe_close_points_batch_device(
            self._h, mode, n_frames, d_keys_un, d_depth, d_has_point, d_n, kps_cap,
            C.addressof(cam), d_rwc_ow, th_depth, min_points, ptr(sf),
            0 if sf is None else len(sf), d_order, d_n_visited, d_create, d_xyz, d_max_dist,
            d_min_dist, d_n_total, d_n_map, d_status))
