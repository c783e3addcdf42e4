"""ctypes binding of the C-ABI in include/srukf.h (libsrukf_hip.so, gfx950 kernels).

This is host plumbing only: every numeric result comes from the HIP kernels.  There is no CPU
fallback — if the library or a gfx950 device is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsrukf_hip.so")

_DBL_FIELDS = ["cam_dx", "cam_dy", "cam_cx", "cam_cy", "cam_k1", "cam_k2", "cam_f", "image_w", "image_h",
               "a1", "a2", "a3", "a4", "sigma_measure", "rho0", "sigma_rho", "sigma_x", "sigma_y", "sigma_z",
               "sigma_theta", "epsilon", "ut_alpha", "ut_beta"]
_INT_FIELDS = ["weight_type", "noise_type", "newton_iters", "reserved_"]

# names of every entry point declared in include/srukf.h (checked by the CPU test-suite)
EXPORTS = [
    "srukf_abi_version", "srukf_default_params", "srukf_create", "srukf_destroy", "srukf_reset", "srukf_last_error",
    "srukf_set_state", "srukf_get_state", "srukf_set_state_device", "srukf_get_state_device", "srukf_get_robot",
    "srukf_get_landmark_block", "srukf_get_landmarks_cartesian", "srukf_get_frame_view", "srukf_get_covariance", "srukf_predict_motion", "srukf_predict_motion_next", "srukf_predict_measurement",
    "srukf_update", "srukf_update_joint", "srukf_set_new_landmarks", "srukf_add_landmarks", "srukf_delete_landmark", "srukf_set_storage", "srukf_set_exclusive", "srukf_set_rank_aware", "srukf_null_directions", "srukf_run_frames_batch", "srukf_prepare_frames", "srukf_prepare_frames_mode", "srukf_debug_poke_state", "srukf_get_state_f32", "srukf_set_landmark_appearance", "srukf_associate", "srukf_get_match_patch", "srukf_stage_sequence", "srukf_run_frames_async", "srukf_run_frames", "srukf_synchronize", "srukf_set_profiling",
    "srukf_clamp_info", "srukf_debug_set", "srukf_debug_switch_at", "srukf_debug_get", "srukf_debug_copy", "srukf_debug_upload", "srukf_debug_split_replay", "srukf_debug_gmw_stamps", "srukf_debug_starve_workers", "srukf_debug_allow_mixed", "srukf_profile_count", "srukf_profile_get", "srukf_profile_reset", "srukf_dims", "srukf_gmw_host",
    "srukf_project_host", "srukf_detect_features", "srukf_capture_appearance", "srukf_get_landmark_record", "srukf_insert_landmarks",
    "srukf_ransac_consensus", "srukf_repredict_measurement",
    "srukf_get_landmarks_display", "srukf_get_frame_view_display",
    "srukf_set_frame_bgr", "srukf_associate_held", "srukf_render_overlay",
    "srukf_archive_set", "srukf_archive_count", "srukf_archive_get_template", "srukf_archive_search",
    "srukf_associate_checked", "srukf_get_match_scores",
    "srukf_stage_images", "srukf_run_images_async", "srukf_run_images", "srukf_get_image_matches",
    "srukf_run_images_checked_async", "srukf_run_images_checked", "srukf_get_image_checks",
    "srukf_images_search_archive", "srukf_get_image_archive",
    "srukf_map_policy", "srukf_images_policy", "srukf_images_set_policy_state", "srukf_get_image_policy", "srukf_images_rewind",
    "srukf_images_ransac", "srukf_get_image_ransac",
    "srukf_images_snapshots", "srukf_get_image_snapshots", "srukf_images_resume",
    "srukf_images_display", "srukf_get_image_display", "srukf_render_image_overlay",
    "srukf_images_rescue_gate", "srukf_get_image_rescue", "srukf_rescue_gate",
    "srukf_delete_landmarks",
    "srukf_stage_images_bgr", "srukf_get_staged_image", "srukf_render_image_overlays",
]

STATUS = {0: "SRUKF_OK", -1: "SRUKF_ERR_BAD_ARG", -2: "SRUKF_ERR_DIM_MISMATCH", -3: "SRUKF_ERR_HIP",
          -4: "SRUKF_ERR_NO_DEVICE", -5: "SRUKF_ERR_SEQUENCE", -6: "SRUKF_ERR_UNSUPPORTED",
          -7: "SRUKF_ERR_CLAMP_PENDING", -8: "SRUKF_ERR_NOMEM"}

STORAGE_F64, STORAGE_F32, STORAGE_F32_MIXED = 0, 1, 2
GPU_SHARED, GPU_EXCLUSIVE, GPU_SHARED_PER_PANEL = 0, 1, 2          # srukf_set_exclusive
UPDATE_SEQUENTIAL, UPDATE_BATCHED, UPDATE_JOINT = 0, 1, 2          # UPDATE_JOINT: the staged replay only (run_frames*, prepare_frames); step-wise: update_joint
NEED_REORDER, NEEDNOT_REORDER = 0, 1


class Params(C.Structure):
    """struct srukf_params."""
    _fields_ = [(k, C.c_double) for k in _DBL_FIELDS] + [(k, C.c_int) for k in _INT_FIELDS]

    @classmethod
    def from_dict(cls, d):
        p = cls()
        for k in _DBL_FIELDS:
            setattr(p, k, float(d[k]))
        for k in _INT_FIELDS:
            setattr(p, k, int(d.get(k, 0)))
        return p

    def to_dict(self):
        return {k: getattr(self, k) for k in _DBL_FIELDS + _INT_FIELDS}


class DetectParams(C.Structure):
    """struct srukf_detect_params (defaults: SLAM.cpp:175-181, 48)."""
    _fields_ = [("max_corners", C.c_int), ("quality_level", C.c_double), ("min_dist", C.c_double), ("block_size", C.c_int),
                ("dist_to_border", C.c_double), ("unfiltered", C.c_int), ("map_gate", C.c_int), ("project_archived", C.c_int)]


class ArchiveParams(C.Structure):
    """struct srukf_archive_params."""
    _fields_ = [("half_cap", C.c_int), ("corr_threshold", C.c_double), ("chi2", C.c_double)]


class MatchParams(C.Structure):
    """struct srukf_match_params."""
    _fields_ = [("corr_threshold", C.c_double), ("ratio", C.c_double), ("exclusion", C.c_int), ("subpixel", C.c_int)]


class PolicyParams(C.Structure):
    """struct srukf_policy_params."""
    _fields_ = [("border", C.c_double), ("rho_min", C.c_double), ("min_predictions", C.c_int), ("min_matches", C.c_int)]


POLICY_SUMMARY_FIELDS = ("n_predicts", "n_matches", "n_deletes", "n_stores", "n_predicts_after", "n_matches_after", "need_add", "change")


class PolicySummary(C.Structure):
    """struct srukf_policy_summary."""
    _fields_ = [(k, C.c_int) for k in POLICY_SUMMARY_FIELDS]


# struct srukf_policy_state / srukf_policy_summary as numpy records; the verdict bits
POLICY_STATE_DTYPE = np.dtype([("nPredictTimes", np.int32), ("nMatchTimes", np.int32), ("predictLocation", np.float64, (2,))])
POLICY_SUMMARY_DTYPE = np.dtype([(k, np.int32) for k in POLICY_SUMMARY_FIELDS])
POLICY_UNMATCHED, POLICY_RHO, POLICY_BEHIND, POLICY_PRED_BORDER, POLICY_MATCH_BORDER, POLICY_STORE = 1, 2, 4, 8, 16, 32


class SrukfError(RuntimeError):
    def __init__(self, rc, msg=""):
        self.rc = rc
        super().__init__(f"{STATUS.get(rc, rc)}: {msg}")


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None


def load_library(path=None):
    """dlopen the in-tree libsrukf_hip.so; raises if it has not been built (no fallback).
    path: measurement scripts only (bench.py --lib, scripts/ab_bench.sh) — an A/B build of the same library, named on the FIRST call; the product reads no
    environment variable and loads nothing else."""
    global _lib, LIB_PATH
    if _lib is not None:
        if path and os.path.abspath(path) != os.path.abspath(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is already loaded; an A/B library must be named on the first load_library call")
        return _lib
    if path:
        LIB_PATH = path
    # PyTorch-ROCm bundles its own libamdhip64.so; if ours (linked against /opt/rocm) initialises
    # HIP first, a later `import torch` in the same process finds no GPUs.  Loading torch first
    # makes both share one runtime.  torch is plumbing here (streams / RCCL), never compute.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.srukf_last_error.restype = C.c_char_p
    L.srukf_last_error.argtypes = [C.c_void_p]
    L.srukf_default_params.argtypes = [C.POINTER(Params)]
    L.srukf_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Params), C.c_int, C.c_void_p]
    L.srukf_destroy.argtypes = [C.c_void_p]
    L.srukf_reset.argtypes = [C.c_void_p]
    L.srukf_set_state.argtypes = [C.c_void_p, _dp, _dp]
    L.srukf_get_state.argtypes = [C.c_void_p, _dp, _dp]
    L.srukf_set_state_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.srukf_get_state_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.srukf_get_robot.argtypes = [C.c_void_p, _dp, _dp]
    L.srukf_get_landmark_block.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.srukf_get_covariance.argtypes = [C.c_void_p, _dp]
    L.srukf_get_landmarks_cartesian.argtypes = [C.c_void_p, _dp, _dp]
    L.srukf_get_frame_view.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp]
    L.srukf_get_landmarks_display.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]
    L.srukf_get_frame_view_display.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
    L.srukf_predict_motion.argtypes = [C.c_void_p, _dp, _dp]
    L.srukf_predict_motion_next.argtypes = [C.c_void_p, _dp, _dp]
    L.srukf_predict_measurement.argtypes = [C.c_void_p, _dp, _dp, _ip]
    L.srukf_update.argtypes = [C.c_void_p, _dp, _ip, C.c_int, C.c_int]
    L.srukf_update_joint.argtypes = [C.c_void_p, _dp, _ip, C.c_int]
    L.srukf_set_new_landmarks.argtypes = [C.c_void_p, C.c_int]
    L.srukf_add_landmarks.argtypes = [C.c_void_p, C.c_int, _dp]
    L.srukf_delete_landmark.argtypes = [C.c_void_p, C.c_int]
    _bp = C.POINTER(C.c_ubyte)
    if hasattr(L, "srukf_delete_landmarks"):           # (an A/B build of an older library, bench.py --lib, deletes one landmark per call)
        L.srukf_delete_landmarks.argtypes = [C.c_void_p, C.c_int, _ip, _dp, _dp, _bp, _dp, _dp, _dp, _ip]
    L.srukf_set_landmark_appearance.argtypes = [C.c_void_p, C.c_int, _bp, _dp, _dp, _dp]
    L.srukf_associate.argtypes = [C.c_void_p, _bp, _dp, _ip, _dp]
    L.srukf_get_match_patch.argtypes = [C.c_void_p, C.c_int, _bp]
    if hasattr(L, "srukf_detect_features"):            # (an A/B build of an older library, bench.py --lib, has no detection: build() checks EXPORTS)
        L.srukf_detect_features.argtypes = [C.c_void_p, _bp, C.POINTER(DetectParams), C.c_int, _dp, C.c_int, _dp, _dp, C.c_int, _ip, _ip, C.c_int, _ip]
        L.srukf_capture_appearance.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _bp]
    if hasattr(L, "srukf_insert_landmarks"):           # (idem: loop points)
        L.srukf_get_landmark_record.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _bp, _dp, _dp, _dp, _ip]
        L.srukf_insert_landmarks.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _bp, _dp, _dp, _dp]
    if hasattr(L, "srukf_ransac_consensus"):           # (idem: 1-point RANSAC)
        L.srukf_ransac_consensus.argtypes = [C.c_void_p, _dp, _ip, C.c_double, _ip, _ip, _dp, _ip]
        L.srukf_repredict_measurement.argtypes = [C.c_void_p, _dp, _dp, _ip]
    if hasattr(L, "srukf_render_overlay"):             # (idem: colour-frame intake, 2-D overlay)
        L.srukf_set_frame_bgr.argtypes = [C.c_void_p, _bp, _bp]
        L.srukf_associate_held.argtypes = [C.c_void_p, _dp, _ip, _dp]
        L.srukf_render_overlay.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip, _bp]
    if hasattr(L, "srukf_archive_search"):             # (idem: archive search by appearance)
        L.srukf_archive_set.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _bp, _dp, _dp, _dp]
        L.srukf_archive_count.argtypes = [C.c_void_p]
        L.srukf_archive_get_template.argtypes = [C.c_void_p, C.c_int, _bp]
        L.srukf_archive_search.argtypes = [C.c_void_p, _bp, C.POINTER(ArchiveParams), _dp, _dp, _ip, _dp, _ip, _dp]
    if hasattr(L, "srukf_associate_checked"):          # (idem: ambiguity veto, sub-pixel matches)
        L.srukf_associate_checked.argtypes = [C.c_void_p, _bp, C.POINTER(MatchParams), _dp, _ip, _dp, _dp, _dp, _ip]
        L.srukf_get_match_scores.argtypes = [C.c_void_p, C.c_int, _dp, _ip, _ip, _ip, _ip]
    if hasattr(L, "srukf_run_images"):                 # (idem: image runs of the staged replay)
        L.srukf_stage_images.argtypes = [C.c_void_p, C.c_int, _bp]
        L.srukf_run_images_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.srukf_run_images.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp]
        L.srukf_get_image_matches.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _ip, _dp, _ip, _dp]
    if hasattr(L, "srukf_run_images_checked"):         # (idem: checked image runs)
        L.srukf_run_images_checked_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(MatchParams), C.c_void_p]
        L.srukf_run_images_checked.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(MatchParams), _dp]
        L.srukf_get_image_checks.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _ip]
    if hasattr(L, "srukf_images_search_archive"):
        L.srukf_images_search_archive.argtypes = [C.c_void_p, C.c_int, C.POINTER(ArchiveParams)]
        L.srukf_get_image_archive.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _dp, _dp, _ip, _dp, _ip, _dp, _ip]
    if hasattr(L, "srukf_map_policy"):
        L.srukf_map_policy.argtypes = [C.c_void_p, C.POINTER(PolicyParams), C.c_void_p, _dp, _ip, _dp, _ip, _ip, C.POINTER(PolicySummary)]
        L.srukf_images_policy.argtypes = [C.c_void_p, C.c_int, C.POINTER(PolicyParams)]
        L.srukf_images_set_policy_state.argtypes = [C.c_void_p, C.c_void_p]
        L.srukf_get_image_policy.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, C.c_void_p, C.c_void_p, _ip]
        L.srukf_images_rewind.argtypes = [C.c_void_p]
    if hasattr(L, "srukf_images_ransac"):              # (idem: the 1-point RANSAC consensus inside image frames)
        L.srukf_images_ransac.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.srukf_get_image_ransac.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _dp, _ip, _ip, _ip, _ip]
    if hasattr(L, "srukf_images_snapshots"):           # (idem: the state at a block's stop)
        L.srukf_images_snapshots.argtypes = [C.c_void_p, C.c_int]
        L.srukf_get_image_snapshots.argtypes = [C.c_void_p, _ip]
        L.srukf_images_resume.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "srukf_images_display"):             # (idem: the display view behind image frames, the overlay of a staged frame)
        L.srukf_images_display.argtypes = [C.c_void_p, C.c_int]
        L.srukf_get_image_display.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _dp]
        L.srukf_render_image_overlay.argtypes = [C.c_void_p, C.c_int, _bp]
    if hasattr(L, "srukf_stage_images_bgr"):           # (idem: colour frames in the staged stack, the overlays of a run of frames)
        L.srukf_stage_images_bgr.argtypes = [C.c_void_p, C.c_int, _bp, C.c_int]
        L.srukf_get_staged_image.argtypes = [C.c_void_p, C.c_int, _bp, _bp]
        L.srukf_render_image_overlays.argtypes = [C.c_void_p, C.c_int, C.c_int, _bp]
    if hasattr(L, "srukf_images_rescue_gate"):         # (idem: the rescue gate on the device)
        L.srukf_images_rescue_gate.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.srukf_get_image_rescue.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip]
        L.srukf_rescue_gate.argtypes = [C.c_void_p, _dp, _ip, _ip, C.c_double, _ip, _dp, _dp, _dp, _ip]
    L.srukf_set_storage.argtypes = [C.c_void_p, C.c_int]
    L.srukf_set_exclusive.argtypes = [C.c_void_p, C.c_int]
    L.srukf_set_rank_aware.argtypes = [C.c_void_p, C.c_int]
    L.srukf_prepare_frames.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "srukf_prepare_frames_mode"):        # (idem: the joint update as a mode of the staged replay)
        L.srukf_prepare_frames_mode.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.srukf_debug_poke_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
    L.srukf_run_frames_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.srukf_null_directions.argtypes = [C.c_void_p]
    L.srukf_get_state_f32.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.srukf_stage_sequence.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip]
    L.srukf_run_frames_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.srukf_run_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp]
    L.srukf_synchronize.argtypes = [C.c_void_p]
    L.srukf_clamp_info.argtypes = [C.c_void_p, _ip, _ip]
    L.srukf_debug_starve_workers.argtypes = [C.c_void_p, C.c_int]
    L.srukf_debug_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.srukf_debug_switch_at.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), _ip, _ip, _ip]
    L.srukf_debug_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_longlong)]
    L.srukf_debug_copy.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.c_longlong]
    L.srukf_debug_upload.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.c_longlong]
    L.srukf_debug_split_replay.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.srukf_debug_gmw_stamps.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    L.srukf_debug_allow_mixed.argtypes = [C.c_void_p, C.c_int]
    L.srukf_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.srukf_profile_count.argtypes = [C.c_void_p]
    L.srukf_profile_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), _dp, C.POINTER(C.c_longlong), _dp, _dp]
    L.srukf_profile_reset.argtypes = [C.c_void_p]
    L.srukf_dims.argtypes = [C.c_void_p, _ip, _ip, _ip, _ip]
    L.srukf_gmw_host.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int, _ip]
    L.srukf_project_host.argtypes = [C.c_int, C.POINTER(Params), C.c_int, _dp, _dp, _dp, _dp, _dp]
    _lib = L
    return L


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _i(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


def default_params():
    p = Params()
    load_library().srukf_default_params(C.byref(p))
    return p.to_dict()


class Filter:
    """One SRUKF on one MI355X (mirror of the numeric side of CSLAM, SLAM.h:118-398)."""

    def __init__(self, n_landmarks, params, device=0, stream=None):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.params = Params.from_dict(params)
        rc = self._lib.srukf_create(C.byref(self._h), n_landmarks, C.byref(self.params), device,
                                    C.c_void_p(stream) if stream else None)
        if rc != 0:
            msg = self._lib.srukf_last_error(None)
            self._h = None
            raise SrukfError(rc, msg.decode() if msg else "")
        self._refresh_dims()

    def _refresh_dims(self):
        N, n, Na, L = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._lib.srukf_dims(self._h, C.byref(N), C.byref(n), C.byref(Na), C.byref(L))
        self.N, self.n, self.Na, self.L = N.value, n.value, Na.value, L.value

    def _chk(self, rc):
        if rc != 0:
            msg = self._lib.srukf_last_error(self._h)
            raise SrukfError(rc, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.srukf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._chk(self._lib.srukf_reset(self._h))

    def set_state(self, X, S):
        X, S = _c(X), _c(S)
        assert X.shape == (self.n,) and S.shape == (self.n, self.n)
        self._chk(self._lib.srukf_set_state(self._h, _d(X), _d(S)))

    def get_state(self):
        X, S = np.empty(self.n), np.empty((self.n, self.n))
        self._chk(self._lib.srukf_get_state(self._h, _d(X), _d(S)))
        return X, S

    def set_state_device(self, dX_ptr, dS_ptr, ld):
        self._chk(self._lib.srukf_set_state_device(self._h, C.c_void_p(dX_ptr), C.c_void_p(dS_ptr), ld))

    def get_state_device(self, dX_ptr, dS_ptr, ld):
        self._chk(self._lib.srukf_get_state_device(self._h, C.c_void_p(dX_ptr), C.c_void_p(dS_ptr), ld))

    def get_robot(self):
        pose, P4 = np.empty(4), np.empty((4, 4))
        self._chk(self._lib.srukf_get_robot(self._h, _d(pose), _d(P4)))
        return pose, P4

    def get_landmark_block(self, k):
        x6, P = np.empty(6), np.empty((6, 6))
        self._chk(self._lib.srukf_get_landmark_block(self._h, k, _d(x6), _d(P)))
        return x6, P

    def get_covariance(self):
        P = np.empty((self.n, self.n))
        self._chk(self._lib.srukf_get_covariance(self._h, _d(P)))
        return P

    def predict_motion(self, odo_prev, odo_cur):
        a, b = _c(odo_prev), _c(odo_cur)
        self._chk(self._lib.srukf_predict_motion(self._h, _d(a), _d(b)))

    def predict_motion_next(self, odo_prev, odo_cur):
        """Look-ahead: the odometry pair of the NEXT frame (srukf_predict_motion_next)."""
        a, b = _c(odo_prev), _c(odo_cur)
        self._chk(self._lib.srukf_predict_motion_next(self._h, _d(a), _d(b)))

    def predict_measurement(self):
        h, Si, vis = np.empty(2 * self.N), np.empty((self.N, 2, 2)), np.empty(self.N, dtype=np.int32)
        self._chk(self._lib.srukf_predict_measurement(self._h, _d(h), _d(Si), _i(vis)))
        return h, Si, vis

    def update(self, z, matched, reorder=NEEDNOT_REORDER, mode=UPDATE_BATCHED):
        z, m = _c(z), _c(matched, np.int32)
        assert z.shape == (2 * self.N,) and m.shape == (self.N,)
        self._chk(self._lib.srukf_update(self._h, _d(z), _i(m), reorder, mode))

    def update_joint(self, z, matched, reorder=NEEDNOT_REORDER):
        """One Kalman update over all of the frame's matches with the full innovation covariance (srukf_update_joint)."""
        z, m = _c(z), _c(matched, np.int32)
        assert z.shape == (2 * self.N,) and m.shape == (self.N,)
        self._chk(self._lib.srukf_update_joint(self._h, _d(z), _i(m), reorder))

    def ransac_consensus(self, z, matched, threshold=8.0):
        """1-point RANSAC consensus over ALL single-match hypotheses (srukf_ransac_consensus), between predict_measurement and update.
        Returns (inlier[N], votes[N], dist[N], best); best = -1 when no matched landmark is visible.  The filter is not changed."""
        z, m = _c(z), _c(matched, np.int32)
        assert z.shape == (2 * self.N,) and m.shape == (self.N,)
        inl, votes, dist, best = np.zeros(self.N, dtype=np.int32), np.zeros(self.N, dtype=np.int32), np.zeros(self.N), C.c_int(-1)
        self._chk(self._lib.srukf_ransac_consensus(self._h, _d(z), _i(m), float(threshold), _i(inl), _i(votes), _d(dist), C.byref(best)))
        return inl, votes, dist, best.value

    def repredict_measurement(self):
        """predict_measurement once more from the posterior of the update just made (srukf_repredict_measurement); a second update may follow."""
        h, Si, vis = np.empty(2 * self.N), np.empty((self.N, 2, 2)), np.empty(self.N, dtype=np.int32)
        self._chk(self._lib.srukf_repredict_measurement(self._h, _d(h), _d(Si), _i(vis)))
        return h, Si, vis

    def rescue_gate(self, z, matched, inlier, chi2=5.99146454710798):
        """The rescue gate after an update of this frame (srukf_rescue_gate): for the matches the consensus dropped (matched and not inlier,
        in a frame with at least two matches of which some but not all are inliers), repredict_measurement's h, Si from the posterior and the chi-square test, in
        one launch that changes neither state nor phase.  Returns dict of flags[N] (bit 0 candidate, bit 1 rescued), h2[2N], Si2[N, 2, 2], chi2[N], n_high."""
        z, m, inl = _c(z), _c(matched, np.int32), _c(inlier, np.int32)
        assert z.shape == (2 * self.N,) and m.shape == (self.N,) and inl.shape == (self.N,)
        if isinstance(chi2, bool) or not isinstance(chi2, (int, float, np.integer, np.floating)):
            raise TypeError("rescue_gate: chi2 must be a real number")
        out = dict(flags=np.zeros(self.N, dtype=np.int32), h2=np.zeros(2 * self.N), Si2=np.zeros((self.N, 2, 2)), chi2=np.zeros(self.N))
        nh = C.c_int(0)
        self._chk(self._lib.srukf_rescue_gate(self._h, _d(z), _i(m), _i(inl), float(chi2), _i(out["flags"]), _d(out["h2"]), _d(out["Si2"]), _d(out["chi2"]), C.byref(nh)))
        out["n_high"] = int(nh.value)
        return out

    def set_new_landmarks(self, K_new):
        """m_nFilters: the last K_new landmarks of the map were just added (NEED_REORDER updates use it)."""
        self._chk(self._lib.srukf_set_new_landmarks(self._h, int(K_new)))

    def add_landmarks(self, uv):
        """Joint initialisation of K new landmarks at distorted pixels uv[K][2]; the filter grows to N + K."""
        uv = _c(uv).reshape(-1, 2)
        self._chk(self._lib.srukf_add_landmarks(self._h, uv.shape[0], _d(uv)))
        self._refresh_dims()

    def get_landmarks_cartesian(self):
        """(xyz[N,3], cov[N,3,3]) of every landmark: getFeatureCartesianInformation batched on the device."""
        xyz, cov = np.zeros((self.N, 3)), np.zeros((self.N, 3, 3))
        self._chk(self._lib.srukf_get_landmarks_cartesian(self._h, _d(xyz), _d(cov)))
        return xyz, cov

    def get_frame_view(self):
        """(X, xyz[N,3], cov[N,3,3], pose[4], P4[4,4]) in one device round trip (srukf_get_frame_view)."""
        X, xyz, cov, pose, P4 = np.zeros(self.n), np.zeros((self.N, 3)), np.zeros((self.N, 3, 3)), np.zeros(4), np.zeros((4, 4))
        self._chk(self._lib.srukf_get_frame_view(self._h, _d(X), _d(xyz), _d(cov), _d(pose), _d(P4)))
        return X, xyz, cov, pose, P4

    def get_landmarks_display(self):
        """(xyz[N,3], cov[N,3,3], axis[N,4], sigma[N,3], rot[N]): get_landmarks_cartesian plus the display ellipsoid of every covariance (quaternion
        (r, x, y, z) of the Jacobi eigenvectors, unsorted 1-sigma semi-axes, plane rotations applied or -1) from the device (srukf_get_landmarks_display)."""
        xyz, cov, axis, sigma = np.zeros((self.N, 3)), np.zeros((self.N, 3, 3)), np.zeros((self.N, 4)), np.zeros((self.N, 3))
        rot = np.zeros(self.N, dtype=np.int32)
        self._chk(self._lib.srukf_get_landmarks_display(self._h, _d(xyz), _d(cov), _d(axis), _d(sigma), _i(rot)))
        return xyz, cov, axis, sigma, rot

    def get_frame_view_display(self):
        """(X, xyz[N,3], cov[N,3,3], axis[N,4], sigma[N,3], pose[4], P4[4,4]): get_frame_view plus the ellipsoids in one round trip (srukf_get_frame_view_display)."""
        X, xyz, cov, pose, P4 = np.zeros(self.n), np.zeros((self.N, 3)), np.zeros((self.N, 3, 3)), np.zeros(4), np.zeros((4, 4))
        axis, sigma = np.zeros((self.N, 4)), np.zeros((self.N, 3))
        self._chk(self._lib.srukf_get_frame_view_display(self._h, _d(X), _d(xyz), _d(cov), _d(axis), _d(sigma), _d(pose), _d(P4)))
        return X, xyz, cov, axis, sigma, pose, P4

    def set_landmark_appearance(self, k, patch, R, t, px):
        """PointsMap::initPatch (21x21 uint8), initRotation (3x3), initTrans (3), initPixel (2) of landmark k."""
        patch = np.ascontiguousarray(patch, dtype=np.uint8); assert patch.shape == (21, 21)
        self._chk(self._lib.srukf_set_landmark_appearance(self._h, int(k), patch.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                          _d(_c(R).reshape(9)), _d(_c(t).reshape(3)), _d(_c(px).reshape(2))))

    def associate(self, gray):
        """wrapPatch + dataAssociation on the device; returns (z[2N], matched[N], corr[N])."""
        gray = np.ascontiguousarray(gray, dtype=np.uint8)
        z, m, cr = np.zeros(2 * self.N), np.zeros(self.N, dtype=np.int32), np.zeros(self.N)
        self._chk(self._lib.srukf_associate(self._h, gray.ctypes.data_as(C.POINTER(C.c_ubyte)), _d(z), _i(m), _d(cr)))
        return z, m, cr

    def set_frame_bgr(self, bgr, want_gray=True):
        """loadPictures on the device (srukf_set_frame_bgr): bgr[image_h, image_w, 3] uint8 (B, G, R) becomes the held colour frame, its conversion
        (the reference's: the blue byte gets 0.299) the held gray frame.  Returns the gray frame [image_h, image_w] (None with want_gray=False)."""
        h, w = int(self.params.image_h), int(self.params.image_w)
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        assert bgr.shape == (h, w, 3)
        gray = np.zeros((h, w), dtype=np.uint8) if want_gray else None
        self._chk(self._lib.srukf_set_frame_bgr(self._h, bgr.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                gray.ctypes.data_as(C.POINTER(C.c_ubyte)) if want_gray else None))
        return gray

    def associate_held(self):
        """associate() on the frame the filter holds (srukf_associate_held): no upload.  Returns (z[2N], matched[N], corr[N])."""
        z, m, cr = np.zeros(2 * self.N), np.zeros(self.N, dtype=np.int32), np.zeros(self.N)
        self._chk(self._lib.srukf_associate_held(self._h, _d(z), _i(m), _d(cr)))
        return z, m, cr

    def associate_checked(self, gray=None, corr_threshold=0.8, ratio=0.9, exclusion=4, subpixel=False):
        """associate() (gray = None: associate_held()) with the score map kept (srukf_associate_checked): a match whose second peak reaches ratio * the best
        is vetoed, subpixel=True refines the best peak by the parabola through its 4-neighbours.  Returns a dict of arrays: z[2N], matched[N], corr[N],
        corr2[N], z2[2N], flags[N] (bit 0 raw, bit 1 ambiguous, bit 2 refined)."""
        N = self.N
        g = None
        if gray is not None:
            gray = np.ascontiguousarray(gray, dtype=np.uint8)
            assert gray.shape == (int(self.params.image_h), int(self.params.image_w))
            g = gray.ctypes.data_as(C.POINTER(C.c_ubyte))
        mp = MatchParams(float(corr_threshold), float(ratio), int(exclusion), int(bool(subpixel)))
        out = dict(z=np.zeros(2 * N), matched=np.zeros(N, dtype=np.int32), corr=np.zeros(N), corr2=np.zeros(N), z2=np.zeros(2 * N),
                   flags=np.zeros(N, dtype=np.int32))
        self._chk(self._lib.srukf_associate_checked(self._h, g, C.byref(mp), _d(out["z"]), _i(out["matched"]), _d(out["corr"]), _d(out["corr2"]),
                                                    _d(out["z2"]), _i(out["flags"])))
        return out

    def match_scores(self, k):
        """(map[wy, wx], x0, y0): the score map the last associate_checked left for landmark k, (x0, y0) the pixel of its top-left candidate centre."""
        buf = np.zeros(441)
        wx, wy, x0, y0 = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self._lib.srukf_get_match_scores(self._h, int(k), _d(buf), C.byref(wx), C.byref(wy), C.byref(x0), C.byref(y0)))
        return buf[:wx.value * wy.value].reshape(wy.value, wx.value).copy(), x0.value, y0.value

    def render_overlay(self, h, Si, z, matched):
        """display2DFeatureModel on the device (srukf_render_overlay): the held frame with the predicted cross, the matched cross and the chi-square
        ellipse of every matched landmark, from the caller's h[2N], Si[4N], z[2N], matched[N].  Returns bgr[image_h, image_w, 3] uint8."""
        N = self.N
        h, Si, z = _c(h).reshape(2 * N), _c(Si).reshape(4 * N), _c(z).reshape(2 * N)
        m = np.ascontiguousarray(matched, dtype=np.int32).reshape(N)
        out = np.zeros((int(self.params.image_h), int(self.params.image_w), 3), dtype=np.uint8)
        self._chk(self._lib.srukf_render_overlay(self._h, _d(h), _d(Si), _d(z), _i(m), out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out

    def get_match_patch(self, k):
        out = np.zeros((17, 17), dtype=np.uint8)
        self._chk(self._lib.srukf_get_match_patch(self._h, int(k), out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out

    def detect_features(self, gray=None, max_corners=8, quality=0.1, min_dist=15.0, block_size=3, border=20, unfiltered=False,
                        map_px=None, map_gate=False, archived=None, project_archived=False):
        """detectAndfilteringFeatures on the device (srukf_detect_features): Shi-Tomasi corners of `gray` (image_h x image_w uint8; None: the
        frame the filter holds) and the reference's filter pass.  map_px[M,4] = (matchLocation, predictLocation) per map entry, archived[A,6] =
        FeatureInfo::state rows.  Returns (uv[K,2] accepted key points, loops[L,2] (key point index, archived index))."""
        dp = DetectParams(int(max_corners), float(quality), float(min_dist), int(block_size), float(border), int(bool(unfiltered)),
                          int(bool(map_gate)), int(bool(project_archived)))
        w, h = int(self.params.image_w), int(self.params.image_h)
        g = None
        if gray is not None:
            gray = np.ascontiguousarray(gray, dtype=np.uint8)
            assert gray.shape == (h, w)
            g = gray.ctypes.data_as(C.POINTER(C.c_ubyte))
        mp = _c(map_px).reshape(-1, 4) if map_px is not None else np.zeros((0, 4))
        ar = _c(archived).reshape(-1, 6) if archived is not None else np.zeros((0, 6))
        cap = int(max_corners) if max_corners > 0 else w * h
        loop_cap = min(cap * ar.shape[0], 1 << 20)
        uv = np.zeros((cap, 2))
        loops = np.zeros((max(loop_cap, 1), 2), dtype=np.int32)
        n_uv, n_loop = C.c_int(), C.c_int()
        self._chk(self._lib.srukf_detect_features(self._h, g, C.byref(dp), mp.shape[0], _d(mp) if mp.size else None, ar.shape[0],
                                                  _d(ar) if ar.size else None, _d(uv), cap, C.byref(n_uv), _i(loops), loop_cap,
                                                  C.byref(n_loop)))
        return uv[:min(n_uv.value, cap)].copy(), loops[:min(n_loop.value, loop_cap)].copy()

    def capture_appearance(self, first, uv, gray=None):
        """integrateFeaturesInformation's appearance fields (SLAM.cpp:918-926) of landmarks first .. first + K - 1 cut on the device:
        the 21x21 init patch at cvRound(uv) of `gray` (None: the held frame), Rwc of the current heading, the robot position."""
        uv = _c(uv).reshape(-1, 2)
        g = None
        if gray is not None:
            gray = np.ascontiguousarray(gray, dtype=np.uint8)
            assert gray.shape == (int(self.params.image_h), int(self.params.image_w))
            g = gray.ctypes.data_as(C.POINTER(C.c_ubyte))
        self._chk(self._lib.srukf_capture_appearance(self._h, int(first), uv.shape[0], _d(uv), g))

    def get_landmark_record(self, k):
        """What an archived landmark takes along (srukf_get_landmark_record): dict with X6[6], S66[6,6] (upper Cholesky factor of the marginal block
        P66), patch[21,21] uint8, R[3,3], t[3], px[2] and has_app (False: no appearance record, the other appearance fields are zero)."""
        x6, S, patch, R, t, px, has = np.zeros(6), np.zeros((6, 6)), np.zeros((21, 21), dtype=np.uint8), np.zeros((3, 3)), np.zeros(3), np.zeros(2), C.c_int()
        self._chk(self._lib.srukf_get_landmark_record(self._h, int(k), _d(x6), _d(S), patch.ctypes.data_as(C.POINTER(C.c_ubyte)), _d(R), _d(t), _d(px),
                                                      C.byref(has)))
        return {"X6": x6, "S66": S, "patch": patch, "R": R, "t": t, "px": px, "has_app": bool(has.value)}

    def insert_landmarks(self, X6, S66, patches=None, R=None, t=None, px=None):
        """Loop points back into the filter (srukf_insert_landmarks): L landmarks with means X6[L,6] and upper-triangular square-root blocks S66[L,6,6],
        no cross-covariance, at positions [N - K_new, N - K_new + L).  patches[L,21,21] uint8 with R[L,3,3], t[L,3], px[L,2]: their appearance records
        (None: no record).  The filter grows to N + L."""
        X6 = _c(X6).reshape(-1, 6)
        L = X6.shape[0]
        S66 = _c(S66).reshape(L, 6, 6)
        pb = None
        if patches is not None:
            patches = np.ascontiguousarray(patches, dtype=np.uint8).reshape(L, 21, 21)
            pb = patches.ctypes.data_as(C.POINTER(C.c_ubyte))
        R = _c(R).reshape(L, 9) if R is not None else None
        t = _c(t).reshape(L, 3) if t is not None else None
        px = _c(px).reshape(L, 2) if px is not None else None
        self._chk(self._lib.srukf_insert_landmarks(self._h, L, _d(X6), _d(S66), pb, _d(R), _d(t), _d(px)))
        self._refresh_dims()

    def archive_set(self, X6, S66, patches, R, t, px):
        """The archive archive_search covers (srukf_archive_set): L records with means X6[L,6], upper-triangular square-root blocks S66[L,6,6] and appearance
        records patches[L,21,21] uint8, R[L,3,3], t[L,3], px[L,2].  Replaces the whole archive; L = 0 (empty arrays) clears it."""
        X6 = _c(X6).reshape(-1, 6)
        L = X6.shape[0]
        S66, R, t, px = _c(S66).reshape(L, 36), _c(R).reshape(L, 9), _c(t).reshape(L, 3), _c(px).reshape(L, 2)
        patches = np.ascontiguousarray(patches, dtype=np.uint8).reshape(L, 441)
        self._chk(self._lib.srukf_archive_set(self._h, L, _d(X6), _d(S66), patches.ctypes.data_as(C.POINTER(C.c_ubyte)), _d(R), _d(t), _d(px)))

    def archive_count(self):
        return int(self._lib.srukf_archive_count(self._h))

    def archive_search(self, gray=None, half_cap=40, corr_threshold=0.8, chi2=5.99146454710798):
        """Every archived record searched for in `gray` (None: the held frame) by appearance (srukf_archive_search).  Returns (h[2L], Si[L,2,2], visible[L],
        z[2L], matched[L], corr[L]).  The filter is not changed."""
        L = self.archive_count()
        g = None
        if gray is not None:
            gray = np.ascontiguousarray(gray, dtype=np.uint8)
            assert gray.shape == (int(self.params.image_h), int(self.params.image_w))
            g = gray.ctypes.data_as(C.POINTER(C.c_ubyte))
        ap = ArchiveParams(int(half_cap), float(corr_threshold), float(chi2))
        h, Si, vis = np.zeros(2 * L), np.zeros((L, 2, 2)), np.zeros(L, dtype=np.int32)
        z, m, cr = np.zeros(2 * L), np.zeros(L, dtype=np.int32), np.zeros(L)
        self._chk(self._lib.srukf_archive_search(self._h, g, C.byref(ap), _d(h), _d(Si), _i(vis), _d(z), _i(m), _d(cr)))
        return h, Si, vis, z, m, cr

    def archive_template(self, j):
        """The 17 x 17 template the last archive_search warped for record j (zeros before any search)."""
        out = np.zeros((17, 17), dtype=np.uint8)
        self._chk(self._lib.srukf_archive_get_template(self._h, int(j), out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out

    def set_exclusive(self, exclusive):
        """True / GPU_EXCLUSIVE (default): the filter has the GPU to itself (one persistent refactorisation launch per frame that may
        use every CU); False / GPU_SHARED: several filters replay concurrently on this GPU (persistent launches of half the CUs,
        at most two admitted at a time); GPU_SHARED_PER_PANEL: one launch per 64-row panel."""
        self._chk(self._lib.srukf_set_exclusive(self._h, int(exclusive)))

    def debug_poke_S(self, row, col, value):
        """Test hook: one entry of S on the device, untracked."""
        self._chk(self._lib.srukf_debug_poke_state(self._h, int(row), int(col), float(value)))

    def set_rank_aware(self, on):
        """Rank-aware refactorisation (default on): structurally null pivots are not factored."""
        self._chk(self._lib.srukf_set_rank_aware(self._h, 1 if on else 0))

    def null_directions(self):
        return self._lib.srukf_null_directions(self._h)

    def set_storage(self, storage):
        """STORAGE_F64 (default) or STORAGE_F32: precision of the state kept between frames."""
        self._chk(self._lib.srukf_set_storage(self._h, int(storage)))

    def get_state_f32(self):
        X, S = np.zeros(self.n, dtype=np.float32), np.zeros((self.n, self.n), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        self._chk(self._lib.srukf_get_state_f32(self._h, X.ctypes.data_as(fp), S.ctypes.data_as(fp)))
        return X, S

    def delete_landmark(self, idx):
        """deleteOneFeature: landmark idx (0-based state order) leaves the map; the filter shrinks to N - 1."""
        self._chk(self._lib.srukf_delete_landmark(self._h, int(idx)))
        self._refresh_dims()

    def delete_landmarks(self, ids, records=False):
        """Several landmarks leave the map in one device call (srukf_delete_landmarks): ids are distinct 0-based positions, in any order; the filter shrinks
        to N - len(ids).  records=True: returns what get_landmark_record(id) gives for each id on the state before the call, as a dict of arrays X6[K,6],
        S66[K,6,6], patch[K,21,21] uint8, R[K,3,3], t[K,3], px[K,2], has_app[K] bool, in the order of ids."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32).ravel()
        K = int(ids.shape[0])
        if not records:
            self._chk(self._lib.srukf_delete_landmarks(self._h, K, _i(ids) if K else None, None, None, None, None, None, None, None))
            self._refresh_dims()
            return None
        M = max(K, 1)
        x6, S, patch = np.zeros((M, 6)), np.zeros((M, 6, 6)), np.zeros((M, 21, 21), dtype=np.uint8)
        R, t, px, has = np.zeros((M, 3, 3)), np.zeros((M, 3)), np.zeros((M, 2)), np.zeros(M, dtype=np.int32)
        self._chk(self._lib.srukf_delete_landmarks(self._h, K, _i(ids) if K else None, _d(x6), _d(S), patch.ctypes.data_as(C.POINTER(C.c_ubyte)), _d(R), _d(t), _d(px),
                                                   _i(has)))
        self._refresh_dims()
        return {"X6": x6[:K], "S66": S[:K], "patch": patch[:K], "R": R[:K], "t": t[:K], "px": px[:K], "has_app": has[:K] != 0}

    def stage_sequence(self, odo, z, matched):
        odo, z, m = _c(odo), _c(z), _c(matched, np.int32)
        F = z.shape[0]
        assert odo.shape == (F + 1, 3) and z.shape == (F, 2 * self.N) and m.shape == (F, self.N)
        self._chk(self._lib.srukf_stage_sequence(self._h, F, _d(odo), _d(z), _i(m)))
        self.F = F

    def prepare_frames(self, count, mode=UPDATE_BATCHED):
        """Capture `count` staged frames of `mode` as one graph for the following run_frames_async(*, count, mode) calls (nothing runs)."""
        if mode == UPDATE_BATCHED: self._chk(self._lib.srukf_prepare_frames(self._h, int(count)))
        else: self._chk(self._lib.srukf_prepare_frames_mode(self._h, int(count), int(mode)))

    def run_frames_async(self, first, count, mode=UPDATE_BATCHED, d_traj_ptr=None):
        self._chk(self._lib.srukf_run_frames_async(self._h, first, count, mode,
                                                   C.c_void_p(d_traj_ptr) if d_traj_ptr else None))

    def run_frames(self, first, count, mode=UPDATE_BATCHED):
        traj = np.empty((count, 8))
        self._chk(self._lib.srukf_run_frames(self._h, first, count, mode, _d(traj)))
        return traj

    def stage_images(self, gray):
        """The gray frames gray[F, image_h, image_w] uint8 of the staged sequence (F = its frame count), copied to the device once (srukf_stage_images).
        Image runs overwrite the z / matched rows of that sequence with what the association finds."""
        if not isinstance(gray, np.ndarray) or gray.dtype != np.uint8:
            raise TypeError("stage_images: gray must be a uint8 array")
        if gray.ndim != 3 or gray.shape[1:] != (int(self.params.image_h), int(self.params.image_w)):
            raise ValueError(f"stage_images: gray must be [F, {int(self.params.image_h)}, {int(self.params.image_w)}], got {gray.shape}")
        if gray.shape[0] < 1:
            raise ValueError("stage_images: no frames")
        gray = np.ascontiguousarray(gray)
        self._chk(self._lib.srukf_stage_images(self._h, gray.shape[0], gray.ctypes.data_as(C.POINTER(C.c_ubyte))))

    @staticmethod
    def _image_run_args(first, count, mode):
        for name, v in (("first", first), ("count", count), ("mode", mode)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"run_images: {name} must be an integer")
        if first < 0 or count < 1:
            raise ValueError("run_images: first >= 0 and count >= 1")

    def run_images_async(self, first, count, mode=UPDATE_BATCHED, d_traj_ptr=None):
        """Staged frames [first, first + count) with the association on the device (srukf_run_images_async); a flagged block is restored by synchronize()."""
        self._image_run_args(first, count, mode)
        self._chk(self._lib.srukf_run_images_async(self._h, int(first), int(count), int(mode), C.c_void_p(d_traj_ptr) if d_traj_ptr else None))

    def run_images(self, first, count, mode=UPDATE_BATCHED):
        """run_images_async + synchronize -> traj[count, 8].  SrukfError(SRUKF_ERR_CLAMP_PENDING) for a flagged block: X, S and every matchPatch are as before the call."""
        self._image_run_args(first, count, mode)
        traj = np.empty((count, 8))
        self._chk(self._lib.srukf_run_images(self._h, int(first), int(count), int(mode), _d(traj)))
        return traj

    def get_image_matches(self, first, count):
        """What the association wrote for staged frames [first, first + count) (srukf_get_image_matches): dict of z[count, 2N], matched[count, N], corr[count, N],
        visible[count, N], h[count, 2N]."""
        self._image_run_args(first, count, UPDATE_BATCHED)
        N = self.N
        out = dict(z=np.zeros((count, 2 * N)), matched=np.zeros((count, N), dtype=np.int32), corr=np.zeros((count, N)),
                   visible=np.zeros((count, N), dtype=np.int32), h=np.zeros((count, 2 * N)))
        self._chk(self._lib.srukf_get_image_matches(self._h, int(first), int(count), _d(out["z"]), _i(out["matched"]), _d(out["corr"]), _i(out["visible"]),
                                                    _d(out["h"])))
        return out

    @staticmethod
    def _match_params(corr_threshold, ratio, exclusion, subpixel):
        """the parameters of a checked image run as the library's struct; types are checked here, values (ratio > 0, exclusion in [1, 20], finite) by the library"""
        for name, v in (("corr_threshold", corr_threshold), ("ratio", ratio)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise TypeError(f"run_images_checked: {name} must be a real number")
        if isinstance(exclusion, bool) or not isinstance(exclusion, (int, np.integer)):
            raise TypeError("run_images_checked: exclusion must be an integer")
        if not isinstance(subpixel, (bool, np.bool_)) and subpixel not in (0, 1):
            raise TypeError("run_images_checked: subpixel must be a bool")
        if not -2 ** 31 <= int(exclusion) < 2 ** 31:
            raise ValueError("run_images_checked: exclusion does not fit an int")
        return MatchParams(float(corr_threshold), float(ratio), int(exclusion), int(bool(subpixel)))

    def run_images_checked_async(self, first, count, mode=UPDATE_BATCHED, corr_threshold=0.8, ratio=0.9, exclusion=4, subpixel=False, d_traj_ptr=None):
        """run_images_async with associate_checked's association in every frame (srukf_run_images_checked_async): a match whose second peak reaches ratio * the best
        is vetoed, subpixel=True refines the best peak.  The parameters may differ from run to run inside a block."""
        self._image_run_args(first, count, mode)
        mp = self._match_params(corr_threshold, ratio, exclusion, subpixel)
        self._chk(self._lib.srukf_run_images_checked_async(self._h, int(first), int(count), int(mode), C.byref(mp), C.c_void_p(d_traj_ptr) if d_traj_ptr else None))

    def run_images_checked(self, first, count, mode=UPDATE_BATCHED, corr_threshold=0.8, ratio=0.9, exclusion=4, subpixel=False):
        """run_images_checked_async + synchronize -> traj[count, 8]; as run_images for a flagged block.  get_image_matches has z / matched / corr / visible / h,
        get_image_checks the rest; match_scores(k) then answers for the run's last frame."""
        self._image_run_args(first, count, mode)
        mp = self._match_params(corr_threshold, ratio, exclusion, subpixel)
        traj = np.empty((count, 8))
        self._chk(self._lib.srukf_run_images_checked(self._h, int(first), int(count), int(mode), C.byref(mp), _d(traj)))
        return traj

    def get_image_checks(self, first, count):
        """What checked image runs wrote beside get_image_matches' record for staged frames [first, first + count) (srukf_get_image_checks): dict of corr2[count, N],
        z2[count, 2N], flags[count, N].  Rows no checked run has written are zero; a row a plain run_images wrote later keeps the checked run's values."""
        self._image_run_args(first, count, UPDATE_BATCHED)
        N = self.N
        out = dict(corr2=np.zeros((count, N)), z2=np.zeros((count, 2 * N)), flags=np.zeros((count, N), dtype=np.int32))
        self._chk(self._lib.srukf_get_image_checks(self._h, int(first), int(count), _d(out["corr2"]), _d(out["z2"]), _i(out["flags"])))
        return out

    @staticmethod
    def _archive_params(half_cap, corr_threshold, chi2):
        """archive_search's parameters as the library's struct; types are checked here, values (half_cap in [10, 40], chi2 > 0, finite) by the library"""
        if isinstance(half_cap, bool) or not isinstance(half_cap, (int, np.integer)):
            raise TypeError("images_search_archive: half_cap must be an integer")
        for name, v in (("corr_threshold", corr_threshold), ("chi2", chi2)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise TypeError(f"images_search_archive: {name} must be a real number")
        if not -2 ** 31 <= int(half_cap) < 2 ** 31:
            raise ValueError("images_search_archive: half_cap does not fit an int")
        return ArchiveParams(int(half_cap), float(corr_threshold), float(chi2))

    def images_search_archive(self, on, half_cap=40, corr_threshold=0.8, chi2=5.99146454710798):
        """The switch of the searching image runs (srukf_images_search_archive): while on, every frame of every later run_images* / run_images_checked* is followed
        by one archive_search of the whole archive on that frame's staged image, on the posterior; get_image_archive has the per-frame record.  Not while an image
        run is in flight (SRUKF_ERR_SEQUENCE)."""
        if not isinstance(on, (bool, np.bool_)) and not (isinstance(on, (int, np.integer)) and on in (0, 1)):
            raise TypeError("images_search_archive: on must be a bool")
        ap = self._archive_params(half_cap, corr_threshold, chi2)
        self._chk(self._lib.srukf_images_search_archive(self._h, int(bool(on)), C.byref(ap)))

    def get_image_archive(self, first, count):
        """What the searching image runs wrote for staged frames [first, first + count) (srukf_get_image_archive): dict of L (the archive size of the rows),
        h[count, 2L], Si[count, L, 2, 2], visible[count, L], z[count, 2L], matched[count, L], corr[count, L], hits[count].  Rows no searching run wrote are zero."""
        self._image_run_args(first, count, UPDATE_BATCHED)
        L, hits = C.c_int(0), np.zeros(count, dtype=np.int32)
        self._chk(self._lib.srukf_get_image_archive(self._h, int(first), int(count), C.byref(L), None, None, None, None, None, None, _i(hits)))
        L = int(L.value)
        out = dict(L=L, h=np.zeros((count, 2 * L)), Si=np.zeros((count, L, 2, 2)), visible=np.zeros((count, L), dtype=np.int32), z=np.zeros((count, 2 * L)),
                   matched=np.zeros((count, L), dtype=np.int32), corr=np.zeros((count, L)), hits=hits)
        if L > 0:
            L2 = C.c_int(0)
            self._chk(self._lib.srukf_get_image_archive(self._h, int(first), int(count), C.byref(L2), _d(out["h"]), _d(out["Si"]), _i(out["visible"]), _d(out["z"]),
                                                        _i(out["matched"]), _d(out["corr"]), _i(out["hits"])))
            assert L2.value == L
        return out

    # ---- the map policy's verdict (srukf_map_policy, srukf_images_policy) ----
    @staticmethod
    def _policy_params(border, rho_min, min_predictions, min_matches):
        """the policy's parameters as the library's struct; types are checked here, values (border finite and >= 0, rho_min finite, counts >= 0) by the library"""
        for name, v in (("border", border), ("rho_min", rho_min)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise TypeError(f"map policy: {name} must be a real number")
        for name, v in (("min_predictions", min_predictions), ("min_matches", min_matches)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"map policy: {name} must be an integer")
            if not -2 ** 31 <= int(v) < 2 ** 31:
                raise ValueError(f"map policy: {name} does not fit an int")
        return PolicyParams(float(border), float(rho_min), int(min_predictions), int(min_matches))

    def _policy_state(self, state, who):
        st = np.ascontiguousarray(state, dtype=POLICY_STATE_DTYPE)
        if st.shape != (self.N,):
            raise ValueError(f"{who}: state must have one POLICY_STATE_DTYPE entry per landmark")
        return st.copy()

    def map_policy(self, state, h, visible, z, matched, border=20.0, rho_min=0.01, min_predictions=10, min_matches=5):
        """The map policy's verdict for one frame on the filter's current X (srukf_map_policy): state[N] (POLICY_STATE_DTYPE) is advanced with the frame's
        association -> (verdict[N] of POLICY_* bits, summary dict, new state)."""
        pp = self._policy_params(border, rho_min, min_predictions, min_matches)
        N = self.N
        st = self._policy_state(state, "map_policy")
        h, z = _c(h).reshape(-1), _c(z).reshape(-1)
        vis, m = _c(visible, np.int32).reshape(-1), _c(matched, np.int32).reshape(-1)
        if h.size != 2 * N or z.size != 2 * N or vis.size != N or m.size != N:
            raise ValueError("map_policy: h / z need 2N entries, visible / matched N")
        verdict, sm = np.zeros(N, dtype=np.int32), PolicySummary()
        self._chk(self._lib.srukf_map_policy(self._h, C.byref(pp), st.ctypes.data_as(C.c_void_p), _d(h), _i(vis), _d(z), _i(m), _i(verdict), C.byref(sm)))
        return verdict, {k: int(getattr(sm, k)) for k in POLICY_SUMMARY_FIELDS}, st

    def images_policy(self, on, border=20.0, rho_min=0.01, min_predictions=10, min_matches=5):
        """The switch of the map policy behind image frames (srukf_images_policy): while on, every frame of every later run_images* / run_images_checked* is
        followed by the verdict on that frame's posterior; get_image_policy has the per-frame record.  Not while an image run is in flight (SRUKF_ERR_SEQUENCE)."""
        if not isinstance(on, (bool, np.bool_)) and not (isinstance(on, (int, np.integer)) and on in (0, 1)):
            raise TypeError("images_policy: on must be a bool")
        pp = self._policy_params(border, rho_min, min_predictions, min_matches)
        self._chk(self._lib.srukf_images_policy(self._h, int(bool(on)), C.byref(pp)))

    def set_policy_state(self, state):
        """Seeds the policy state the staged images own (srukf_images_set_policy_state): state[N] of POLICY_STATE_DTYPE.  Images staged, no run pending."""
        st = self._policy_state(state, "set_policy_state")
        self._chk(self._lib.srukf_images_set_policy_state(self._h, st.ctypes.data_as(C.c_void_p)))

    def get_image_policy(self, first, count):
        """What the policy wrote behind staged frames [first, first + count) (srukf_get_image_policy): dict of verdict[count, N], summary (structured array
        [count] of POLICY_SUMMARY_FIELDS), state[N] (the device state now) and first_change (the lowest frame whose summary has `change`, or -1)."""
        self._image_run_args(first, count, UPDATE_BATCHED)
        N = self.N
        out = dict(verdict=np.zeros((count, N), dtype=np.int32), summary=np.zeros(count, dtype=POLICY_SUMMARY_DTYPE), state=np.zeros(N, dtype=POLICY_STATE_DTYPE))
        fc = C.c_int(-1)
        self._chk(self._lib.srukf_get_image_policy(self._h, int(first), int(count), _i(out["verdict"]), out["summary"].ctypes.data_as(C.c_void_p),
                                                   out["state"].ctypes.data_as(C.c_void_p), C.byref(fc)))
        out["first_change"] = int(fc.value)
        return out

    def images_rewind(self):
        """Puts back the checkpoint of the image block the last synchronize ended clean: X, S, every matchPatch and the policy state (srukf_images_rewind).
        SrukfError(SRUKF_ERR_SEQUENCE) when a run is pending, no image block has been synchronised, or the state has been written since."""
        self._chk(self._lib.srukf_images_rewind(self._h))

    # ---- the 1-point RANSAC consensus inside image frames (srukf_images_ransac) ----
    def images_ransac(self, on, threshold=8.0):
        """The switch of the consensus inside image frames (srukf_images_ransac): while on, every frame of every later run_images* / run_images_checked* runs
        ransac_consensus' kernels between its association and its update, and the update uses the consensus set only (the frame's `matched` row is rewritten to it);
        get_image_ransac has the per-frame record.  threshold: pixels, finite and positive.  Not while a run is in flight (SRUKF_ERR_SEQUENCE)."""
        if not isinstance(on, (bool, np.bool_)) and not (isinstance(on, (int, np.integer)) and on in (0, 1)):
            raise TypeError("images_ransac: on must be a bool")
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
            raise TypeError("images_ransac: threshold must be a real number")
        self._chk(self._lib.srukf_images_ransac(self._h, int(bool(on)), float(threshold)))

    def get_image_ransac(self, first, count):
        """What the consensus wrote for staged frames [first, first + count) (srukf_get_image_ransac): dict of flags[count, N] (bit 0: matched and visible, bit 1:
        low-innovation inlier), votes[count, N], dist[count, N], best[count], n_active[count], n_low[count] and first_outlier (the lowest frame whose consensus
        dropped a match, or -1).  Rows no such frame wrote are zero."""
        self._image_run_args(first, count, UPDATE_BATCHED)
        N = self.N
        out = dict(flags=np.zeros((count, N), dtype=np.int32), votes=np.zeros((count, N), dtype=np.int32), dist=np.zeros((count, N)),
                   best=np.zeros(count, dtype=np.int32), n_active=np.zeros(count, dtype=np.int32), n_low=np.zeros(count, dtype=np.int32))
        fo = C.c_int(-1)
        self._chk(self._lib.srukf_get_image_ransac(self._h, int(first), int(count), _i(out["flags"]), _i(out["votes"]), _d(out["dist"]), _i(out["best"]),
                                                   _i(out["n_active"]), _i(out["n_low"]), C.byref(fo)))
        out["first_outlier"] = int(fo.value)
        return out

    # ---- the rescue gate behind the frames that hold the consensus (srukf_images_rescue_gate) ----
    def images_rescue_gate(self, on, chi2=5.99146454710798):
        """The switch of the rescue gate (srukf_images_rescue_gate): while on together with images_ransac, every frame of every later run_images* /
        run_images_checked* is followed by the test whether a match its consensus dropped would be rescued (get_image_rescue has the record), and the snapshot
        guard stops on a rescue instead of a dropped match.  chi2: finite and positive.  Not while a run is in flight (SRUKF_ERR_SEQUENCE)."""
        if not isinstance(on, (bool, np.bool_)) and not (isinstance(on, (int, np.integer)) and on in (0, 1)):
            raise TypeError("images_rescue_gate: on must be a bool")
        if isinstance(chi2, bool) or not isinstance(chi2, (int, float, np.integer, np.floating)):
            raise TypeError("images_rescue_gate: chi2 must be a real number")
        self._chk(self._lib.srukf_images_rescue_gate(self._h, int(bool(on)), float(chi2)))

    def get_image_rescue(self, first, count):
        """What the rescue gate wrote for staged frames [first, first + count) (srukf_get_image_rescue): dict of flags[count, N] (bit 0: candidate, bit 1: rescued),
        h2[count, 2N], Si2[count, N, 2, 2], chi2[count, N], n_cand[count], n_high[count] and first_rescue (the lowest frame that would rescue a match, or -1).
        Rows of non-candidates and rows no such frame wrote are zero."""
        self._image_run_args(first, count, UPDATE_BATCHED)
        N = self.N
        out = dict(flags=np.zeros((count, N), dtype=np.int32), h2=np.zeros((count, 2 * N)), Si2=np.zeros((count, N, 2, 2)), chi2=np.zeros((count, N)),
                   n_cand=np.zeros(count, dtype=np.int32), n_high=np.zeros(count, dtype=np.int32))
        fr = C.c_int(-1)
        self._chk(self._lib.srukf_get_image_rescue(self._h, int(first), int(count), _i(out["flags"]), _d(out["h2"]), _d(out["Si2"]), _d(out["chi2"]),
                                                   _i(out["n_cand"]), _i(out["n_high"]), C.byref(fr)))
        out["first_rescue"] = int(fr.value)
        return out

    # ---- the state at a block's stop (srukf_images_snapshots / srukf_images_resume) ----
    def images_snapshots(self, on):
        """The switch of the snapshot launch in front of image frames (srukf_images_snapshots): while on, every frame of every later run_images* /
        run_images_checked* first keeps the state it starts from (X, S, matchPatches, policy state) in slot frame & 1, as long as no frame of the block in front of
        it has stopped the block; images_resume then cuts the block without running frames again.  Not while a run is in flight or a block is pending."""
        if not isinstance(on, (bool, np.bool_)) and not (isinstance(on, (int, np.integer)) and on in (0, 1)):
            raise TypeError("images_snapshots: on must be a bool")
        self._chk(self._lib.srukf_images_snapshots(self._h, int(bool(on))))

    def get_image_snapshots(self):
        """The staged frames whose start the two slots hold, (slot 0, slot 1); -1: none (srukf_get_image_snapshots).  Waits for the stream."""
        tags = np.full(2, -1, dtype=np.int32)
        self._chk(self._lib.srukf_get_image_snapshots(self._h, _i(tags)))
        return int(tags[0]), int(tags[1])

    def images_resume(self, keep):
        """Cuts the image block the last synchronize ended clean to its first `keep` frames without running them again (srukf_images_resume): X, S, every
        matchPatch and the policy state become what the block's frame `keep` started from, rows >= keep of the policy and consensus records are zeroed.  keep 0 is
        images_rewind, keep == the frames run changes nothing.  SrukfError(SRUKF_ERR_SEQUENCE) where images_rewind is refused, when a run of the block had the
        switch off, or when no slot holds that frame (the block can then still be rewound)."""
        if isinstance(keep, (bool, np.bool_)) or not isinstance(keep, (int, np.integer)):
            raise TypeError("images_resume: keep must be an int")
        if keep < 0:
            raise ValueError("images_resume: keep must be >= 0")
        self._chk(self._lib.srukf_images_resume(self._h, int(keep)))

    # ---- the display view behind image frames, the overlay of a staged frame (srukf_images_display) ----
    def images_display(self, on):
        """The switch of the display view behind image frames (srukf_images_display): while on, every frame of every later run_images* / run_images_checked* is
        followed by get_frame_view_display's launches into that frame's row of a record (get_image_display), and render_image_overlay can draw the frame.  The
        run is issued frame by frame, as with images_policy.  Not while a run is in flight or a block is pending."""
        if not isinstance(on, (bool, np.bool_)) and not (isinstance(on, (int, np.integer)) and on in (0, 1)):
            raise TypeError("images_display: on must be a bool")
        self._chk(self._lib.srukf_images_display(self._h, int(bool(on))))

    def get_image_display(self, first, count):
        """The display view behind staged frames [first, first + count) (srukf_get_image_display): dict of xyz[count, N, 3], cov[count, N, 3, 3],
        axis[count, N, 4], sigma[count, N, 3], rot[count, N], pose[count, 4], P4[count, 4, 4] and Si[count, N, 2, 2] (what the frame's association read).
        Rows no run with images_display on has written are zero."""
        self._image_run_args(first, count, UPDATE_BATCHED)
        N = self.N
        out = dict(xyz=np.zeros((count, N, 3)), cov=np.zeros((count, N, 3, 3)), axis=np.zeros((count, N, 4)), sigma=np.zeros((count, N, 3)),
                   rot=np.zeros((count, N), dtype=np.int32), pose=np.zeros((count, 4)), P4=np.zeros((count, 4, 4)), Si=np.zeros((count, N, 2, 2)))
        self._chk(self._lib.srukf_get_image_display(self._h, int(first), int(count), _d(out["xyz"]), _d(out["cov"]), _d(out["axis"]), _d(out["sigma"]),
                                                    _i(out["rot"]), _d(out["pose"]), _d(out["P4"]), _d(out["Si"])))
        return out

    def render_image_overlay(self, frame):
        """render_overlay for staged frame `frame` from what the device holds (srukf_render_image_overlay): the frame's gray image with the predicted cross, the
        matched cross and the chi-square ellipse of every landmark the filter used.  Returns bgr[image_h, image_w, 3] uint8.  SrukfError(SRUKF_ERR_SEQUENCE)
        when no run with images_display on has written that frame's row."""
        if isinstance(frame, (bool, np.bool_)) or not isinstance(frame, (int, np.integer)):
            raise TypeError("render_image_overlay: frame must be an int")
        if frame < 0:
            raise ValueError("render_image_overlay: frame must be >= 0")
        out = np.zeros((int(self.params.image_h), int(self.params.image_w), 3), dtype=np.uint8)
        self._chk(self._lib.srukf_render_image_overlay(self._h, int(frame), out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out

    # ---- colour frames in the staged stack, the overlays of a run of frames ----
    def stage_images_bgr(self, bgr, keep_colour=True):
        """stage_images for colour frames bgr[F, image_h, image_w, 3] uint8 (B, G, R), converted on the device by set_frame_bgr's rule (srukf_stage_images_bgr).
        Behind it the filter is what stage_images with the converted frames leaves.  keep_colour: the colour stack stays on the device and
        render_image_overlay(s) draw on it."""
        if not isinstance(bgr, np.ndarray) or bgr.dtype != np.uint8:
            raise TypeError("stage_images_bgr: bgr must be a uint8 array")
        if not isinstance(keep_colour, (bool, np.bool_)):
            raise TypeError("stage_images_bgr: keep_colour must be a bool")
        if bgr.ndim != 4 or bgr.shape[1:] != (int(self.params.image_h), int(self.params.image_w), 3):
            raise ValueError(f"stage_images_bgr: bgr must be [F, {int(self.params.image_h)}, {int(self.params.image_w)}, 3], got {bgr.shape}")
        if bgr.shape[0] < 1:
            raise ValueError("stage_images_bgr: no frames")
        bgr = np.ascontiguousarray(bgr)
        self._chk(self._lib.srukf_stage_images_bgr(self._h, bgr.shape[0], bgr.ctypes.data_as(C.POINTER(C.c_ubyte)), int(bool(keep_colour))))

    def get_staged_image(self, frame, want_bgr=False):
        """Frame `frame` of the staged stack (srukf_get_staged_image): gray[image_h, image_w] uint8, or with want_bgr (gray, bgr[image_h, image_w, 3]).
        SrukfError(SRUKF_ERR_SEQUENCE) for want_bgr when no colour stack is kept."""
        if isinstance(frame, (bool, np.bool_)) or not isinstance(frame, (int, np.integer)):
            raise TypeError("get_staged_image: frame must be an int")
        if not isinstance(want_bgr, (bool, np.bool_)):
            raise TypeError("get_staged_image: want_bgr must be a bool")
        if frame < 0:
            raise ValueError("get_staged_image: frame must be >= 0")
        H, W = int(self.params.image_h), int(self.params.image_w)
        gray = np.zeros((H, W), dtype=np.uint8)
        bgr = np.zeros((H, W, 3), dtype=np.uint8) if want_bgr else None
        self._chk(self._lib.srukf_get_staged_image(self._h, int(frame), gray.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                   bgr.ctypes.data_as(C.POINTER(C.c_ubyte)) if want_bgr else None))
        return (gray, bgr) if want_bgr else gray

    def render_image_overlays(self, first, count):
        """render_image_overlay for staged frames [first, first + count) in one device call (srukf_render_image_overlays): bgr[count, image_h, image_w, 3]
        uint8, frame q of it what render_image_overlay(first + q) returns.  SrukfError(SRUKF_ERR_SEQUENCE) when a frame of the range is not drawable."""
        for name, v in (("first", first), ("count", count)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"render_image_overlays: {name} must be an int")
        if first < 0 or count < 1:
            raise ValueError("render_image_overlays: first must be >= 0 and count >= 1")
        out = np.zeros((int(count), int(self.params.image_h), int(self.params.image_w), 3), dtype=np.uint8)
        self._chk(self._lib.srukf_render_image_overlays(self._h, int(first), int(count), out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out

    def synchronize(self):
        self._chk(self._lib.srukf_synchronize(self._h))

    def clamp_info(self):
        """(frame, row) of the last SRUKF_ERR_CLAMP_PENDING; (-1, -1) if none."""
        fr, row = C.c_int(), C.c_int()
        self._chk(self._lib.srukf_clamp_info(self._h, C.byref(fr), C.byref(row)))
        return fr.value, row.value

    def debug_allow_mixed(self, on):
        """Study hook: accept STORAGE_F32_MIXED below its epsilon floor."""
        self._chk(self._lib.srukf_debug_allow_mixed(self._h, int(on)))

    def debug_set(self, key, value):
        """Measurement / test switch of this filter (or a process-wide one): see srukf_debug_set in include/srukf.h."""
        self._chk(self._lib.srukf_debug_set(self._h, key.encode(), int(value)))

    def debug_get(self, key):
        v = C.c_longlong()
        self._chk(self._lib.srukf_debug_get(self._h, key.encode(), C.byref(v)))
        return v.value

    def debug_copy(self, key, count):
        """Diagnostic copy of the first `count` doubles of a device work buffer ("Z", "DZ", "sigR", "Cmat", "Xr1", "Utp", "P1", "h", "Si", "Ut", "PxyR", "joint_R")."""
        out = np.empty(int(count), dtype=np.float64)
        self._chk(self._lib.srukf_debug_copy(self._h, key.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), int(count)))
        return out

    def debug_upload(self, key, arr):
        """The other direction of debug_copy (measurement scripts)."""
        a = np.ascontiguousarray(arr, dtype=np.float64).ravel()
        self._chk(self._lib.srukf_debug_upload(self._h, key.encode(), a.ctypes.data_as(C.POINTER(C.c_double)), a.size))

    def debug_split_replay(self, which, reps=1):
        """One launch of the split form's pair alone against recorded buffers (scripts/split_replay.py)."""
        self._chk(self._lib.srukf_debug_split_replay(self._h, int(which), int(reps)))

    def debug_gmw_stamps(self):
        """Diagnostic builds only: the time stamps the persistent launch left since the last call (and arms the next launches)."""
        buf = (C.c_ulonglong * 4096)()
        self._chk(self._lib.srukf_debug_gmw_stamps(self._h, buf))
        return np.ctypeslib.as_array(buf).copy()

    def debug_starve_workers(self, on):
        """Test hook: persistent factorisation launches start without their workers."""
        self._chk(self._lib.srukf_debug_starve_workers(self._h, int(on)))

    def set_profiling(self, on):
        self._chk(self._lib.srukf_set_profiling(self._h, int(on)))

    def profile_reset(self):
        self._chk(self._lib.srukf_profile_reset(self._h))

    def profile(self):
        out = {}
        for i in range(self._lib.srukf_profile_count(self._h)):
            name, ms, cnt, fl, by = C.c_char_p(), C.c_double(), C.c_longlong(), C.c_double(), C.c_double()
            self._chk(self._lib.srukf_profile_get(self._h, i, C.byref(name), C.byref(ms), C.byref(cnt), C.byref(fl), C.byref(by)))
            out[name.value.decode()] = {"ms": ms.value, "launches": cnt.value, "alg_flops": fl.value, "alg_bytes": by.value}
        return out


def debug_set_global(key, value):
    """Process-wide measurement / test switch (srukf_debug_set with a NULL context)."""
    rc = load_library().srukf_debug_set(None, key.encode(), int(value))
    if rc != 0:
        raise SrukfError(rc, f"srukf_debug_set({key})")


def debug_switches(filter=None):
    """Every switch of srukf_debug_set -> {key: (per_filter, default, value)}; value: the current setting (per-filter keys: this filter's; without one, the default)."""
    lib, out, i = load_library(), {}, 0
    key, per, dflt, val = C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
    while lib.srukf_debug_switch_at(filter._h if filter is not None else None, i, C.byref(key), C.byref(per), C.byref(dflt), C.byref(val)) == 0:
        out[key.value.decode()] = (bool(per.value), dflt.value, val.value)
        i += 1
    return out


def run_frames_batch(filters, first, count, mode=UPDATE_BATCHED):
    """B filters through the same block of staged frames concurrently on one GPU (srukf_run_frames_batch) -> traj[B, count, 8]."""
    B = len(filters)
    hs = (C.c_void_p * B)(*[f._h.value for f in filters])
    traj = np.empty((B, count, 8))
    st = (C.c_int * B)()
    rc = load_library().srukf_run_frames_batch(hs, B, first, count, mode, _d(traj), st)
    if rc != 0:
        bad = [b for b in range(B) if st[b] != 0]
        filters[bad[0] if bad else 0]._chk(rc)
    return traj


def gmw(G, eps=1e-13, force_slow=False, device=0):
    """Device modified Cholesky of a symmetric matrix (SLAM.cpp:2197-2327) -> (S, D, clamp_hit)."""
    G = _c(G)
    n = G.shape[0]
    S, D, hit = np.zeros((n, n)), np.zeros(n), C.c_int(0)
    rc = load_library().srukf_gmw_host(device, n, _d(G), _d(S), _d(D), eps, int(force_slow), C.byref(hit))
    if rc != 0:
        raise SrukfError(rc, "srukf_gmw_host")
    return S, D, hit.value


def project(params, feat6, pos3, psi, err2, device=0):
    """Device camera projection of individual points (SLAM.cpp:1662-1670)."""
    p = Params.from_dict(params)
    feat6, pos3, psi, err2 = _c(feat6).reshape(-1, 6), _c(pos3).reshape(-1, 3), _c(psi).reshape(-1), _c(err2).reshape(-1, 2)
    out = np.zeros((feat6.shape[0], 2))
    rc = load_library().srukf_project_host(device, C.byref(p), feat6.shape[0], _d(feat6), _d(pos3), _d(psi), _d(err2), _d(out))
    if rc != 0:
        raise SrukfError(rc, "srukf_project_host")
    return out
