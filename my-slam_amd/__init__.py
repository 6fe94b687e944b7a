"""my-slam_amd: MI355X-native ORB front-end (extractor + Hamming matcher) behind a C ABI.

The product is `lib/liborbx.so` (hand-written HIP for gfx950, see csrc/).  This module is only the
ctypes plumbing the tests and bench.py use to reach that C ABI from Python; there is no CPU path:
if the library is missing or no HIP device is present every entry point raises.

The directory name carries a hyphen (the framework's name); load it with
    importlib.util.spec_from_file_location("my_slam_amd", "<repo>/my-slam_amd/__init__.py")
or via tests/conftest.py / the loader at the top of bench.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# ORBX_LIB: developer switch for A/B builds of the same library (tools/dbg/ab_variants.sh); never a different back end
LIB_PATH = os.environ.get("ORBX_LIB") or os.path.join(PKG_DIR, "lib", "liborbx.so")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28
# orbm_camera (include/orbm.h): what CreateNewMapPoints' per-match loop reads of a key frame
ORBX_MAX_LEVELS = 16
CAM_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                      ("cy", "<f4"), ("invfx", "<f4"), ("invfy", "<f4"), ("mb", "<f4"), ("mbf", "<f4"), ("scale_factor", "<f4"),
                      ("nlevels", "<i4"), ("scale_factors", "<f4", (ORBX_MAX_LEVELS,)), ("level_sigma2", "<f4", (ORBX_MAX_LEVELS,))])
assert CAM_DTYPE.itemsize == 228
# orbm_frame_view (include/orbm.h): what Frame::isInFrustum reads of the frame
VIEW_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                       ("cy", "<f4"), ("mbf", "<f4"), ("bounds", "<f4", (4,)), ("log_scale_factor", "<f4"), ("nlevels", "<i4"),
                       ("scale_factors", "<f4", (ORBX_MAX_LEVELS,))])
assert VIEW_DTYPE.itemsize == 168
# orbm_fuse_view (include/orbm.h): what ORBmatcher::Fuse reads of a target key frame beyond its features; grid = orbm_kf_grid
KF_GRID_DTYPE = np.dtype([("assign_min_x", "<f4"), ("assign_min_y", "<f4"), ("inv_w", "<f4"), ("inv_h", "<f4"), ("query_min_x", "<f4"),
                          ("query_min_y", "<f4")])
FUSE_VIEW_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                            ("cy", "<f4"), ("mbf", "<f4"), ("bounds", "<f4", (4,)), ("log_scale_factor", "<f4"), ("nlevels", "<i4"),
                            ("scale_factors", "<f4", (ORBX_MAX_LEVELS,)), ("inv_level_sigma2", "<f4", (ORBX_MAX_LEVELS,)),
                            ("grid", KF_GRID_DTYPE)])
assert FUSE_VIEW_DTYPE.itemsize == 256      # sizeof(orbm_fuse_view): tests/test_fuse_views_cxx.py compares it with the C struct
# orbm_fuse_status (include/orbm.h)
(ORBM_FUSE_MATCH, ORBM_FUSE_SKIPPED, ORBM_FUSE_BEHIND, ORBM_FUSE_OUT_IMAGE, ORBM_FUSE_DISTANCE, ORBM_FUSE_VIEW_ANGLE, ORBM_FUSE_UNDEFINED,
 ORBM_FUSE_NO_MATCH) = range(8)
# orbm_pose_camera (include/orbm.h): the calibration of one problem of pose_optimization_batch
POSE_CAM_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("bf", "<f4")])
assert POSE_CAM_DTYPE.itemsize == 20
# orbm_sim3_camera (include/orbm.h): the two calibrations {fx, fy, cx, cy} and mbFixScale of one problem of sim3_hypotheses
SIM3_CAM_DTYPE = np.dtype([("K1", "<f4", (4,)), ("K2", "<f4", (4,)), ("fix_scale", "<i4")])
assert SIM3_CAM_DTYPE.itemsize == 36
# orbm_pnp_camera (include/orbm.h): the calibration and mRansacMinSet of one problem of pnp_hypotheses
PNP_CAM_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("set_size", "<i4")])
assert PNP_CAM_DTYPE.itemsize == 20
ORBM_PNP_MAX_SET = 8
# orbm_init_params (include/orbm.h): Normalize's T1, T2 (row-major 3 x 3) and sigma of one problem of init_hypotheses
INIT_PARAMS_DTYPE = np.dtype([("T1", "<f4", (9,)), ("T2", "<f4", (9,)), ("sigma", "<f4")])
assert INIT_PARAMS_DTYPE.itemsize == 76
INIT_MODEL_H, INIT_MODEL_F = 0, 1
ORBM_INIT_MAX_MOTIONS = 8
# orbm_init_rt_status (include/orbm.h): the line of Initializer::CheckRT that decided a match
(ORBM_INIT_RT_GOOD, ORBM_INIT_RT_GOOD_LOW_PARALLAX, ORBM_INIT_RT_NOT_INLIER, ORBM_INIT_RT_NOT_FINITE, ORBM_INIT_RT_BEHIND1,
 ORBM_INIT_RT_BEHIND2, ORBM_INIT_RT_REPROJ1, ORBM_INIT_RT_REPROJ2) = range(8)

ORBX_OK = 0
ORBX_E_INVALID, ORBX_E_CAPACITY, ORBX_E_SHAPE, ORBX_E_HIP, ORBX_E_CAND_OVERFLOW, ORBX_E_TREE_OVERFLOW = -1, -2, -3, -4, -5, -6
ORBM_TRI_NO_MATCH = 255      # orbm_tri_status of a (view, feature) slot without a pair (ORBmatcher.create_new_map_points)
ORBX_OPT_BLUR_ROUNDING = 1
ORBX_OPT_SUBBATCHES = 2
ORBX_OPT_OVERLAP_PYRAMID = 3
ORBX_OPT_BATCH_CHUNK = 4
# orbx_format (include/orbx.h): what a handle's frames hold; colour frames are converted to grey on the GPU
ORBX_FMT_GRAY8, ORBX_FMT_BGR8, ORBX_FMT_RGB8, ORBX_FMT_BGRA8, ORBX_FMT_RGBA8 = 0, 1, 2, 3, 4
_FMT_CHANNELS = {ORBX_FMT_GRAY8: 1, ORBX_FMT_BGR8: 3, ORBX_FMT_RGB8: 3, ORBX_FMT_BGRA8: 4, ORBX_FMT_RGBA8: 4}


class OrbxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("orbx status %d: %s" % (code, msg))
        self.code = code


def build(verbose=False):
    """Compile lib/liborbx.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", PKG_DIR] + ([] if verbose else ["-s"]))
    return LIB_PATH


_lib = None


def lib():
    """The loaded C-ABI library.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OrbxError(ORBX_E_HIP, "%s is missing: run __graft_entry__.build() / make -C my-slam_amd" % LIB_PATH)
    try:
        # PyTorch-ROCm wheels carry their own libamdhip64; whichever copy is mapped first serves the whole
        # process.  Loading torch first keeps `torch.cuda` usable next to liborbx (bench.py, tests).
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.orbx_create.argtypes = [C.POINTER(vp), C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.orbx_create.restype = C.c_int
    L.orbx_destroy.argtypes = [vp]
    L.orbx_destroy.restype = None
    L.orbx_set_option.argtypes = [vp, C.c_int, C.c_int]
    L.orbx_get_levels.argtypes = [vp]
    L.orbx_set_input_format.argtypes = [vp, C.c_int]
    L.orbx_set_input_format.restype = C.c_int
    L.orbx_get_input_format.argtypes = [vp]
    L.orbx_get_input_format.restype = C.c_int
    L.orbx_get_scale_factor.argtypes = [vp]
    L.orbx_get_scale_factor.restype = C.c_float
    L.orbx_get_tables.argtypes = [vp, vp, vp, vp, vp]
    L.orbx_get_features_per_level.argtypes = [vp, vp]
    L.orbx_capacity.argtypes = [vp]
    L.orbx_extract.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, ip]
    L.orbx_extract_begin.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.orbx_extract_begin.restype = C.c_int
    L.orbx_extract_end.argtypes = [vp, vp, vp, C.c_int, ip]
    L.orbx_extract_end.restype = C.c_int
    L.orbx_extract_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, C.c_int, vp]
    L.orbx_extract_batch_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, C.c_int, vp, vp, vp]
    L.orbx_level_size.argtypes = [vp, C.c_int, ip, ip]
    L.orbx_download_level.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int]
    L.orbx_extract_batch_multi.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, C.c_int, vp]
    L.orbx_extract_batch_multi.restype = C.c_int
    L.orbx_download_pyramid.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    L.orbx_download_pyramid.restype = C.c_int
    L.orbx_download_candidates.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int]
    L.orbx_last_stage_ms.argtypes = [vp, vp]
    L.orbx_set_profiling.argtypes = [vp, C.c_int]
    L.orbx_stage_ms_ring.argtypes = [vp, vp, C.c_int]
    L.orbx_last_error.restype = C.c_char_p
    L.orbx_version.restype = C.c_char_p
    L.orbx_debug_sincos.argtypes = [vp, vp, vp, C.c_int]
    L.orbx_stereo_matches.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_float, C.c_float, vp, vp]
    L.orbx_stereo_matches.restype = C.c_int
    for name in ("orbx_set_option", "orbx_get_levels", "orbx_get_tables", "orbx_get_features_per_level",
                 "orbx_capacity", "orbx_extract", "orbx_extract_batch", "orbx_extract_batch_device",
                 "orbx_level_size", "orbx_download_level", "orbx_download_candidates", "orbx_last_stage_ms",
                 "orbx_set_profiling", "orbx_debug_sincos"):
        getattr(L, name).restype = C.c_int
    _bind_matcher(L)
    _bind_voc(L)
    _bind_pose(L)
    _bind_sim3(L)
    _bind_init(L)
    _bind_kfdb(L)
    _lib = L
    return L


def _bind_voc(L):
    vp = C.c_void_p
    if not hasattr(L, "orbv_load_text"):
        return
    L.orbv_load_text.argtypes = [C.POINTER(vp), C.c_char_p, C.c_int]
    L.orbv_destroy.argtypes = [vp]
    L.orbv_destroy.restype = None
    L.orbv_info.argtypes = [vp] + [C.POINTER(C.c_int)] * 6
    L.orbv_transform_features.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.orbv_bow_vector.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int]
    L.orbv_feature_vector.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int]
    L.orbv_score_l1.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int]
    L.orbv_score_l1.restype = C.c_double
    L.orbv_last_error.restype = C.c_char_p
    for name in ("orbv_load_text", "orbv_info", "orbv_transform_features", "orbv_bow_vector", "orbv_feature_vector"):
        getattr(L, name).restype = C.c_int


def _bind_kfdb(L):
    vp, ip, u64 = C.c_void_p, C.POINTER(C.c_int), C.c_uint64
    if not hasattr(L, "orbk_create"):
        return
    L.orbk_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.orbk_destroy.argtypes = [vp]
    L.orbk_destroy.restype = None
    L.orbk_add.argtypes = [vp, u64, vp, vp, C.c_int]
    L.orbk_erase.argtypes = [vp, u64]
    L.orbk_clear.argtypes = [vp]
    L.orbk_size.argtypes = [vp]
    L.orbk_score.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, ip]
    L.orbk_query_begin.argtypes = [vp, C.c_int, u64, vp, vp, C.c_int, vp, C.c_int, C.c_float, vp, vp, C.c_int, ip]
    L.orbk_query_end.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, ip]
    L.orbk_last_error.restype = C.c_char_p
    for name in ("orbk_create", "orbk_add", "orbk_erase", "orbk_clear", "orbk_size", "orbk_score", "orbk_query_begin",
                 "orbk_query_end"):
        getattr(L, name).restype = C.c_int


RAND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)


def _bind_pose(L):
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    if not hasattr(L, "orbp_pnp_create"):
        return
    L.orbp_pnp_create.argtypes = [C.POINTER(vp), C.c_int, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float]
    L.orbp_pnp_destroy.argtypes = [vp]
    L.orbp_pnp_destroy.restype = None
    L.orbp_pnp_set_rand.argtypes = [vp, RAND_FN, vp, C.c_int]
    L.orbp_pnp_set_rand.restype = None
    L.orbp_pnp_set_ransac_parameters.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
    L.orbp_pnp_get_ransac_state.argtypes = [vp, ip, ip, C.POINTER(C.c_float), ip]
    L.orbp_pnp_get_ransac_state.restype = None
    L.orbp_pnp_iterate.argtypes = [vp, C.c_int, ip, vp, ip, vp]
    L.orbp_pnp_find.argtypes = [vp, vp, ip, vp]
    L.orbp_epnp.argtypes = [C.c_int, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp]
    L.orbp_epnp.restype = C.c_double
    L.orbp_pose_optimization.argtypes = [C.c_int, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp]
    L.orbp_pnp_get_problem.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbp_pnp_draw.argtypes = [vp, C.c_int, vp]
    L.orbp_pnp_queued.argtypes = [vp, vp]
    L.orbp_pnp_hypothesis.argtypes = [vp, vp, vp, vp, vp, ip]
    L.orbp_pnp_attach_results.argtypes = [vp, C.c_int, vp, vp, vp]
    L.orbm_pnp_hypotheses.argtypes = [vp, C.c_int] + [vp] * 11
    L.orbm_pnp_hypotheses_device.argtypes = [vp, C.c_int, C.c_int] + [vp] * 12
    L.orbm_pnp_hypotheses.restype = L.orbm_pnp_hypotheses_device.restype = C.c_int
    L.orbp_optimize_sim3.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_int, vp, vp]
    L.orbp_sim3_from_rts.argtypes = [vp, vp, C.c_float, vp]
    L.orbp_optimize_sim3.restype = L.orbp_sim3_from_rts.restype = C.c_int
    L.orbp_local_bundle_adjustment.argtypes = [vp] * 6
    L.orbm_local_bundle_adjustment.argtypes = [vp] * 7
    L.orbp_local_bundle_adjustment.restype = L.orbm_local_bundle_adjustment.restype = C.c_int
    L.orbm_local_bundle_adjustment_split.argtypes = [vp] * 9
    L.orbm_local_bundle_adjustment_split.restype = C.c_int
    L.orbp_bundle_adjustment.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.orbm_bundle_adjustment.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.orbm_bundle_adjustment_split.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.orbp_bundle_adjustment.restype = L.orbm_bundle_adjustment.restype = L.orbm_bundle_adjustment_split.restype = C.c_int
    L.orbp_optimize_essential_graph.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.orbm_optimize_essential_graph.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    L.orbm_optimize_essential_graph_split.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.orbp_optimize_essential_graph.restype = L.orbm_optimize_essential_graph.restype = C.c_int
    L.orbm_optimize_essential_graph_split.restype = C.c_int
    L.orbp_eg_set_dense.argtypes = [C.c_int]
    L.orbp_eg_set_dense.restype = None
    L.orbm_spd_solve_f64.argtypes = [vp, vp, vp, C.c_int, vp, ip]
    L.orbm_spd_solve_f64.restype = C.c_int
    L.orbp_lba_set_stop_probe.argtypes = [vp, vp]
    L.orbp_lba_set_stop_probe.restype = None
    L.orbp_last_error.restype = C.c_char_p
    for name in ("orbp_pnp_create", "orbp_pnp_set_ransac_parameters", "orbp_pnp_iterate", "orbp_pnp_find",
                 "orbp_pose_optimization", "orbp_pnp_get_problem", "orbp_pnp_draw", "orbp_pnp_queued", "orbp_pnp_hypothesis",
                 "orbp_pnp_attach_results"):
        getattr(L, name).restype = C.c_int


def _bind_sim3(L):
    vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)
    L.orbp_sim3_create.argtypes = [C.POINTER(vp), C.c_int, vp, vp, vp, vp, vp, vp, C.c_int]
    L.orbp_sim3_destroy.argtypes = [vp]
    L.orbp_sim3_destroy.restype = None
    L.orbp_sim3_set_rand.argtypes = [vp, RAND_FN, vp, C.c_int]
    L.orbp_sim3_set_rand.restype = None
    L.orbp_sim3_set_ransac_parameters.argtypes = [vp, C.c_double, C.c_int, C.c_int]
    L.orbp_sim3_get_ransac_state.argtypes = [vp, ip, ip, fp, ip, ip]
    L.orbp_sim3_get_ransac_state.restype = None
    L.orbp_sim3_get_problem.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbp_sim3_draw.argtypes = [vp, C.c_int, vp]
    L.orbp_sim3_queued.argtypes = [vp, vp]
    L.orbp_sim3_hypothesis.argtypes = [vp, vp, vp, vp, fp, vp, ip]
    L.orbp_sim3_attach_results.argtypes = [vp, C.c_int, vp, vp, vp]
    L.orbp_sim3_iterate.argtypes = [vp, C.c_int, ip, vp, ip, vp]
    L.orbp_sim3_find.argtypes = [vp, vp, ip, vp]
    L.orbp_sim3_get_estimated.argtypes = [vp, vp, vp, fp]
    L.orbp_sim3_math.argtypes = [C.c_int, C.c_double, C.c_double]
    L.orbp_sim3_math.restype = C.c_double
    for name in ("orbp_sim3_create", "orbp_sim3_set_ransac_parameters", "orbp_sim3_get_problem", "orbp_sim3_draw", "orbp_sim3_queued",
                 "orbp_sim3_hypothesis", "orbp_sim3_attach_results", "orbp_sim3_iterate", "orbp_sim3_find", "orbp_sim3_get_estimated"):
        getattr(L, name).restype = C.c_int
    L.orbm_sim3_hypotheses.argtypes = [vp, C.c_int] + [vp] * 12
    L.orbm_sim3_hypotheses_device.argtypes = [vp, C.c_int, C.c_int] + [vp] * 13
    L.orbm_sim3_hypotheses.restype = L.orbm_sim3_hypotheses_device.restype = C.c_int


def _bind_init(L):
    vp, ip, fp, f = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_float
    L.orbp_init_create.argtypes = [C.POINTER(vp), vp, C.c_int, f, f, f, f, f, C.c_int]
    L.orbp_init_destroy.argtypes = [vp]
    L.orbp_init_destroy.restype = None
    L.orbp_init_set_rand.argtypes = [vp, RAND_FN, vp, C.c_int]
    L.orbp_init_set_rand.restype = None
    L.orbp_init_set_current.argtypes = [vp, vp, C.c_int, vp]
    L.orbp_init_get_sizes.argtypes = [vp, ip, ip, ip, ip, ip]
    L.orbp_init_draw.argtypes = [vp, vp]
    L.orbp_init_get_problem.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.orbp_init_normalized.argtypes = [vp, vp, vp, vp, vp]
    L.orbp_init_hypothesis.argtypes = [vp, C.c_int, vp, vp, fp, vp, ip]
    L.orbp_init_attach_results.argtypes = [vp, C.c_int, vp, vp, vp]
    L.orbp_init_find.argtypes = [vp, C.c_int, vp, fp, vp, ip]
    L.orbp_init_motions.argtypes = [vp, C.c_int, vp, vp, ip]
    L.orbp_init_check_rt.argtypes = [vp, vp, vp, vp, vp, vp, fp, ip]
    L.orbp_init_check_rt_matches.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.orbp_init_attach_check_rt.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.orbp_init_plan_check_rt.argtypes = [vp, ip, vp, vp, vp, ip]
    L.orbp_init_initialize.argtypes = [vp, vp, vp, vp, vp]
    for name in ("create", "set_current", "get_sizes", "draw", "get_problem", "normalized", "hypothesis", "attach_results", "find", "motions",
                 "check_rt", "check_rt_matches", "attach_check_rt", "plan_check_rt", "initialize"):
        getattr(L, "orbp_init_" + name).restype = C.c_int
    L.orbm_init_hypotheses.argtypes = [vp, C.c_int] + [vp] * 11
    L.orbm_init_hypotheses_device.argtypes = [vp, C.c_int, C.c_int] + [vp] * 12
    L.orbm_init_check_rt.argtypes = [vp, C.c_int, vp, vp, vp, f, C.c_int, vp, vp, vp, vp]
    L.orbm_init_check_rt_device.argtypes = [vp, C.c_int, vp, vp, vp, f, C.c_int, vp, vp, vp, vp, vp]
    L.orbm_init_hypotheses.restype = L.orbm_init_hypotheses_device.restype = C.c_int
    L.orbm_init_check_rt.restype = L.orbm_init_check_rt_device.restype = C.c_int


def _bind_matcher(L):
    vp = C.c_void_p
    if not hasattr(L, "orbm_create"):
        return
    L.orbm_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int]
    L.orbm_destroy.argtypes = [vp]
    L.orbm_destroy.restype = None
    L.orbm_distance.argtypes = [vp, vp]
    L.orbm_best2.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
    L.orbm_distances.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.orbm_best2_batch_device.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.orbm_match_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp]
    L.orbm_grid_build.argtypes = [vp, vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]
    L.orbm_grid_count.argtypes = [vp]
    L.orbm_features_in_area.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int]
    L.orbm_search_area_best2.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.orbm_search_area_best2_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.orbm_rot_filter.argtypes = [vp, vp, vp, C.c_int]
    L.orbm_search_by_bow.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int,
                                     vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp, vp]
    L.orbm_three_maxima.argtypes = [vp, C.c_int, vp]
    L.orbm_search_for_initialization.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_float, C.c_int, vp, vp]
    L.orbm_search_for_initialization.restype = C.c_int
    L.orbm_search_by_projection_last.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float,
                                                 C.c_float, C.c_float, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_float, C.c_int, C.c_int, vp, vp, vp]
    L.orbm_search_by_projection_last.restype = C.c_int
    L.orbm_search_by_projection_map.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int,
                                                C.c_float, C.c_float, vp, vp, vp]
    L.orbm_search_by_projection_map.restype = C.c_int
    L.orbm_project_points.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.orbm_project_points.restype = C.c_int
    L.orbm_predict_scale.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int]
    L.orbm_predict_scale.restype = C.c_int
    L.orbm_search_by_projection_kf.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_float, C.c_int, C.c_int,
                                               vp, vp, vp]
    L.orbm_search_by_projection_kf.restype = C.c_int
    L.orbm_undistort_keypoints.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, vp, C.c_int, vp]
    L.orbm_undistort_keypoints.restype = C.c_int
    L.orbm_image_bounds.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, vp, C.c_int, vp]
    L.orbm_image_bounds.restype = C.c_int
    f = C.c_float
    L.orbm_reserve.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.orbm_grid_build_kf.argtypes = [vp, vp, C.c_int, f, f, f, f, f, f]
    L.orbm_sim3_decompose.argtypes = [vp, vp, vp]
    L.orbm_sim3_relative.argtypes = [f, vp, vp, vp, vp, vp]
    L.orbm_project_points_kf.argtypes = [vp, vp, f, f, f, f, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.orbm_project_points_sim3.argtypes = [vp, vp, vp, f, f, f, f, vp, vp, C.c_int, vp, vp, vp, vp]
    L.orbm_search_by_projection_sim3.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.orbm_search_by_bow_kf.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int,
                                        vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, f, C.c_int, vp, vp]
    L.orbm_search_for_triangulation.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int,
                                                vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int,
                                                vp, vp, f, f, f, f, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.orbm_fuse.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, f, vp, vp]
    L.orbm_fuse_sim3.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, f, vp, vp]
    L.orbm_search_by_sim3.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp,
                                      vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, f, vp, vp]
    L.orbm_distinctive_descriptors.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.orbm_distinctive_descriptors_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.orbm_distinctive_descriptors.restype = L.orbm_distinctive_descriptors_device.restype = C.c_int
    L.orbm_triangulate_matches.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp]
    L.orbm_triangulate_matches_device.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
    L.orbm_triangulate_matches.restype = L.orbm_triangulate_matches_device.restype = C.c_int
    L.orbm_create_new_map_points.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int,
                                             vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.orbm_create_new_map_points.restype = C.c_int
    L.orbm_frustum.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_frustum_device.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_search_local_points.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_float,
                                           vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_frustum.restype = L.orbm_frustum_device.restype = L.orbm_search_local_points.restype = C.c_int
    L.orbm_pose_optimization_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_pose_optimization_batch_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_pose_optimization_batch.restype = L.orbm_pose_optimization_batch_device.restype = C.c_int
    L.orbm_optimize_sim3_batch.argtypes = [vp, C.c_int] + [vp] * 13
    L.orbm_optimize_sim3_batch_device.argtypes = [vp, C.c_int] + [vp] * 14
    L.orbm_optimize_sim3_batch.restype = L.orbm_optimize_sim3_batch_device.restype = C.c_int
    L.orbm_search_by_bow_batch.argtypes = [vp, vp, C.c_int, vp, f, C.c_int, vp, vp]
    L.orbm_search_by_bow_kf_batch.argtypes = [vp, vp, vp, C.c_int, f, C.c_int, vp, vp]
    L.orbm_search_by_bow_batch.restype = L.orbm_search_by_bow_kf_batch.restype = C.c_int
    L.orbm_fuse_views.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, f, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_fuse_views.restype = C.c_int
    for name in ("orbm_reserve", "orbm_grid_build_kf", "orbm_sim3_decompose", "orbm_sim3_relative", "orbm_project_points_kf",
                 "orbm_project_points_sim3", "orbm_search_by_projection_sim3", "orbm_search_by_bow_kf", "orbm_search_for_triangulation",
                 "orbm_fuse", "orbm_fuse_sim3", "orbm_search_by_sim3", "orbm_search_by_bow"):
        getattr(L, name).restype = C.c_int
    L.orbm_last_error.restype = C.c_char_p
    for name in ("orbm_create", "orbm_distance", "orbm_best2", "orbm_distances", "orbm_best2_batch_device",
                 "orbm_match_batch_device", "orbm_rot_filter", "orbm_three_maxima", "orbm_grid_build",
                 "orbm_features_in_area", "orbm_search_area_best2", "orbm_search_area_best2_device", "orbm_grid_count"):
        getattr(L, name).restype = C.c_int


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class BowSide(C.Structure):
    """orbm_bow_side (include/orbm.h): one side of a batched SearchByBoW"""
    _fields_ = [("desc", C.c_void_p), ("kps", C.c_void_p), ("n", C.c_int32), ("valid", C.c_void_p),
                ("fv_node", C.c_void_p), ("fv_off", C.c_void_p), ("fv_idx", C.c_void_p), ("fv_n", C.c_int32)]


def bow_sides(sides):
    """(kps, desc, featvec, valid) tuples -> (array of orbm_bow_side, the arrays it points into: keep them alive for the call)"""
    arr = (BowSide * max(len(sides), 1))()
    keep = []
    for k, (kps, desc, featvec, valid) in enumerate(sides):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        node, off, idx = [np.ascontiguousarray(a, np.int32) for a in featvec]
        valid = None if valid is None else np.ascontiguousarray(valid, np.uint8)
        if len(kps) != len(desc) or (valid is not None and len(valid) != len(desc)) or len(off) != len(node) + 1:
            raise OrbxError(ORBX_E_INVALID, "side %d: %d keypoints, %d descriptors, %d node ids, %d offsets" % (k, len(kps), len(desc), len(node), len(off)))
        keep.append((desc, kps, node, off, idx, valid))
        a = lambda x: x.ctypes.data if x is not None and x.size else None
        arr[k] = BowSide(a(desc), a(kps), len(desc), a(valid), a(node), off.ctypes.data, a(idx), len(node))
    return arr, keep


def _chk(rc):
    if rc != ORBX_OK:
        raise OrbxError(rc, lib().orbx_last_error().decode())


class ORBextractor:
    """Python mirror of ORB_SLAM2::ORBextractor (include/ORBextractor.h:46-112) over the C ABI."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7,
                 device=0, max_width=640, max_height=480, max_batch=1):
        self.L = lib()
        self.h = C.c_void_p()
        _chk(self.L.orbx_create(C.byref(self.h), nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST,
                                device, max_width, max_height, max_batch))
        self.nlevels = nlevels
        self.max_batch = max_batch
        self.cap = self.L.orbx_capacity(self.h)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.orbx_destroy(self.h)
            self.h = None

    __del__ = close

    # getters (include/ORBextractor.h:63-83)
    def GetLevels(self):
        return self.L.orbx_get_levels(self.h)

    def GetScaleFactor(self):
        return self.L.orbx_get_scale_factor(self.h)

    def _tables(self):
        t = [np.zeros(self.nlevels, np.float32) for _ in range(4)]
        _chk(self.L.orbx_get_tables(self.h, *[_p(a) for a in t]))
        return t

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def features_per_level(self):
        q = np.zeros(self.nlevels, np.int32)
        _chk(self.L.orbx_get_features_per_level(self.h, _p(q)))
        return q

    def set_blur_rounding(self, mode):
        _chk(self.L.orbx_set_option(self.h, ORBX_OPT_BLUR_ROUNDING, mode))

    def set_subbatches(self, n):
        _chk(self.L.orbx_set_option(self.h, ORBX_OPT_SUBBATCHES, n))

    def set_batch_chunk(self, frames):
        """Frames per chunk of extract_batch's upload / extract / download pipeline (0 = one piece)."""
        _chk(self.L.orbx_set_option(self.h, ORBX_OPT_BATCH_CHUNK, int(frames)))

    def set_overlap_pyramid(self, on):
        _chk(self.L.orbx_set_option(self.h, ORBX_OPT_OVERLAP_PYRAMID, int(on)))

    def set_input_format(self, fmt):
        """ORBX_FMT_GRAY8 (default) or a colour format: every extraction entry point then takes (..., H, W, 3|4) uint8 frames."""
        _chk(self.L.orbx_set_input_format(self.h, int(fmt)))

    @property
    def input_format(self):
        return self.L.orbx_get_input_format(self.h)

    def _check_frames(self, a, batch):
        """The array's shape against the handle's format: (H, W) grey or (H, W, cn) colour, one more leading axis for a batch."""
        cn = _FMT_CHANNELS[self.input_format]
        want = (2 if cn == 1 else 3) + (1 if batch else 0)
        if a.dtype != np.uint8 or a.ndim != want or (cn > 1 and a.shape[-1] != cn):
            raise OrbxError(ORBX_E_INVALID, "input format %d takes uint8 arrays of shape (%sH, W%s), got %s %s"
                            % (self.input_format, "B, " if batch else "", ", %d" % cn if cn > 1 else "", a.dtype, a.shape))
        return cn

    def set_profiling(self, on):
        _chk(self.L.orbx_set_profiling(self.h, int(on)))

    def stage_ms(self):
        ms = np.zeros(4, np.float32)
        _chk(self.L.orbx_last_stage_ms(self.h, _p(ms)))
        return ms

    def stage_ms_ring(self, max_calls=16):
        """Stage times of the last calls under set_profiling(2) (rows: newest first; the stream must be synchronised)."""
        ms = np.zeros((max_calls, 4), np.float32)
        n = self.L.orbx_stage_ms_ring(self.h, _p(ms), max_calls)
        _chk(min(n, 0))
        return ms[:n]

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors) -> (keypoints[KP_DTYPE], descriptors[n,32])."""
        if image is None or image.size == 0:
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        if self.input_format != ORBX_FMT_GRAY8 or image.ndim != 2:
            cn = self._check_frames(image, False)
            if image.strides[1] != cn or image.strides[2] != 1:
                image = np.ascontiguousarray(image)
        else:
            assert image.dtype == np.uint8 and image.ndim == 2   # assert(image.type() == CV_8UC1), :1052
            if image.strides[1] != 1:
                image = np.ascontiguousarray(image)
        H, W = image.shape[:2]
        kps = np.zeros(self.cap, KP_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        n = C.c_int()
        _chk(self.L.orbx_extract(self.h, _p(image), W, H, image.strides[0], _p(kps), _p(desc), self.cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_begin(self, image):
        """First half of __call__: stage + enqueue, no wait (include/orbx.h: orbx_extract_begin)."""
        if image is None or image.size == 0:
            _chk(self.L.orbx_extract_begin(self.h, None, 0, 0, 0))
            return
        if self.input_format != ORBX_FMT_GRAY8 or image.ndim != 2:
            cn = self._check_frames(image, False)
            assert image.strides[1] == cn and image.strides[2] == 1
        else:
            assert image.dtype == np.uint8 and image.ndim == 2 and image.strides[1] == 1
        _chk(self.L.orbx_extract_begin(self.h, image.ctypes.data_as(C.c_void_p), image.shape[1], image.shape[0], image.strides[0]))

    def extract_end(self):
        """Second half: wait and return (keypoints, descriptors)."""
        kps = np.zeros(self.cap, KP_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        n = C.c_int(0)
        _chk(self.L.orbx_extract_end(self.h, _p(kps), _p(desc), self.cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_batch(self, images):
        images = np.ascontiguousarray(images, dtype=np.uint8)
        if self.input_format != ORBX_FMT_GRAY8 or images.ndim != 3:
            self._check_frames(images, True)
        B, H, W = images.shape[:3]
        kps = np.zeros((B, self.cap), KP_DTYPE)
        desc = np.zeros((B, self.cap, 32), np.uint8)
        counts = np.zeros(B, np.int32)
        _chk(self.L.orbx_extract_batch(self.h, _p(images), B, W, H, images.strides[1], images.strides[0],
                                       _p(kps), _p(desc), self.cap, _p(counts)))
        return [(kps[k, :counts[k]].copy(), desc[k, :counts[k]].copy()) for k in range(B)]

    def extract_batch_raw(self, images):
        """orbx_extract_batch without the per-frame slicing: (kps [B,cap], desc [B,cap,32], counts [B]).  A row / frame
        pitch larger than the width (a view into a bigger array) is passed through as it is.
        The three arrays are this object's reusable buffers (the zero-allocation benchmark path): the next call with the same
        batch size overwrites them in place, so copy what must survive it; rows at and beyond counts[f] are stale data of
        earlier calls."""
        images = np.asarray(images, dtype=np.uint8)
        if self.input_format != ORBX_FMT_GRAY8 or images.ndim != 3:
            cn = self._check_frames(images, True)
            if images.strides[3] != 1 or images.strides[2] != cn or images.strides[1] < images.shape[2] * cn or \
                    images.strides[0] < images.strides[1] * (images.shape[1] - 1) + images.shape[2] * cn:
                images = np.ascontiguousarray(images)
        elif images.strides[2] != 1 or images.strides[1] < images.shape[2] or images.strides[0] < images.strides[1] * (images.shape[1] - 1) + images.shape[2]:
            images = np.ascontiguousarray(images)
        B, H, W = images.shape[:3]
        if getattr(self, "_raw", None) is None or self._raw[0].shape[0] != B:
            self._raw = (np.zeros((B, self.cap), KP_DTYPE), np.zeros((B, self.cap, 32), np.uint8), np.zeros(B, np.int32))
        kps, desc, counts = self._raw
        _chk(self.L.orbx_extract_batch(self.h, _p(images), B, W, H, images.strides[1], images.strides[0],
                                       _p(kps), _p(desc), self.cap, _p(counts)))
        return kps, desc, counts

    def extract_batch_device(self, d_images_ptr, B, W, H, row_stride, frame_stride,
                             d_kps_ptr, d_desc_ptr, d_counts_ptr, d_status_ptr, stream=None):
        """All pointers are device addresses (e.g. torch tensor .data_ptr()); asynchronous."""
        _chk(self.L.orbx_extract_batch_device(self.h, d_images_ptr, B, W, H, row_stride, frame_stride,
                                              d_kps_ptr, d_desc_ptr, self.cap, d_counts_ptr, d_status_ptr, stream))

    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        _chk(self.L.orbx_level_size(self.h, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def image_pyramid(self, frame=0, border=0):
        """mvImagePyramid of the last call (host copies)."""
        out = []
        for l in range(self.nlevels):
            w, h = self.level_size(l)
            a = np.zeros((h + 2 * border, w + 2 * border), np.uint8)
            _chk(self.L.orbx_download_level(self.h, frame, l, _p(a), a.strides[0], border))
            out.append(a)
        return out

    def image_pyramid_all(self, frame=0, border=19):
        """All levels in one call (orbx_download_pyramid: one synchronisation), with the reference's 19-px reflect-101 border."""
        out = []
        for l in range(self.nlevels):
            w, h = self.level_size(l)
            out.append(np.zeros((h + 2 * border, w + 2 * border), np.uint8))
        ptrs = (C.c_void_p * self.nlevels)(*[a.ctypes.data for a in out])
        strides = (C.c_int * self.nlevels)(*[a.strides[0] for a in out])
        _chk(self.L.orbx_download_pyramid(self.h, frame, ptrs, strides, border))
        return out

    def candidates(self, frame, level, cap=1 << 20):
        a = np.zeros((cap, 3), np.int32)
        n = self.L.orbx_download_candidates(self.h, frame, level, _p(a), cap)
        if n < 0:
            _chk(n)
        return a[:n].copy()


def extract_batch_multi(extractors, images):
    """orbx_extract_batch_multi: one batch of host frames sharded over several ORBextractor handles (one per GPU; one host thread
    each).  Returns (kps [B, cap], desc [B, cap, 32], counts [B]) like ORBextractor.extract_batch_raw."""
    images = np.ascontiguousarray(images, dtype=np.uint8)
    if extractors[0].input_format != ORBX_FMT_GRAY8 or images.ndim != 3:
        extractors[0]._check_frames(images, True)
    B, H, W = images.shape[:3]
    cap = max(e.cap for e in extractors)
    kps = np.zeros((B, cap), KP_DTYPE); desc = np.zeros((B, cap, 32), np.uint8); counts = np.zeros(B, np.int32)
    hs = (C.c_void_p * len(extractors))(*[e.h for e in extractors])
    _chk(lib().orbx_extract_batch_multi(hs, len(extractors), _p(images), B, W, H, images.strides[1], images.strides[0],
                                        _p(kps), _p(desc), cap, _p(counts)))
    return kps, desc, counts


def ComputeStereoMatches(left, right, kl, dl, kr, dr, mb, mbf):
    """Frame::ComputeStereoMatches on the two extractors' last pyramids -> (mvuRight, mvDepth)."""
    kl = np.ascontiguousarray(kl, KP_DTYPE); kr = np.ascontiguousarray(kr, KP_DTYPE)
    dl = np.ascontiguousarray(dl, np.uint8); dr = np.ascontiguousarray(dr, np.uint8)
    u = np.zeros(len(kl), np.float32); d = np.zeros(len(kl), np.float32)
    _chk(lib().orbx_stereo_matches(left.h, right.h, _p(kl), _p(dl), len(kl), _p(kr), _p(dr), len(kr), mb, mbf, _p(u), _p(d)))
    return u, d


def debug_sincos(theta):
    theta = np.ascontiguousarray(theta, np.float32)
    c = np.empty_like(theta)
    s = np.empty_like(theta)
    _chk(lib().orbx_debug_sincos(_p(theta), _p(c), _p(s), len(theta)))
    return c, s


def _mchk(rc):
    if rc != ORBX_OK:
        raise OrbxError(rc, lib().orbm_last_error().decode())


def _device_ptrs(method, want, stream, none_ok=True):
    """The argument check of the *_device methods: want = (tensor, name of its torch dtype) pairs.  Returns (the tensors' device
    pointers, None for a None tensor; the raw stream of a torch stream, a raw hipStream_t or None)."""
    import torch
    for t, dt in want:
        if (t is None and not none_ok) or (t is not None and (not t.is_cuda or t.dtype != getattr(torch, dt) or not t.is_contiguous())):
            raise OrbxError(ORBX_E_INVALID, "%s wants contiguous device tensors of the documented dtypes" % method)
    return [None if t is None else C.c_void_p(t.data_ptr()) for t, _ in want], getattr(stream, "cuda_stream", stream)


def _cat(parts, shape, dtype):
    """The problems' arrays back to back; `shape` is that of no problem at all."""
    return np.ascontiguousarray(np.concatenate(parts), dtype) if parts else np.zeros(shape, dtype)


def _hyp_offsets(counts):
    """(off int32, hyp_off int32, mask_off int64), B + 1 entries each, from every problem's (correspondences n, hypotheses h): the
    frame of the hypothesis kernels (csrc/orbm_hyp.h), a hypothesis owning ceil(n / 32) mask words."""
    B = len(counts)
    off, hyp_off, mask_off = np.zeros(B + 1, np.int32), np.zeros(B + 1, np.int32), np.zeros(B + 1, np.int64)
    for p, (n, h) in enumerate(counts):
        off[p + 1] = off[p] + n
        hyp_off[p + 1] = hyp_off[p] + h
        mask_off[p + 1] = mask_off[p] + h * ((n + 31) // 32)
    return off, hyp_off, mask_off


def _split_hypotheses(off, hyp_off, mask_off, first, second, masks):
    """The flat results of a hypothesis call -> per problem (first [h, ...], second [h, ...], masks uint32 [h, ceil(n / 32)])."""
    out = []
    for p in range(len(off) - 1):
        h0, h1 = int(hyp_off[p]), int(hyp_off[p + 1])
        W = (int(off[p + 1]) - int(off[p]) + 31) // 32
        out.append((first[h0:h1].copy(), second[h0:h1].copy(), masks[mask_off[p]:mask_off[p + 1]].reshape(h1 - h0, W).copy()))
    return out


class ORBmatcher:
    """Python mirror of the Hamming primitives of ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:41-89)."""
    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio=0.6, checkOri=True, device=0, max_queries=8192, max_train=8192, max_pairs=1 << 22):
        self.L = lib()
        self.mfNNratio, self.mbCheckOrientation = float(nnratio), bool(checkOri)
        self.h = C.c_void_p()
        _mchk(self.L.orbm_create(C.byref(self.h), device, max_queries, max_train, max_pairs))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.orbm_destroy(self.h)
            self.h = None

    __del__ = close

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return lib().orbm_distance(_p(a), _p(b))

    def best2(self, q, t, cand_off=None, cand_idx=None):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        nq, nt = len(q), len(t)
        bi, bd, sd = (np.full(nq, -1, np.int32), np.full(nq, 256, np.int32), np.full(nq, 256, np.int32))
        if cand_off is not None:
            cand_off = np.ascontiguousarray(cand_off, np.int32)
            cand_idx = np.ascontiguousarray(cand_idx, np.int32)
        _mchk(self.L.orbm_best2(self.h, _p(q), nq, _p(t), nt, _p(cand_off), _p(cand_idx), _p(bi), _p(bd), _p(sd)))
        return bi, bd, sd

    def distances(self, q, t, cand_off=None, cand_idx=None):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        nq, nt = len(q), len(t)
        if cand_off is not None:
            cand_off = np.ascontiguousarray(cand_off, np.int32)
            cand_idx = np.ascontiguousarray(cand_idx, np.int32)
            out = np.zeros(int(cand_off[-1]), np.int32)
        else:
            out = np.zeros(nq * nt, np.int32)
        _mchk(self.L.orbm_distances(self.h, _p(q), nq, _p(t), nt, _p(cand_off), _p(cand_idx), _p(out)))
        return out

    def distinctive_descriptors(self, off, desc):
        """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) for a batch of MapPoints: point p owns the rows
        off[p]:off[p+1] of desc, in the order of its observations.  Returns (best, best_median), int32 per point: the row
        whose median distance to the point's rows is the smallest (the first such row), and that median; -1 for an empty run."""
        off = np.ascontiguousarray(off, np.int32).reshape(-1)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        if len(off) < 1 or (len(off) > 1 and int(off[-1]) != len(desc)):
            raise OrbxError(ORBX_E_INVALID, "off has %d entries ending at %s, desc has %d rows" % (len(off), off[-1:], len(desc)))
        n = len(off) - 1
        best, med = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        _mchk(self.L.orbm_distinctive_descriptors(self.h, n, _p(off), _p(desc), _p(best), _p(med)))
        return best, med

    def distinctive_descriptors_device(self, n_points, d_off, d_desc, total_rows, max_run, d_best, d_best_median=None, stream=None):
        """The same on raw device pointers; nothing is synchronised.  total_rows = off[n_points], max_run >= the longest run."""
        _mchk(self.L.orbm_distinctive_descriptors_device(self.h, n_points, d_off, d_desc, total_rows, max_run, d_best, d_best_median, stream))

    def triangulate_matches(self, cam1, kps_un1, keys_xy1, u_right1, depth1, cams2, off2, kps_un2, keys_xy2, u_right2, depth2, matches):
        """The per-match loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:288-434) for all matches in one call.
        cam1: one CAM_DTYPE record, cams2: one per second view; the second views' feature arrays are concatenated, view v owning
        off2[v]:off2[v+1]; matches: int32 [n, 3] = idx1, idx2 inside its view, view.  Returns (status uint8 [n], x3d float32
        [n, 3]): the orbm_tri_status of every match and the new point of the accepted ones (status <= 2)."""
        cam1 = np.ascontiguousarray(cam1, CAM_DTYPE).reshape(1)
        cams2 = np.ascontiguousarray(cams2, CAM_DTYPE).reshape(-1)
        off2 = np.ascontiguousarray(off2, np.int32).reshape(-1)
        k1, k2 = np.ascontiguousarray(kps_un1, KP_DTYPE), np.ascontiguousarray(kps_un2, KP_DTYPE)
        x1, x2 = np.ascontiguousarray(keys_xy1, np.float32).reshape(-1, 2), np.ascontiguousarray(keys_xy2, np.float32).reshape(-1, 2)
        u1, u2 = np.ascontiguousarray(u_right1, np.float32), np.ascontiguousarray(u_right2, np.float32)
        d1, d2 = np.ascontiguousarray(depth1, np.float32), np.ascontiguousarray(depth2, np.float32)
        matches = np.ascontiguousarray(matches, np.int32).reshape(-1, 3)
        if len(off2) != len(cams2) + 1 or not (len(k1) == len(x1) == len(u1) == len(d1)) or not (len(k2) == len(x2) == len(u2) == len(d2)) \
                or (len(off2) > 0 and int(off2[-1]) != len(k2)):
            raise OrbxError(ORBX_E_INVALID, "array lengths disagree: %d views, off2 %s, %d / %d features" % (len(cams2), off2[-1:], len(k1), len(k2)))
        n = len(matches)
        status, x3d = np.full(n, 255, np.uint8), np.zeros((n, 3), np.float32)
        _mchk(self.L.orbm_triangulate_matches(self.h, _p(cam1), _p(k1), _p(x1), _p(u1), _p(d1), len(k1), _p(cams2), len(cams2), _p(off2),
                                              _p(k2), _p(x2), _p(u2), _p(d2), _p(matches), n, _p(status), _p(x3d)))
        return status, x3d

    def triangulate_matches_device(self, d_cam1, d_kps_un1, d_keys_xy1, d_u_right1, d_depth1, n1, d_cams2, ncams2, d_off2, d_kps_un2,
                                   d_keys_xy2, d_u_right2, d_depth2, d_matches, n, d_status, d_x3d, stream=None):
        """The same on raw device pointers; nothing is synchronised.  Out-of-range indices get status 12 (ORBM_TRI_BAD_INDEX)."""
        _mchk(self.L.orbm_triangulate_matches_device(self.h, d_cam1, d_kps_un1, d_keys_xy1, d_u_right1, d_depth1, n1, d_cams2, ncams2, d_off2,
                                                     d_kps_un2, d_keys_xy2, d_u_right2, d_depth2, d_matches, n, d_status, d_x3d, stream))

    def create_new_map_points(self, cam1, kps_un1, keys_xy1, u_right1, depth1, desc1, has_mp1, featvec1, cams2, F12, off2, kps_un2,
                              keys_xy2, u_right2, depth2, desc2, has_mp2, fv2_view_off, featvec2, only_stereo=False):
        """LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:209-454) for all neighbours in one call: SearchForTriangulation
        against every second view and the per-match loop over what it found, on one snapshot.  Key frame 1 and the concatenated
        second views as for triangulate_matches, plus descriptors, has_mp flags and FeatureVectors (featvec1 = (node, off, idx);
        featvec2 = the views' (node, off, idx) concatenated, view v owning the nodes fv2_view_off[v]:fv2_view_off[v+1], indices
        inside their view) and F12 float32 [nviews, 3, 3].  Returns (matches12 int32 [nviews, n1], status uint8 [nviews, n1],
        x3d float32 [nviews, n1, 3], nmatches int32 [nviews]); status 255 (ORBM_TRI_NO_MATCH) where matches12 < 0."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
        cam1 = np.ascontiguousarray(cam1, CAM_DTYPE).reshape(1)
        cams2 = np.ascontiguousarray(cams2, CAM_DTYPE).reshape(-1)
        off2, fvo = i32(off2), i32(fv2_view_off)
        k1, k2 = np.ascontiguousarray(kps_un1, KP_DTYPE), np.ascontiguousarray(kps_un2, KP_DTYPE)
        x1, x2 = f32(keys_xy1).reshape(-1, 2), f32(keys_xy2).reshape(-1, 2)
        u1, u2, z1, z2 = f32(u_right1), f32(u_right2), f32(depth1), f32(depth2)
        d1, d2 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32), np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        h1, h2 = np.ascontiguousarray(has_mp1, np.uint8).reshape(-1), np.ascontiguousarray(has_mp2, np.uint8).reshape(-1)
        n1n, n1o, n1i = [i32(a) for a in featvec1]
        n2n, n2o, n2i = [i32(a) for a in featvec2]
        F12 = f32(F12).reshape(-1, 9)
        nv, n1 = len(cams2), len(k1)
        if len(off2) != nv + 1 or len(fvo) != nv + 1 or len(F12) != nv or not (n1 == len(x1) == len(u1) == len(z1) == len(d1) == len(h1)) \
                or not (len(k2) == len(x2) == len(u2) == len(z2) == len(d2) == len(h2) == int(off2[-1])) \
                or len(n1o) != len(n1n) + 1 or len(n2o) != len(n2n) + 1 or int(fvo[-1]) != len(n2n) or int(n1o[-1]) != len(n1i) or int(n2o[-1]) != len(n2i):
            raise OrbxError(ORBX_E_INVALID, "array lengths disagree: %d views, off2 %s, fv2_view_off %s, %d / %d features" % (nv, off2[-1:], fvo[-1:], n1, len(k2)))
        m12 = np.full((nv, n1), -1, np.int32)
        status, x3d, nm = np.full((nv, n1), 255, np.uint8), np.zeros((nv, n1, 3), np.float32), np.zeros(nv, np.int32)
        _mchk(self.L.orbm_create_new_map_points(self.h, _p(cam1), _p(k1), _p(x1), _p(u1), _p(z1), _p(d1), n1, _p(h1), _p(n1n), _p(n1o), _p(n1i), len(n1n),
                                                _p(cams2), _p(F12), nv, _p(off2), _p(k2), _p(x2), _p(u2), _p(z2), _p(d2), _p(h2), _p(fvo), _p(n2n), _p(n2o),
                                                _p(n2i), 1 if only_stereo else 0, _p(m12), _p(status), _p(x3d), _p(nm)))
        return m12, status, x3d, nm

    def fuse_views(self, views, off, kps_un, u_right, desc_kf, skip, xw, normal, mf_max, mf_min, mp_desc, th=3.0):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:825-952) for all target key frames of
        LocalMapping::SearchInNeighbors in one call, on one snapshot.  views: FUSE_VIEW_DTYPE records; the views' features
        concatenated, view v owning off[v]:off[v+1] of kps_un / u_right / desc_kf; skip uint8 [nviews, n_mp]; xw, normal, mf_max,
        mf_min (the raw mfMax / MinDistance) and mp_desc per MapPoint.  Returns (status uint8, best_idx int32, best_dist int32,
        proj_u, proj_v, proj_ur float32, pred_level int32, all [nviews, n_mp], nfused int32 [nviews]): the orbm_fuse_status of
        every slot, the feature inside its view a matched slot is fused with (-1 otherwise), and the projection of the slots that
        were searched (status MATCH or NO_MATCH)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        views = np.ascontiguousarray(views, FUSE_VIEW_DTYPE).reshape(-1)
        off = np.ascontiguousarray(off, np.int32).reshape(-1)
        kps = np.ascontiguousarray(kps_un, KP_DTYPE).reshape(-1)
        ur, dk = f32(u_right).reshape(-1), np.ascontiguousarray(desc_kf, np.uint8).reshape(-1, 32)
        xw, normal, mx, mn = f32(xw).reshape(-1, 3), f32(normal).reshape(-1, 3), f32(mf_max).reshape(-1), f32(mf_min).reshape(-1)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        nv, n = len(views), len(xw)
        skip = np.ascontiguousarray(skip, np.uint8).reshape(-1)
        if len(off) != nv + 1 or not (len(kps) == len(ur) == len(dk) == int(off[-1])) or not (len(normal) == len(mx) == len(mn) == len(md) == n) \
                or len(skip) != nv * n:
            raise OrbxError(ORBX_E_INVALID, "array lengths disagree: %d views, off %s, %d / %d / %d features, %d MapPoints, %d skip flags"
                            % (nv, off[-1:], len(kps), len(ur), len(dk), n, len(skip)))
        status = np.full((nv, n), 255, np.uint8)
        bi, bd, lv = np.full((nv, n), -1, np.int32), np.full((nv, n), 256, np.int32), np.zeros((nv, n), np.int32)
        pu, pv, pr = np.zeros((nv, n), np.float32), np.zeros((nv, n), np.float32), np.zeros((nv, n), np.float32)
        nf = np.zeros(nv, np.int32)
        _mchk(self.L.orbm_fuse_views(self.h, _p(views), nv, _p(off), _p(kps), _p(ur), _p(dk), n, _p(skip), _p(xw), _p(normal), _p(mx), _p(mn),
                                     _p(md), C.c_float(th), _p(status), _p(bi), _p(bd), _p(pu), _p(pv), _p(pr), _p(lv), _p(nf)))
        return status, bi, bd, pu, pv, pr, lv, nf

    @staticmethod
    def _frustum_inputs(view, skip, xw, normal, mf_max, mf_min):
        view = np.ascontiguousarray(view, VIEW_DTYPE).reshape(1)
        skip = np.ascontiguousarray(skip, np.uint8).reshape(-1)
        xw, normal = np.ascontiguousarray(xw, np.float32).reshape(-1, 3), np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        mf_max, mf_min = np.ascontiguousarray(mf_max, np.float32).reshape(-1), np.ascontiguousarray(mf_min, np.float32).reshape(-1)
        n = len(skip)
        if not (len(xw) == len(normal) == len(mf_max) == len(mf_min) == n):
            raise OrbxError(ORBX_E_INVALID, "array lengths disagree: %d / %d / %d / %d / %d" % (n, len(xw), len(normal), len(mf_max), len(mf_min)))
        out = (np.full(n, 255, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32),
               np.zeros(n, np.float32))
        return (view, skip, xw, normal, mf_max, mf_min), out, n

    def frustum(self, view, skip, xw, normal, mf_max, mf_min, viewing_cos_limit=0.5):
        """Frame::isInFrustum (src/Frame.cc:269-325) for the local MapPoints of Tracking::SearchLocalPoints (src/Tracking.cc:1174-1187)
        in one call.  view: one VIEW_DTYPE record; skip[i] = mnLastFrameSeen == mnId or isBad(); mf_max / mf_min: the raw
        mfMaxDistance / mfMinDistance.  Returns (status uint8, proj_x, proj_y, proj_xr float32, pred_level int32, view_cos float32,
        n_to_match): the orbm_frustum_status of every point and the mTrack* values of the ones in view (status 0)."""
        a, out, n = self._frustum_inputs(view, skip, xw, normal, mf_max, mf_min)
        nt = C.c_int(0)
        _mchk(self.L.orbm_frustum(self.h, _p(a[0]), n, _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), _p(a[5]), C.c_float(viewing_cos_limit),
                                  *[_p(o) for o in out], C.byref(nt)))
        return out + (nt.value,)

    def frustum_device(self, d_view, n, d_skip, d_xw, d_normal, d_mf_max, d_mf_min, viewing_cos_limit, d_status, d_proj_x, d_proj_y,
                       d_proj_xr, d_pred_level, d_view_cos, stream=None):
        """The same on raw device pointers (the view block included); nothing is synchronised and nothing is counted."""
        _mchk(self.L.orbm_frustum_device(self.h, d_view, n, d_skip, d_xw, d_normal, d_mf_max, d_mf_min, C.c_float(viewing_cos_limit),
                                         d_status, d_proj_x, d_proj_y, d_proj_xr, d_pred_level, d_view_cos, stream))

    @staticmethod
    def pack_pose_problems(problems):
        """The CSR arrays of orbm_pose_optimization_batch from a list of PoseOptimization argument tuples
        (obs, inv_sigma2, xw, fx, fy, cx, cy, Tcw[, u_right[, bf]]) -> (off int32 [B+1], obs float32 [N, 2], u_right float32 [N] or
        None when no problem has one, inv_sigma2 float32 [N], xw float32 [N, 3], cams POSE_CAM_DTYPE [B], Tcw float32 [B, 16]).
        A problem without u_right gets -1 (monocular) on all its edges when another problem has one."""
        B = len(problems)
        off = np.zeros(B + 1, np.int32)
        cams, T = np.zeros(B, POSE_CAM_DTYPE), np.zeros((B, 16), np.float32)
        obs, s2, xw, ur = [], [], [], []
        for p, args in enumerate(problems):
            o, s, x, fx, fy, cx, cy, Tcw = args[:8]
            u = args[8] if len(args) > 8 else None
            bf = args[9] if len(args) > 9 else 0.0
            o = np.ascontiguousarray(o, np.float32).reshape(-1, 2)
            s = np.ascontiguousarray(s, np.float32).reshape(-1)
            x = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
            u = None if u is None else np.ascontiguousarray(u, np.float32).reshape(-1)
            if not (len(o) == len(s) == len(x)) or (u is not None and len(u) != len(o)):
                raise OrbxError(ORBX_E_INVALID, "problem %d: array lengths disagree: %d / %d / %d" % (p, len(o), len(s), len(x)))
            obs.append(o); s2.append(s); xw.append(x); ur.append(u)
            off[p + 1] = off[p] + len(o)
            cams[p] = (fx, fy, cx, cy, bf)
            T[p] = np.asarray(Tcw, np.float32).reshape(16)
        f32 = np.float32
        u_all = None
        if any(u is not None for u in ur):
            u_all = _cat([u if u is not None else np.full(len(o), -1, f32) for u, o in zip(ur, obs)], (0,), f32)
        return off, _cat(obs, (0, 2), f32), u_all, _cat(s2, (0,), f32), _cat(xw, (0, 3), f32), cams, T

    def pose_optimization_batch(self, problems):
        """Optimizer::PoseOptimization (src/Optimizer.cc:239-451) for a list of independent problems in one launch, each an argument
        tuple of PoseOptimization().  Returns a list of PoseOptimization()'s results: (Tcw 4x4 float32, mvbOutlier bool[n], n_inliers)."""
        off, obs, ur, s2, xw, cams, T = self.pack_pose_problems(problems)
        B = len(problems)
        out, good = np.zeros(max(int(off[-1]), 1), np.uint8), np.zeros(max(B, 1), np.int32)
        _mchk(self.L.orbm_pose_optimization_batch(self.h, B, _p(off), _p(obs), _p(ur), _p(s2), _p(xw), _p(cams), _p(T), _p(out), _p(good)))
        return [(T[p].reshape(4, 4).copy(), out[off[p]:off[p + 1]].astype(bool), int(good[p])) for p in range(B)]

    def pose_optimization_batch_device(self, n_problems, off, obs, u_right, inv_sigma2, xw, cams, Tcw, outlier, n_good, stream=None):
        """The same on torch tensors on the handle's device: off int32 [B+1], obs float32 [N, 2], u_right float32 [N] or None,
        inv_sigma2 float32 [N], xw float32 [N, 3], cams float32 [B, 5] (fx, fy, cx, cy, bf), Tcw float32 [B, 16] (in/out),
        outlier uint8 [N], n_good int32 [B].  Nothing is copied or synchronised; stream: a torch stream, a raw hipStream_t or None
        (the handle's stream)."""
        want = ((off, "int32"), (obs, "float32"), (u_right, "float32"), (inv_sigma2, "float32"), (xw, "float32"), (cams, "float32"),
                (Tcw, "float32"), (outlier, "uint8"), (n_good, "int32"))
        ptrs, s = _device_ptrs("pose_optimization_batch_device", want, stream)
        _mchk(self.L.orbm_pose_optimization_batch_device(self.h, n_problems, *ptrs, s))

    @staticmethod
    def pack_sim3opt_problems(problems):
        """The CSR arrays of orbm_optimize_sim3_batch from a list of OptimizeSim3 argument tuples
        (x1c, x2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2, th2, fix_scale, S12) -> (off int32 [B+1], x1c float32 [N, 3], x2c,
        obs1 float32 [N, 2], obs2, inv_sigma2_1 float32 [N], inv_sigma2_2, cams float32 [B, 8], th2 float32 [B], fix_scale int32 [B],
        S12 float64 [B, 8])."""
        B = len(problems)
        off = np.zeros(B + 1, np.int32)
        cams, th2, fix, S = np.zeros((B, 8), np.float32), np.zeros(B, np.float32), np.zeros(B, np.int32), np.zeros((B, 8), np.float64)
        cols = [[] for _ in range(6)]
        widths = (3, 3, 2, 2, 1, 1)
        for p, args in enumerate(problems):
            arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, w) for a, w in zip(args[:6], widths)]
            if len(set(len(a) for a in arrs)) != 1:
                raise OrbxError(ORBX_E_INVALID, "problem %d: array lengths disagree: %s" % (p, [len(a) for a in arrs]))
            for c, a in zip(cols, arrs):
                c.append(a)
            off[p + 1] = off[p] + len(arrs[0])
            cams[p, :4], cams[p, 4:] = np.asarray(args[6], np.float32), np.asarray(args[7], np.float32)
            th2[p], fix[p] = args[8], 1 if args[9] else 0
            S[p] = np.asarray(args[10], np.float64).reshape(8)
        x1, x2, o1, o2, s1, s2 = (_cat(c, (0, w), np.float32) for c, w in zip(cols, widths))
        return off, x1, x2, o1, o2, s1.reshape(-1), s2.reshape(-1), cams, th2, fix, S

    def optimize_sim3_batch(self, problems):
        """Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) for a list of independent problems in one launch, each an argument
        tuple of OptimizeSim3().  Returns a list of OptimizeSim3()'s results: (S12 float64 [8], flags bool[n], nIn)."""
        off, x1, x2, o1, o2, s1, s2, cams, th2, fix, S = self.pack_sim3opt_problems(problems)
        B = len(problems)
        flags, n_in = np.zeros(max(int(off[-1]), 1), np.uint8), np.zeros(max(B, 1), np.int32)
        _mchk(self.L.orbm_optimize_sim3_batch(self.h, B, _p(off), _p(x1), _p(x2), _p(o1), _p(o2), _p(s1), _p(s2), _p(cams), _p(th2), _p(fix),
                                              _p(S), _p(flags), _p(n_in)))
        return [(S[p].copy(), flags[off[p]:off[p + 1]].astype(bool), int(n_in[p])) for p in range(B)]

    def optimize_sim3_batch_device(self, n_problems, off, x1c, x2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cams, th2, fix_scale, S12,
                                   flags, n_in, stream=None):
        """The same on torch tensors on the handle's device: off int32 [B+1], x1c / x2c float32 [N, 3], obs1 / obs2 float32 [N, 2],
        inv_sigma2_1 / inv_sigma2_2 float32 [N], cams float32 [B, 8], th2 float32 [B], fix_scale int32 [B], S12 float64 [B, 8]
        (in/out), flags uint8 [N], n_in int32 [B].  Nothing is copied or synchronised; stream: a torch stream, a raw hipStream_t or
        None (the handle's stream)."""
        f32 = "float32"
        want = ((off, "int32"), (x1c, f32), (x2c, f32), (obs1, f32), (obs2, f32), (inv_sigma2_1, f32), (inv_sigma2_2, f32), (cams, f32),
                (th2, f32), (fix_scale, "int32"), (S12, "float64"), (flags, "uint8"), (n_in, "int32"))
        ptrs, s = _device_ptrs("optimize_sim3_batch_device", want, stream, none_ok=n_problems == 0)
        _mchk(self.L.orbm_optimize_sim3_batch_device(self.h, n_problems, *ptrs, s))

    @staticmethod
    def pack_lba_problem(problem):
        """pack_lba_problem() of the module: the flat arrays of orbm_local_bundle_adjustment from a problem dict"""
        return pack_lba_problem(problem)

    def local_bundle_adjustment(self, problem, stop=None):
        """Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778) on the GPU: the problem, results and `stop` of
        LocalBundleAdjustment(), through orbm_local_bundle_adjustment."""
        rc, Tcw, xw, erase, stats = _lba_call(lambda *args: self.L.orbm_local_bundle_adjustment(self.h, *args), problem, stop)
        if rc < 0:
            _mchk(rc)
        return rc, Tcw, xw, erase, stats

    def bundle_adjustment(self, problem, n_iterations=5, robust=True, stop=None):
        """Optimizer::BundleAdjustment (src/Optimizer.cc:49-237) on the GPU: the problem, arguments and results of
        BundleAdjustment(), through orbm_bundle_adjustment (the reduced system goes to the many-workgroup solve of spd_solve)."""
        rc, Tcw, xw, stats = _ba_call(lambda *args: self.L.orbm_bundle_adjustment(self.h, *args), problem, n_iterations, robust, stop)
        if rc < 0:
            _mchk(rc)
        return rc, Tcw, xw, stats

    def optimize_essential_graph(self, problem, n_iterations=20):
        """Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044) on the GPU: the problem, argument and results of
        optimize_essential_graph(), through orbm_optimize_essential_graph (the 7N x 7N system goes to the solve of spd_solve)."""
        rc, Tcw, xw, Scw, stats = _eg_call(lambda *args: self.L.orbm_optimize_essential_graph(self.h, *args), problem, n_iterations)
        _mchk(rc)
        return rc, Tcw, xw, Scw, stats

    def spd_solve(self, A, b):
        """orbm_spd_solve_f64: A x = b for a symmetric positive definite float64 [n, n] A (its lower triangle is read) by the
        blocked Cholesky of csrc/orbm_spd.hip -> (x float64 [n], ok bool).  ok False (a pivot not positive or not finite): x is
        zeros."""
        A = np.ascontiguousarray(A, np.float64)
        b = np.ascontiguousarray(b, np.float64).reshape(-1)
        if A.ndim != 2 or A.shape[0] != A.shape[1] or len(b) != A.shape[0]:
            raise OrbxError(ORBX_E_INVALID, "spd_solve: A must be [n, n] and b [n]")
        x = np.full(max(len(b), 1), np.nan)
        ok = C.c_int(-1)
        _mchk(self.L.orbm_spd_solve_f64(self.h, _p(A), _p(b), len(b), _p(x), C.byref(ok)))
        return x[:len(b)], bool(ok.value)

    @staticmethod
    def pack_sim3_problems(problems):
        """The arrays of orbm_sim3_hypotheses from a list of problems, each a Sim3Solver (its queued triples) or a tuple
        (x3dc1 [n, 3], x3dc2 [n, 3], max_err1 [n], max_err2 [n], K1 (4), K2 (4), fix_scale, triples [h, 3]) ->
        (off int32 [B+1], x3dc1 float32 [N, 3], x3dc2, max_err1 float32 [N], max_err2, cams SIM3_CAM_DTYPE [B], hyp_off int32 [B+1],
        triples int32 [H, 3], mask_off int64 [B+1])."""
        cams = np.zeros(len(problems), SIM3_CAM_DTYPE)
        x1s, x2s, e1s, e2s, tris = [], [], [], [], []
        for p, pr in enumerate(problems):
            if isinstance(pr, Sim3Solver):
                pr = pr.problem()
            x1, x2, e1, e2, K1, K2, fix, tri = pr
            x1 = np.ascontiguousarray(x1, np.float32).reshape(-1, 3)
            x2 = np.ascontiguousarray(x2, np.float32).reshape(-1, 3)
            e1 = np.ascontiguousarray(e1, np.float32).reshape(-1)
            e2 = np.ascontiguousarray(e2, np.float32).reshape(-1)
            tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
            if not (len(x1) == len(x2) == len(e1) == len(e2)):
                raise OrbxError(ORBX_E_INVALID, "problem %d: array lengths disagree: %d / %d / %d / %d" % (p, len(x1), len(x2), len(e1), len(e2)))
            x1s.append(x1); x2s.append(x2); e1s.append(e1); e2s.append(e2); tris.append(tri)
            cams[p] = (np.asarray(K1, np.float32).reshape(4), np.asarray(K2, np.float32).reshape(4), int(bool(fix)))
        off, hyp_off, mask_off = _hyp_offsets([(len(x1), len(tri)) for x1, tri in zip(x1s, tris)])
        return (off, _cat(x1s, (0, 3), np.float32), _cat(x2s, (0, 3), np.float32), _cat(e1s, (0,), np.float32), _cat(e2s, (0,), np.float32),
                cams, hyp_off, _cat(tris, (0, 3), np.int32), mask_off)

    def sim3_hypotheses(self, problems):
        """Every hypothesis of every problem in one launch (orbm_sim3_hypotheses; problems as in pack_sim3_problems).  Returns a list
        of (n_inliers int32 [h], sRt float32 [h, 13], masks uint32 [h, ceil(n / 32)]) per problem: what Sim3Solver.attach_results takes."""
        off, x1, x2, e1, e2, cams, hyp_off, tri, mask_off = self.pack_sim3_problems(problems)
        B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
        cnt, sRt, masks = np.zeros(max(H, 1), np.int32), np.zeros((max(H, 1), 13), np.float32), np.zeros(max(MW, 1), np.uint32)
        _mchk(self.L.orbm_sim3_hypotheses(self.h, B, _p(off), _p(x1), _p(x2), _p(e1), _p(e2), _p(cams), _p(hyp_off), _p(tri), _p(mask_off),
                                          _p(cnt), _p(sRt), _p(masks)))
        return _split_hypotheses(off, hyp_off, mask_off, cnt, sRt, masks)

    def sim3_hypotheses_device(self, n_problems, total_hypotheses, off, x3dc1, x3dc2, max_err1, max_err2, cams, hyp_off, triples, mask_off,
                               n_inliers, sRt, masks, stream=None):
        """The same on torch tensors on the handle's device: off int32 [B+1], x3dc1 / x3dc2 float32 [N, 3], max_err1 / max_err2
        float32 [N], cams uint8 [B, 36] (SIM3_CAM_DTYPE bytes), hyp_off int32 [B+1], triples int32 [H, 3], mask_off int64 [B+1],
        n_inliers int32 [H], sRt float32 [H, 13], masks int32 [mask words].  Nothing is copied or synchronised; stream: a torch
        stream, a raw hipStream_t or None (the handle's stream)."""
        want = ((off, "int32"), (x3dc1, "float32"), (x3dc2, "float32"), (max_err1, "float32"), (max_err2, "float32"), (cams, "uint8"),
                (hyp_off, "int32"), (triples, "int32"), (mask_off, "int64"), (n_inliers, "int32"), (sRt, "float32"), (masks, "int32"))
        ptrs, s = _device_ptrs("sim3_hypotheses_device", want, stream)
        _mchk(self.L.orbm_sim3_hypotheses_device(self.h, n_problems, total_hypotheses, *ptrs, s))

    @staticmethod
    def pack_init_problems(problems):
        """The arrays of orbm_init_hypotheses from a list of problems, each an Initializer (its drawn sets: the H of every set, then
        the F) or a tuple (uv [n, 4], pn [n, 4], T1 (9), T2 (9), sigma, sets [h, 8], models [h]) ->
        (off int32 [B+1], uv float32 [N, 4], pn float32 [N, 4], params INIT_PARAMS_DTYPE [B], hyp_off int32 [B+1], sets int32 [H, 8],
        models int32 [H], mask_off int64 [B+1])."""
        params = np.zeros(len(problems), INIT_PARAMS_DTYPE)
        uvs, pns, setss, modelss = [], [], [], []
        for p, pr in enumerate(problems):
            if isinstance(pr, Initializer):
                pr = pr.problem()
            uv, pn, T1, T2, sigma, sets, models = pr
            uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 4)
            pn = np.ascontiguousarray(pn, np.float32).reshape(-1, 4)
            sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
            models = np.ascontiguousarray(models, np.int32).reshape(-1)
            if len(uv) != len(pn) or len(sets) != len(models):
                raise OrbxError(ORBX_E_INVALID, "problem %d: array lengths disagree: %d / %d matches, %d / %d hypotheses"
                                % (p, len(uv), len(pn), len(sets), len(models)))
            uvs.append(uv); pns.append(pn); setss.append(sets); modelss.append(models)
            params[p] = (np.asarray(T1, np.float32).reshape(9), np.asarray(T2, np.float32).reshape(9), np.float32(sigma))
        off, hyp_off, mask_off = _hyp_offsets([(len(uv), len(sets)) for uv, sets in zip(uvs, setss)])
        return (off, _cat(uvs, (0, 4), np.float32), _cat(pns, (0, 4), np.float32), params, hyp_off, _cat(setss, (0, 8), np.int32),
                _cat(modelss, (0,), np.int32), mask_off)

    def init_hypotheses(self, problems):
        """Every H / F hypothesis of every problem in one launch (orbm_init_hypotheses; problems as in pack_init_problems).  Returns a
        list of (score_M float32 [h, 10], n_inliers int32 [h], masks uint32 [h, ceil(n / 32)]) per problem: what
        Initializer.attach_results takes."""
        off, uv, pn, params, hyp_off, sets, models, mask_off = self.pack_init_problems(problems)
        B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
        sm, cnt, masks = np.zeros((max(H, 1), 10), np.float32), np.zeros(max(H, 1), np.int32), np.zeros(max(MW, 1), np.uint32)
        _mchk(self.L.orbm_init_hypotheses(self.h, B, _p(off), _p(uv), _p(pn), _p(params), _p(hyp_off), _p(sets), _p(models), _p(mask_off),
                                          _p(sm), _p(cnt), _p(masks)))
        return _split_hypotheses(off, hyp_off, mask_off, sm, cnt, masks)

    def init_hypotheses_device(self, n_problems, total_hypotheses, off, uv, pn, params, hyp_off, sets, models, mask_off, score_M, n_inliers,
                               masks, stream=None):
        """The same on torch tensors on the handle's device: off int32 [B+1], uv / pn float32 [N, 4], params uint8 [B, 76]
        (INIT_PARAMS_DTYPE bytes), hyp_off int32 [B+1], sets int32 [H, 8], models int32 [H], mask_off int64 [B+1], score_M float32
        [H, 10], n_inliers int32 [H], masks int32 [mask words].  Nothing is copied or synchronised; stream: a torch stream, a raw
        hipStream_t or None (the handle's stream)."""
        want = ((off, "int32"), (uv, "float32"), (pn, "float32"), (params, "uint8"), (hyp_off, "int32"), (sets, "int32"), (models, "int32"),
                (mask_off, "int64"), (score_M, "float32"), (n_inliers, "int32"), (masks, "int32"))
        ptrs, s = _device_ptrs("init_hypotheses_device", want, stream)
        _mchk(self.L.orbm_init_hypotheses_device(self.h, n_problems, total_hypotheses, *ptrs, s))

    def init_check_rt(self, uv, inliers, K, th2, Rt):
        """CheckRT's per-match part for every motion of Rt [k, 12] in one launch (orbm_init_check_rt) ->
        (status uint8 [k, n], cos_parallax float32 [k, n], p3d float32 [k, n, 3])."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 4)
        inl = np.ascontiguousarray(inliers, np.uint8).reshape(-1)
        K = np.ascontiguousarray(K, np.float32).reshape(4)
        Rt = np.ascontiguousarray(Rt, np.float32).reshape(-1, 12)
        n, k = len(uv), len(Rt)
        if len(inl) != n:
            raise OrbxError(ORBX_E_INVALID, "init_check_rt: %d matches, %d flags" % (n, len(inl)))
        status, cosp, p3d = np.zeros((k, n), np.uint8), np.zeros((k, n), np.float32), np.zeros((k, n, 3), np.float32)
        _mchk(self.L.orbm_init_check_rt(self.h, n, _p(uv), _p(inl), _p(K), float(th2), k, _p(Rt), _p(status), _p(cosp), _p(p3d)))
        return status, cosp, p3d

    def init_check_rt_device(self, n, uv, inliers, K, th2, n_motions, Rt, status, cos_parallax, p3d, stream=None):
        """The same on torch tensors on the handle's device: uv float32 [n, 4], inliers uint8 [n], Rt float32 [k, 12], status uint8
        [k, n], cos_parallax float32 [k, n], p3d float32 [k, n, 3]; K = (fx, fy, cx, cy) and th2 are host values."""
        want = ((uv, "float32"), (inliers, "uint8"), (Rt, "float32"), (status, "uint8"), (cos_parallax, "float32"), (p3d, "float32"))
        (uv, inliers, Rt, status, cos_parallax, p3d), s = _device_ptrs("init_check_rt_device", want, stream)
        K = np.ascontiguousarray(K, np.float32).reshape(4)
        _mchk(self.L.orbm_init_check_rt_device(self.h, n, uv, inliers, _p(K), float(th2), n_motions, Rt, status, cos_parallax, p3d, s))

    @staticmethod
    def pack_pnp_problems(problems):
        """The arrays of orbm_pnp_hypotheses from a list of problems, each a PnPsolver (its queued samples) or a tuple
        (p2d [n, 2], p3d [n, 3], max_err [n], K (fx, fy, cx, cy), set_size, samples [h, set_size]) ->
        (off int32 [B+1], p2d float32 [N, 2], p3d float32 [N, 3], max_err float32 [N], cams PNP_CAM_DTYPE [B], hyp_off int32 [B+1],
        samples int32 [H, 8] (padded with -1), mask_off int64 [B+1])."""
        cams = np.zeros(len(problems), PNP_CAM_DTYPE)
        p2s, p3s, es, sms = [], [], [], []
        for p, pr in enumerate(problems):
            if isinstance(pr, PnPsolver):
                pr = pr.problem()
            p2d, p3d, e, K, set_size, sm = pr
            p2d = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
            p3d = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
            e = np.ascontiguousarray(e, np.float32).reshape(-1)
            set_size = int(set_size)
            sm = np.ascontiguousarray(sm, np.int32).reshape(-1, set_size) if set_size > 0 else np.zeros((0, 0), np.int32)
            if not (len(p2d) == len(p3d) == len(e)):
                raise OrbxError(ORBX_E_INVALID, "problem %d: array lengths disagree: %d / %d / %d" % (p, len(p2d), len(p3d), len(e)))
            padded = np.full((len(sm), ORBM_PNP_MAX_SET), -1, np.int32)
            k = min(set_size, ORBM_PNP_MAX_SET)      # a larger set is refused by the call (cams carries its true size)
            padded[:, :k] = sm[:, :k]
            p2s.append(p2d); p3s.append(p3d); es.append(e); sms.append(padded)
            K = np.asarray(K, np.float32).reshape(4)
            cams[p] = (K[0], K[1], K[2], K[3], set_size)
        off, hyp_off, mask_off = _hyp_offsets([(len(p2d), len(sm)) for p2d, sm in zip(p2s, sms)])
        return (off, _cat(p2s, (0, 2), np.float32), _cat(p3s, (0, 3), np.float32), _cat(es, (0,), np.float32), cams, hyp_off,
                _cat(sms, (0, ORBM_PNP_MAX_SET), np.int32), mask_off)

    def pnp_hypotheses(self, problems):
        """Every EPnP hypothesis of every problem in one launch (orbm_pnp_hypotheses; problems as in pack_pnp_problems).  Returns a
        list of (n_inliers int32 [h], Rt float64 [h, 12], masks uint32 [h, ceil(n / 32)]) per problem: what
        PnPsolver.attach_results takes."""
        off, p2d, p3d, e, cams, hyp_off, sm, mask_off = self.pack_pnp_problems(problems)
        B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
        cnt, Rt, masks = np.zeros(max(H, 1), np.int32), np.zeros((max(H, 1), 12), np.float64), np.zeros(max(MW, 1), np.uint32)
        _mchk(self.L.orbm_pnp_hypotheses(self.h, B, _p(off), _p(p2d), _p(p3d), _p(e), _p(cams), _p(hyp_off), _p(sm), _p(mask_off),
                                         _p(cnt), _p(Rt), _p(masks)))
        return _split_hypotheses(off, hyp_off, mask_off, cnt, Rt, masks)

    def pnp_hypotheses_device(self, n_problems, total_hypotheses, off, p2d, p3d, max_err, cams, hyp_off, samples, mask_off, n_inliers, Rt,
                              masks, stream=None):
        """The same on torch tensors on the handle's device: off int32 [B+1], p2d float32 [N, 2], p3d float32 [N, 3], max_err float32
        [N], cams uint8 [B, 20] (PNP_CAM_DTYPE bytes), hyp_off int32 [B+1], samples int32 [H, 8], mask_off int64 [B+1], n_inliers
        int32 [H], Rt float64 [H, 12], masks int32 [mask words].  Nothing is copied or synchronised; stream: a torch stream, a raw
        hipStream_t or None (the handle's stream)."""
        want = ((off, "int32"), (p2d, "float32"), (p3d, "float32"), (max_err, "float32"), (cams, "uint8"), (hyp_off, "int32"),
                (samples, "int32"), (mask_off, "int64"), (n_inliers, "int32"), (Rt, "float64"), (masks, "int32"))
        ptrs, s = _device_ptrs("pnp_hypotheses_device", want, stream)
        _mchk(self.L.orbm_pnp_hypotheses_device(self.h, n_problems, total_hypotheses, *ptrs, s))

    def search_local_points(self, view, skip, xw, normal, mf_max, mf_min, mp_desc, mp_obs, kps_cur, desc_cur, cur_obs, th,
                            u_right=None, viewing_cos_limit=0.5):
        """Tracking::SearchLocalPoints (src/Tracking.cc:1174-1199) in one call: frustum() followed by SearchByProjectionMap() on the
        points in view, the projection staying on the device in between.  The frame's grid must be in the handle (grid_build);
        cur_obs (int32) is updated in place.  Returns frustum()'s tuple + (cur_match, nmatches)."""
        a, out, n = self._frustum_inputs(view, skip, xw, normal, mf_max, mf_min)
        mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32); mp_obs = np.ascontiguousarray(mp_obs, np.int32).reshape(-1)
        kps_cur = np.ascontiguousarray(kps_cur, KP_DTYPE); desc_cur = np.ascontiguousarray(desc_cur, np.uint8).reshape(-1, 32)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        if len(mp_desc) != n or len(mp_obs) != n or len(desc_cur) != len(kps_cur) or (ur is not None and len(ur) != len(kps_cur)):
            raise OrbxError(ORBX_E_INVALID, "array lengths disagree: %d MapPoints, %d key points" % (n, len(kps_cur)))
        assert cur_obs.dtype == np.int32 and cur_obs.flags["C_CONTIGUOUS"] and len(cur_obs) == len(kps_cur)
        cm = np.full(len(kps_cur), -1, np.int32)
        nt, nm = C.c_int(0), C.c_int(0)
        _mchk(self.L.orbm_search_local_points(self.h, _p(a[0]), n, _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), _p(a[5]), C.c_float(viewing_cos_limit),
                                              _p(mp_desc), _p(mp_obs), _p(kps_cur), _p(desc_cur), _p(ur), len(kps_cur), C.c_float(th),
                                              C.c_float(self.mfNNratio), *[_p(o) for o in out], C.byref(nt), _p(cur_obs), _p(cm), C.byref(nm)))
        return out + (nt.value, cm, nm.value)

    def match_dense(self, q, kq, t, kt, th=None):
        """Dense SearchByBoW-style acceptance + rotation filter on host buffers (via best2)."""
        bi, bd, sd = self.best2(q, t)
        th = self.TH_LOW if th is None else th
        m = np.where((bd <= th) & (bd.astype(np.float32) < np.float32(self.mfNNratio) * sd.astype(np.float32)), bi, -1).astype(np.int32)
        if self.mbCheckOrientation:
            aq = np.ascontiguousarray(kq["angle"], np.float32)
            at = np.ascontiguousarray(kt["angle"], np.float32)
            n = self.L.orbm_rot_filter(_p(aq), _p(at), _p(m), len(m))
            if n < 0:
                _mchk(n)
        else:
            n = int((m >= 0).sum())
        return n, m

    def match_batch_device(self, d_q, d_kq, d_nq, d_t, d_kt, d_nt, cap, nbatch, d_match12, d_nmatches,
                           th=None, stream=None):
        th = self.TH_LOW if th is None else th
        _mchk(self.L.orbm_match_batch_device(self.h, d_q, d_kq, d_nq, d_t, d_kt, d_nt, cap, nbatch, th,
                                             self.mfNNratio, int(self.mbCheckOrientation), d_match12, d_nmatches, stream))

    def best2_batch_device(self, d_q, d_nq, d_t, d_nt, cap, nbatch, d_best_idx, d_best_d, d_second_d, stream=None):
        """best2 for nbatch device-resident pairs ([nbatch, cap, 32] descriptors, int32 counts per pair) into three int32
        [nbatch, cap] arrays; -1 / 256 / 256 beyond a pair's query count.  Raw device pointers; nothing is synchronised."""
        _mchk(self.L.orbm_best2_batch_device(self.h, d_q, d_nq, d_t, d_nt, cap, nbatch, d_best_idx, d_best_d, d_second_d, stream))

    # ---- N1: Frame grid (src/Frame.cc:230-245, 327-392) ----
    def grid_build(self, kps_un, min_x, max_x, min_y, max_y):
        """Frame::AssignFeaturesToGrid for mvKeysUn with the image bounds mnMinX..mnMaxY."""
        kps_un = np.ascontiguousarray(kps_un, KP_DTYPE)
        self._grid_n = len(kps_un)
        _mchk(self.L.orbm_grid_build(self.h, _p(kps_un), len(kps_un), min_x, max_x, min_y, max_y))

    def grid_count(self):
        """Keypoints in the handle's grid (frame or key frame), -1 when it holds none."""
        return self.L.orbm_grid_count(self.h)

    @staticmethod
    def _windows(x, y, r, min_level, max_level):
        x = np.ascontiguousarray(x, np.float32); y = np.ascontiguousarray(y, np.float32)
        r = np.broadcast_to(np.asarray(r, np.float32), x.shape).copy()
        mn = np.broadcast_to(np.asarray(min_level, np.int32), x.shape).copy()
        mx = np.broadcast_to(np.asarray(max_level, np.int32), x.shape).copy()
        return x, y, r, mn, mx

    def GetFeaturesInArea(self, x, y, r, minLevel=-1, maxLevel=-1, cap=None):
        """Frame::GetFeaturesInArea for arrays of windows -> (cand_off[nq+1], cand_idx) in reference order."""
        x, y, r, mn, mx = self._windows(x, y, r, minLevel, maxLevel)
        nq = len(x)
        cap = cap or max(1, nq * max(getattr(self, "_grid_n", 0), 1))
        cap = min(cap, 1 << 22)
        off = np.zeros(nq + 1, np.int32); idx = np.zeros(cap, np.int32)
        n = self.L.orbm_features_in_area(self.h, _p(x), _p(y), _p(r), _p(mn), _p(mx), nq, _p(off), _p(idx), cap)
        if n < 0:
            _mchk(n)
        return off, idx[:n].copy()

    def search_area_best2(self, qdesc, x, y, r, minLevel, maxLevel, train_desc, skip=None):
        qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        train_desc = np.ascontiguousarray(train_desc, np.uint8).reshape(-1, 32)
        x, y, r, mn, mx = self._windows(x, y, r, minLevel, maxLevel)
        nq = len(x)
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.uint8)
        bi, bd, sd = np.full(nq, -1, np.int32), np.full(nq, 256, np.int32), np.full(nq, 256, np.int32)
        _mchk(self.L.orbm_search_area_best2(self.h, _p(qdesc), _p(x), _p(y), _p(r), _p(mn), _p(mx), nq, _p(train_desc), _p(skip),
                                            _p(bi), _p(bd), _p(sd)))
        return bi, bd, sd

    def SearchByProjectionLast(self, has_point, xw, mp_desc, mp_obs, kps_last, Tcw, Tlw, K, mb, mbf, bounds, scale_factors,
                               kps_cur, desc_cur, cur_obs, th, mono, u_right=None):
        """ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (src/ORBmatcher.cc:1328-1470);
        arguments as in include/orbm.h.  cur_obs (int32, in/out).  Returns (cur_match, nmatches)."""
        has_point = np.ascontiguousarray(has_point, np.uint8); xw = np.ascontiguousarray(xw, np.float32).reshape(-1, 3)
        mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32); mp_obs = np.ascontiguousarray(mp_obs, np.int32)
        kps_last = np.ascontiguousarray(kps_last); kps_cur = np.ascontiguousarray(kps_cur)
        desc_cur = np.ascontiguousarray(desc_cur, np.uint8).reshape(-1, 32)
        Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(16); Tlw = np.ascontiguousarray(Tlw, np.float32).reshape(16)
        b = np.ascontiguousarray(bounds, np.float32); sf = np.ascontiguousarray(scale_factors, np.float32)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        assert cur_obs.dtype == np.int32 and cur_obs.flags["C_CONTIGUOUS"] and len(cur_obs) == len(kps_cur)
        cm = np.full(len(kps_cur), -1, np.int32)
        nm = C.c_int(0)
        fx, fy, cx, cy = K
        _mchk(self.L.orbm_search_by_projection_last(self.h, len(kps_last), _p(has_point), _p(xw), _p(mp_desc), _p(mp_obs), _p(kps_last), _p(Tcw), _p(Tlw),
                                                    fx, fy, cx, cy, mb, mbf, _p(b), _p(sf), len(sf), _p(kps_cur), _p(desc_cur), _p(ur), len(kps_cur),
                                                    th, int(mono), 1 if self.mbCheckOrientation else 0, _p(cur_obs), _p(cm), C.byref(nm)))
        return cm, nm.value

    def SearchByProjectionMap(self, in_view, proj_x, proj_y, pred_level, view_cos, mp_desc, mp_obs, scale_factors, kps_cur, desc_cur,
                              cur_obs, th, proj_xr=None, u_right=None):
        """ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th) (src/ORBmatcher.cc:45-125);
        arguments as in include/orbm.h.  Returns (cur_match, nmatches); cur_obs (int32) is updated in place."""
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        in_view = np.ascontiguousarray(in_view, np.uint8); px, py, pxr, vc = f32(proj_x), f32(proj_y), f32(proj_xr), f32(view_cos)
        lv = np.ascontiguousarray(pred_level, np.int32); mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        mp_obs = np.ascontiguousarray(mp_obs, np.int32); sf = f32(scale_factors); ur = f32(u_right)
        kps_cur = np.ascontiguousarray(kps_cur); desc_cur = np.ascontiguousarray(desc_cur, np.uint8).reshape(-1, 32)
        assert cur_obs.dtype == np.int32 and cur_obs.flags["C_CONTIGUOUS"] and len(cur_obs) == len(kps_cur)
        cm = np.full(len(kps_cur), -1, np.int32)
        nm = C.c_int(0)
        _mchk(self.L.orbm_search_by_projection_map(self.h, len(in_view), _p(in_view), _p(px), _p(py), _p(pxr), _p(lv), _p(vc), _p(mp_desc), _p(mp_obs),
                                                   _p(sf), len(sf), _p(kps_cur), _p(desc_cur), _p(ur), len(kps_cur), th, C.c_float(self.mfNNratio),
                                                   _p(cur_obs), _p(cm), C.byref(nm)))
        return cm, nm.value

    @staticmethod
    def ProjectPoints(Tcw, K, bounds, xw):
        """orbm_project_points: (u, v, invzc, dist3D, in_image) of world points under the pose Tcw (src/ORBmatcher.cc:1498-1514)."""
        L = lib()
        Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(16); b = np.ascontiguousarray(bounds, np.float32)
        xw = np.ascontiguousarray(xw, np.float32).reshape(-1, 3)
        n = len(xw)
        u, v, iz, d3 = (np.zeros(n, np.float32) for _ in range(4))
        inside = np.zeros(n, np.uint8)
        fx, fy, cx, cy = K
        _mchk(L.orbm_project_points(_p(Tcw), fx, fy, cx, cy, _p(b), _p(xw), n, _p(u), _p(v), _p(iz), _p(d3), _p(inside)))
        return u, v, iz, d3, inside

    @staticmethod
    def PredictScale(mf_max_distance, dist, log_scale_factor, n_levels):
        L = lib()
        return np.array([L.orbm_predict_scale(float(a), float(b), float(log_scale_factor), int(n_levels))
                         for a, b in zip(np.asarray(mf_max_distance, np.float32), np.asarray(dist, np.float32))], np.int32)

    def SearchByProjectionKF(self, use, proj_u, proj_v, pred_level, mp_desc, kf_angle, scale_factors, kps_cur, desc_cur, cur_has_point, th, orb_dist):
        """ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1472-1599)
        after the projection step; arguments as in include/orbm.h.  cur_has_point (uint8, in/out).  Returns (cur_match, nmatches)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        use = np.ascontiguousarray(use, np.uint8); pu, pv, ka, sf = f32(proj_u), f32(proj_v), f32(kf_angle), f32(scale_factors)
        lv = np.ascontiguousarray(pred_level, np.int32); mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        kps_cur = np.ascontiguousarray(kps_cur); desc_cur = np.ascontiguousarray(desc_cur, np.uint8).reshape(-1, 32)
        assert cur_has_point.dtype == np.uint8 and cur_has_point.flags["C_CONTIGUOUS"] and len(cur_has_point) == len(kps_cur)
        cm = np.full(len(kps_cur), -1, np.int32)
        nm = C.c_int(0)
        _mchk(self.L.orbm_search_by_projection_kf(self.h, len(use), _p(use), _p(pu), _p(pv), _p(lv), _p(mp_desc), _p(ka), _p(sf), len(sf),
                                                  _p(kps_cur), _p(desc_cur), len(kps_cur), th, int(orb_dist), 1 if self.mbCheckOrientation else 0,
                                                  _p(cur_has_point), _p(cm), C.byref(nm)))
        return cm, nm.value

    # ---- the LocalMapping / LoopClosing matchers (include/orbm.h; src/ORBmatcher.cc:290-403, 522-655, 657-823, 825-975, 977-1100, 1102-1326) ----
    def reserve(self, max_queries=0, max_train=0, max_pairs=0):
        _mchk(self.L.orbm_reserve(self.h, int(max_queries), int(max_train), int(max_pairs)))

    def grid_build_kf(self, kps_un, grid):
        """KeyFrame grid: grid = (assign_min_x, assign_min_y, inv_w, inv_h, query_min_x, query_min_y)."""
        kps_un = np.ascontiguousarray(kps_un)
        _mchk(self.L.orbm_grid_build_kf(self.h, _p(kps_un), len(kps_un), *[float(v) for v in grid]))

    @staticmethod
    def Sim3Decompose(Scw):
        Scw = np.ascontiguousarray(Scw, np.float32).reshape(16)
        T, Ow = np.zeros(16, np.float32), np.zeros(3, np.float32)
        _mchk(lib().orbm_sim3_decompose(_p(Scw), _p(T), _p(Ow)))
        return T.reshape(4, 4), Ow

    @staticmethod
    def Sim3Relative(s12, R12, t12):
        R12 = np.ascontiguousarray(R12, np.float32).reshape(9); t12 = np.ascontiguousarray(t12, np.float32).reshape(3)
        sR12, sR21, t21 = np.zeros(9, np.float32), np.zeros(9, np.float32), np.zeros(3, np.float32)
        _mchk(lib().orbm_sim3_relative(C.c_float(s12), _p(R12), _p(t12), _p(sR12), _p(sR21), _p(t21)))
        return sR12.reshape(3, 3), sR21.reshape(3, 3), t21

    @staticmethod
    def ProjectPointsKF(Tcw, K, bounds, xw, normal=None, Ow=None):
        """orbm_project_points_kf: (u, v, invz, dist3D, ok)."""
        Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(16); b = np.ascontiguousarray(bounds, np.float32)
        xw = np.ascontiguousarray(xw, np.float32).reshape(-1, 3)
        if normal is not None:
            normal = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        if Ow is not None:
            Ow = np.ascontiguousarray(Ow, np.float32).reshape(3)
        n = len(xw)
        u, v, iz, d3 = (np.zeros(n, np.float32) for _ in range(4))
        ok = np.zeros(n, np.uint8)
        fx, fy, cx, cy = K
        _mchk(lib().orbm_project_points_kf(_p(Tcw), _p(Ow), fx, fy, cx, cy, _p(b), _p(xw), _p(normal), n, _p(u), _p(v), _p(iz), _p(d3), _p(ok)))
        return u, v, iz, d3, ok

    @staticmethod
    def ProjectPointsSim3(TAw, sR, t, K, boundsB, xw):
        TAw = np.ascontiguousarray(TAw, np.float32).reshape(16); sR = np.ascontiguousarray(sR, np.float32).reshape(9)
        t = np.ascontiguousarray(t, np.float32).reshape(3); b = np.ascontiguousarray(boundsB, np.float32)
        xw = np.ascontiguousarray(xw, np.float32).reshape(-1, 3)
        n = len(xw)
        u, v, d3 = (np.zeros(n, np.float32) for _ in range(3))
        ok = np.zeros(n, np.uint8)
        fx, fy, cx, cy = K
        _mchk(lib().orbm_project_points_sim3(_p(TAw), _p(sR), _p(t), fx, fy, cx, cy, _p(b), _p(xw), n, _p(u), _p(v), _p(d3), _p(ok)))
        return u, v, d3, ok

    def SearchByProjectionSim3(self, use, proj_u, proj_v, pred_level, mp_desc, scale_factors, kps_kf, desc_kf, kf_matched, th):
        """SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) after the projection step.  kf_matched uint8 in/out.
        Returns (kf_match, nmatches)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        use = np.ascontiguousarray(use, np.uint8); pu, pv, sf = f32(proj_u), f32(proj_v), f32(scale_factors)
        lv = np.ascontiguousarray(pred_level, np.int32); mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        kps_kf = np.ascontiguousarray(kps_kf); desc_kf = np.ascontiguousarray(desc_kf, np.uint8).reshape(-1, 32)
        assert kf_matched.dtype == np.uint8 and kf_matched.flags["C_CONTIGUOUS"] and len(kf_matched) == len(kps_kf)
        km = np.full(len(kps_kf), -1, np.int32)
        nm = C.c_int(0)
        _mchk(self.L.orbm_search_by_projection_sim3(self.h, len(use), _p(use), _p(pu), _p(pv), _p(lv), _p(mp_desc), _p(sf), len(sf), _p(kps_kf),
                                                    _p(desc_kf), len(kps_kf), int(th), _p(kf_matched), _p(km), C.byref(nm)))
        return km, nm.value

    def SearchByBoWKF(self, kps1, desc1, featvec1, valid1, kps2, desc2, featvec2, valid2):
        """SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12): returns (matches12, nmatches)."""
        desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        kps1 = np.ascontiguousarray(kps1); kps2 = np.ascontiguousarray(kps2)
        n1, o1, i1 = [np.ascontiguousarray(a, np.int32) for a in featvec1]
        n2, o2, i2 = [np.ascontiguousarray(a, np.int32) for a in featvec2]
        valid1 = np.ascontiguousarray(valid1, np.uint8); valid2 = np.ascontiguousarray(valid2, np.uint8)
        m12 = np.full(len(desc1), -1, np.int32)
        nm = C.c_int(0)
        _mchk(self.L.orbm_search_by_bow_kf(self.h, _p(desc1), _p(kps1), len(desc1), _p(valid1), _p(n1), _p(o1), _p(i1), len(n1),
                                           _p(desc2), _p(kps2), len(desc2), _p(valid2), _p(n2), _p(o2), _p(i2), len(n2),
                                           C.c_float(self.mfNNratio), 1 if self.mbCheckOrientation else 0, _p(m12), C.byref(nm)))
        return m12, nm.value

    def SearchForTriangulation(self, kps1, desc1, has_mp1, u_right1, featvec1, kps2, desc2, has_mp2, u_right2, featvec2,
                               Cw, T2w, K2, F12, scale_factors2, level_sigma2_2, only_stereo=False):
        """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo): returns (matches12, nmatches)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        kps1 = np.ascontiguousarray(kps1); kps2 = np.ascontiguousarray(kps2)
        n1, o1, i1 = [np.ascontiguousarray(a, np.int32) for a in featvec1]
        n2, o2, i2 = [np.ascontiguousarray(a, np.int32) for a in featvec2]
        h1 = np.ascontiguousarray(has_mp1, np.uint8); h2 = np.ascontiguousarray(has_mp2, np.uint8)
        ur1, ur2, Cw, T2w, F12, sf2, ls2 = f32(u_right1), f32(u_right2), f32(Cw).reshape(3), f32(T2w).reshape(16), f32(F12).reshape(9), f32(scale_factors2), f32(level_sigma2_2)
        m12 = np.full(len(desc1), -1, np.int32)
        nm = C.c_int(0)
        fx, fy, cx, cy = K2
        _mchk(self.L.orbm_search_for_triangulation(self.h, _p(kps1), _p(desc1), len(desc1), _p(h1), _p(ur1), _p(n1), _p(o1), _p(i1), len(n1),
                                                   _p(kps2), _p(desc2), len(desc2), _p(h2), _p(ur2), _p(n2), _p(o2), _p(i2), len(n2),
                                                   _p(Cw), _p(T2w), fx, fy, cx, cy, _p(F12), _p(sf2), _p(ls2), len(sf2), 1 if only_stereo else 0,
                                                   1 if self.mbCheckOrientation else 0, _p(m12), C.byref(nm)))
        return m12, nm.value

    def Fuse(self, use, proj_u, proj_v, proj_ur, pred_level, mp_desc, scale_factors, inv_level_sigma2, kps_kf, u_right_kf, desc_kf, th=3.0):
        """Fuse(KeyFrame*, vpMapPoints, th), the search half: returns (best_idx, nfused)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        use = np.ascontiguousarray(use, np.uint8); pu, pv, pr, sf, inv, urk = f32(proj_u), f32(proj_v), f32(proj_ur), f32(scale_factors), f32(inv_level_sigma2), f32(u_right_kf)
        lv = np.ascontiguousarray(pred_level, np.int32); mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        kps_kf = np.ascontiguousarray(kps_kf); desc_kf = np.ascontiguousarray(desc_kf, np.uint8).reshape(-1, 32)
        bi = np.full(len(use), -1, np.int32)
        nf = C.c_int(0)
        _mchk(self.L.orbm_fuse(self.h, len(use), _p(use), _p(pu), _p(pv), _p(pr), _p(lv), _p(mp_desc), _p(sf), _p(inv), len(sf), _p(kps_kf), _p(urk),
                               _p(desc_kf), len(kps_kf), C.c_float(th), _p(bi), C.byref(nf)))
        return bi, nf.value

    def FuseSim3(self, use, proj_u, proj_v, pred_level, mp_desc, scale_factors, kps_kf, desc_kf, th):
        """Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint), the search half: returns (best_idx, nfused)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        use = np.ascontiguousarray(use, np.uint8); pu, pv, sf = f32(proj_u), f32(proj_v), f32(scale_factors)
        lv = np.ascontiguousarray(pred_level, np.int32); mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        kps_kf = np.ascontiguousarray(kps_kf); desc_kf = np.ascontiguousarray(desc_kf, np.uint8).reshape(-1, 32)
        bi = np.full(len(use), -1, np.int32)
        nf = C.c_int(0)
        _mchk(self.L.orbm_fuse_sim3(self.h, len(use), _p(use), _p(pu), _p(pv), _p(lv), _p(mp_desc), _p(sf), len(sf), _p(kps_kf), _p(desc_kf), len(kps_kf),
                                    C.c_float(th), _p(bi), C.byref(nf)))
        return bi, nf.value

    def SearchBySim3(self, use1, u1, v1, lv1, mp_desc1, use2, u2, v2, lv2, mp_desc2, kps1, desc1, grid1, sf1, kps2, desc2, grid2, sf2, th):
        """SearchBySim3, the two searches and the agreement check: returns (match12, nfound).  grid1 / grid2 as for grid_build_kf."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        u8 = lambda a: np.ascontiguousarray(a, np.uint8)
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        use1, use2, u1, v1, u2, v2, lv1, lv2, sf1, sf2 = u8(use1), u8(use2), f32(u1), f32(v1), f32(u2), f32(v2), i32(lv1), i32(lv2), f32(sf1), f32(sf2)
        mp_desc1 = u8(mp_desc1).reshape(-1, 32); mp_desc2 = u8(mp_desc2).reshape(-1, 32)
        kps1 = np.ascontiguousarray(kps1); kps2 = np.ascontiguousarray(kps2); desc1 = u8(desc1).reshape(-1, 32); desc2 = u8(desc2).reshape(-1, 32)
        g1, g2 = f32(grid1), f32(grid2)
        m12 = np.full(len(use1), -1, np.int32)
        nf = C.c_int(0)
        _mchk(self.L.orbm_search_by_sim3(self.h, len(use1), _p(use1), _p(u1), _p(v1), _p(lv1), _p(mp_desc1), len(use2), _p(use2), _p(u2), _p(v2), _p(lv2),
                                         _p(mp_desc2), _p(kps1), _p(desc1), len(kps1), _p(g1), _p(sf1), len(sf1), _p(kps2), _p(desc2), len(kps2), _p(g2),
                                         _p(sf2), len(sf2), C.c_float(th), _p(m12), C.byref(nf)))
        return m12, nf.value

    def SearchForInitialization(self, kps1, desc1, kps2, desc2, prev_matched, windowSize=10):
        """ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:405-520).
        The grid of frame 2 must be current (grid_build(kps2, ...)).  prev_matched (n1, 2) float32 is updated in place;
        returns (vnMatches12, nmatches)."""
        kps1 = np.ascontiguousarray(kps1); kps2 = np.ascontiguousarray(kps2)
        desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        assert prev_matched.dtype == np.float32 and prev_matched.flags["C_CONTIGUOUS"] and prev_matched.shape == (len(kps1), 2)
        m12 = np.full(len(kps1), -1, np.int32)
        nm = C.c_int(0)
        _mchk(self.L.orbm_search_for_initialization(self.h, _p(kps1), _p(desc1), len(kps1), _p(kps2), _p(desc2), len(kps2), _p(prev_matched),
                                                    int(windowSize), C.c_float(self.mfNNratio), 1 if self.mbCheckOrientation else 0, _p(m12), C.byref(nm)))
        return m12, nm.value

    def SearchByBoW(self, kps_kf, desc_kf, featvec_kf, kps_f, desc_f, featvec_f, valid_kf=None):
        """ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (src/ORBmatcher.cc:159-288).  featvec_* are the
        (node ids, offsets, indices) triples of ORBVocabulary.transform; returns (match_f, nmatches) with match_f[i] =
        key-frame feature matched to frame feature i or -1."""
        desc_kf = np.ascontiguousarray(desc_kf, np.uint8).reshape(-1, 32)
        desc_f = np.ascontiguousarray(desc_f, np.uint8).reshape(-1, 32)
        kps_kf = np.ascontiguousarray(kps_kf); kps_f = np.ascontiguousarray(kps_f)
        nk, ok, ik = [np.ascontiguousarray(a, np.int32) for a in featvec_kf]
        nf, of, i_f = [np.ascontiguousarray(a, np.int32) for a in featvec_f]
        if valid_kf is not None:
            valid_kf = np.ascontiguousarray(valid_kf, np.uint8)
        match_f = np.full(len(desc_f), -1, np.int32)
        nm = C.c_int(0)
        _mchk(self.L.orbm_search_by_bow(self.h, _p(desc_kf), _p(kps_kf), len(desc_kf), _p(valid_kf), _p(nk), _p(ok), _p(ik), len(nk),
                                        _p(desc_f), _p(kps_f), len(desc_f), _p(nf), _p(of), _p(i_f), len(nf),
                                        C.c_float(self.mfNNratio), 1 if self.mbCheckOrientation else 0, _p(match_f), C.byref(nm)))
        return match_f, nm.value

    def SearchByBoWBatch(self, kfs, frame):
        """SearchByBoW(pKF, F, ...) for every candidate key frame of Tracking::Relocalization in one call (orbm_search_by_bow_batch).
        kfs: list of (kps, desc, featvec, valid) with valid None = every feature usable; frame: the same tuple (valid ignored).
        Returns (len(kfs) x n_frame int32 table, len(kfs) int32 counts): row c == SearchByBoW(kfs[c], frame)."""
        ks, keep_k = bow_sides(list(kfs))
        fr, keep_f = bow_sides([frame])
        nkf, nf = len(kfs), fr[0].n
        table = np.full((nkf, nf), -1, np.int32)
        counts = np.zeros(nkf, np.int32)
        _mchk(self.L.orbm_search_by_bow_batch(self.h, C.cast(ks, C.c_void_p), nkf, C.cast(fr, C.c_void_p), C.c_float(self.mfNNratio),
                                              1 if self.mbCheckOrientation else 0, _p(table), _p(counts)))
        return table, counts

    def SearchByBoWKFBatch(self, kf1, kfs2):
        """SearchByBoW(pKF1, pKF2, ...) for every candidate key frame of LoopClosing::ComputeSim3 in one call
        (orbm_search_by_bow_kf_batch).  Sides as for SearchByBoWBatch, `valid` required.  Returns (len(kfs2) x n1 int32 table,
        len(kfs2) int32 counts): row c == SearchByBoWKF(kf1, kfs2[c])."""
        k1, keep_1 = bow_sides([kf1])
        ks, keep_k = bow_sides(list(kfs2))
        nkf, n1 = len(kfs2), k1[0].n
        table = np.full((nkf, n1), -1, np.int32)
        counts = np.zeros(nkf, np.int32)
        _mchk(self.L.orbm_search_by_bow_kf_batch(self.h, C.cast(k1, C.c_void_p), C.cast(ks, C.c_void_p), nkf, C.c_float(self.mfNNratio),
                                                 1 if self.mbCheckOrientation else 0, _p(table), _p(counts)))
        return table, counts


class ORBVocabulary:
    """DBoW2 TemplatedVocabulary<FORB> (text format) with the tree descent on the GPU (include/orbv.h)."""

    def __init__(self, path, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        rc = self.L.orbv_load_text(C.byref(self.h), path.encode(), device)
        if rc != ORBX_OK:
            raise OrbxError(rc, self.L.orbv_last_error().decode())
        v = [C.c_int() for _ in range(6)]
        self.L.orbv_info(self.h, *[C.byref(x) for x in v])
        self.k, self.depth, self.nnodes, self.nwords, self.scoring, self.weighting = [x.value for x in v]

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.orbv_destroy(self.h)
            self.h = None

    __del__ = close

    def transform_features(self, desc, levelsup=4):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        w = np.zeros(n, np.int32); nd = np.zeros(n, np.int32); wt = np.zeros(n, np.float64)
        rc = self.L.orbv_transform_features(self.h, _p(desc), n, levelsup, _p(w), _p(nd), _p(wt))
        if rc != ORBX_OK:
            raise OrbxError(rc, self.L.orbv_last_error().decode())
        return w, nd, wt

    def transform(self, desc, levelsup=4):
        """transform(features, BowVector, FeatureVector, levelsup) -> ((ids, vals), (node_ids, off, idx))."""
        w, nd, wt = self.transform_features(desc, levelsup)
        n = len(w)
        ids = np.zeros(max(n, 1), np.int32); vals = np.zeros(max(n, 1), np.float64)
        nb = self.L.orbv_bow_vector(self.h, _p(w), _p(wt), n, _p(ids), _p(vals), len(ids))
        nids = np.zeros(max(n, 1), np.int32); off = np.zeros(n + 1, np.int32); idx = np.zeros(max(n, 1), np.int32)
        nn = self.L.orbv_feature_vector(_p(nd), _p(wt), n, _p(nids), _p(off), _p(idx), len(nids))
        if nb < 0 or nn < 0:
            raise OrbxError(min(nb, nn), self.L.orbv_last_error().decode())
        return (ids[:nb].copy(), vals[:nb].copy()), (nids[:nn].copy(), off[:nn + 1].copy(), idx[:off[nn]].copy())

    def score(self, bow1, bow2):
        return self.L.orbv_score_l1(_p(bow1[0]), _p(bow1[1]), len(bow1[0]), _p(bow2[0]), _p(bow2[1]), len(bow2[0]))


ORBK_RELOC, ORBK_LOOP = 0, 1
ORBK_RECORD = np.dtype([("id", "<u8"), ("words", "<i4"), ("first", "<i4"), ("score", "<f8")])
assert ORBK_RECORD.itemsize == 24


def _kchk(rc):
    if rc != ORBX_OK:
        raise OrbxError(rc, lib().orbk_last_error().decode())


def _bow(bow):
    ids, vals = bow
    return np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vals, np.float64)


class KeyFrameDatabase:
    """ORB_SLAM2::KeyFrameDatabase (src/KeyFrameDatabase.cc) over include/orbk.h.  Keyframes are ids with a BowVector
    (ascending word ids, values); covis maps an id to its GetBestCovisibilityKeyFrames(10), in order."""

    def __init__(self, nwords, scoring=0, device=0, max_keyframes=1024, max_entries=1 << 20):
        self.L = lib()
        self.h = C.c_void_p()
        _kchk(self.L.orbk_create(C.byref(self.h), device, nwords, scoring, max_keyframes, max_entries))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.orbk_destroy(self.h)
            self.h = None

    __del__ = close

    def add(self, kf_id, bow):
        ids, vals = _bow(bow)
        _kchk(self.L.orbk_add(self.h, kf_id, _p(ids), _p(vals), len(ids)))

    def erase(self, kf_id):
        _kchk(self.L.orbk_erase(self.h, kf_id))

    def clear(self):
        _kchk(self.L.orbk_clear(self.h))

    def __len__(self):
        n = self.L.orbk_size(self.h)
        _kchk(min(n, 0))
        return n

    def score(self, bow):
        """One record (id, words, first, score) per live keyframe sharing a word with bow, in add order."""
        ids, vals = _bow(bow)
        n = C.c_int(max(len(self), 1))
        while True:         # another thread may add keyframes after the size is read: retry with the count the call needs
            out = np.zeros(max(n.value, 1), ORBK_RECORD)
            rc = self.L.orbk_score(self.h, _p(ids), _p(vals), len(ids), _p(out), len(out), C.byref(n))
            if rc != ORBX_E_CAPACITY:
                break
        _kchk(rc)
        return out[:n.value].copy()

    def query_begin(self, kind, query_id, bow, connected=(), min_score=0.0, cap=None):
        """Phase 1: returns lScoreAndMatch as (ids uint64, si float32) in encounter order.  With cap given, a scored list
        longer than cap raises ORBX_E_CAPACITY (and changes no state); without it the buffer grows to what the call needs."""
        ids, vals = _bow(bow)
        conn = np.ascontiguousarray(list(connected), np.uint64)
        n = C.c_int(max(len(self), 1) if cap is None else cap)
        while True:         # a capacity error commits no state, so the retry is the same query
            c = n.value if cap is None else cap
            sc = np.zeros(max(c, 1), np.uint64); si = np.zeros(max(c, 1), np.float32)
            rc = self.L.orbk_query_begin(self.h, kind, query_id, _p(ids), _p(vals), len(ids), _p(conn), len(conn),
                                         min_score, _p(sc), _p(si), c, C.byref(n))
            if rc != ORBX_E_CAPACITY or cap is not None:
                break
        _kchk(rc)
        return sc[:n.value].copy(), si[:n.value].copy()

    def query_end(self, kind, scored, covis):
        """Phase 2: covis maps each scored id to its ordered neighbour ids; returns the candidate ids."""
        nb = [list(covis.get(int(k), ())) for k in scored]
        off = np.zeros(len(nb) + 1, np.int32)
        off[1:] = np.cumsum([len(x) for x in nb]) if nb else []
        nb_ids = np.ascontiguousarray([x for l in nb for x in l], np.uint64)
        out = np.zeros(max(len(scored), 1), np.uint64)
        n = C.c_int()
        _kchk(self.L.orbk_query_end(self.h, kind, _p(off), _p(nb_ids), _p(out), len(out), C.byref(n)))
        return [int(x) for x in out[:n.value]]

    def DetectRelocalizationCandidates(self, query_id, bow, covis):
        sc, _ = self.query_begin(ORBK_RELOC, query_id, bow)
        return self.query_end(ORBK_RELOC, sc, covis)

    def DetectLoopCandidates(self, query_id, bow, connected, min_score, covis):
        sc, _ = self.query_begin(ORBK_LOOP, query_id, bow, connected, min_score)
        return self.query_end(ORBK_LOOP, sc, covis)


def UndistortKeyPoints(kps, fx, fy, cx, cy, dist_coef):
    """Frame::UndistortKeyPoints (src/Frame.cc:404-434): mvKeys -> mvKeysUn for mDistCoef = (k1, k2, p1, p2[, k3])."""
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    d = np.ascontiguousarray(dist_coef, np.float32)
    out = np.empty_like(kps)
    _mchk(lib().orbm_undistort_keypoints(_p(kps), len(kps), fx, fy, cx, cy, _p(d), len(d), _p(out)))
    return out


def ComputeImageBounds(width, height, fx, fy, cx, cy, dist_coef):
    """Frame::ComputeImageBounds (src/Frame.cc:436-463) -> (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    d = np.ascontiguousarray(dist_coef, np.float32)
    b = np.zeros(4, np.float32)
    _mchk(lib().orbm_image_bounds(width, height, fx, fy, cx, cy, _p(d), len(d), _p(b)))
    return tuple(float(v) for v in b)


def _pchk(rc):
    if rc < 0:
        raise OrbxError(rc, lib().orbp_last_error().decode())
    return rc


class PnPsolver:
    """Mirror of ORB_SLAM2::PnPsolver (include/PnPsolver.h:66-78, src/PnPsolver.cc:66-344) over orbp_pnp_*: host-side
    EPnP RANSAC.  The Frame / MapPoint arguments of the reference constructor become the arrays it reads from them:
    p2d = mvKeysUn[i].pt, sigma2 = mvLevelSigma2[octave], p3d = GetWorldPos() of the non-bad matches."""

    def __init__(self, p2d, sigma2, p3d, fx, fy, cx, cy, rand=None, rand_max=None):
        self.L = lib()
        self.p2d = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
        self.sigma2 = np.ascontiguousarray(sigma2, np.float32)
        self.p3d = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
        self.N = len(self.p2d)
        self.h = C.c_void_p()
        _pchk(self.L.orbp_pnp_create(C.byref(self.h), self.N, _p(self.p2d), _p(self.sigma2), _p(self.p3d), fx, fy, cx, cy))
        self._cb = None
        if rand is not None:
            self._cb = RAND_FN(lambda ctx: int(rand()))
            self.L.orbp_pnp_set_rand(self.h, self._cb, None, int(rand_max))

    def close(self):
        if self.h:
            self.L.orbp_pnp_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        _pchk(self.L.orbp_pnp_set_ransac_parameters(self.h, probability, minInliers, maxIterations, minSet, epsilon, th2))

    def ransac_state(self):
        mi, mx, it, ep = C.c_int(), C.c_int(), C.c_int(), C.c_float()
        self.L.orbp_pnp_get_ransac_state(self.h, C.byref(mi), C.byref(mx), C.byref(ep), C.byref(it))
        return {"min_inliers": mi.value, "max_its": mx.value, "epsilon": ep.value, "iterations": it.value}

    def iterate(self, nIterations):
        """-> (Tcw 4x4 float32 or None, bNoMore, vbInliers (bool[N]) or None, nInliers)"""
        no_more, ninl = C.c_int(), C.c_int()
        inl = np.zeros(max(self.N, 1), np.uint8)
        T = np.zeros(16, np.float32)
        got = _pchk(self.L.orbp_pnp_iterate(self.h, nIterations, C.byref(no_more), _p(inl), C.byref(ninl), _p(T)))
        if not got:
            return None, bool(no_more.value), None, 0
        return T.reshape(4, 4), bool(no_more.value), inl[:self.N].astype(bool), ninl.value

    def find(self):
        st = self.ransac_state()
        T, _, inl, n = self.iterate(st["max_its"])
        return T, inl, n

    def _problem(self):
        n = max(self.N, 1)
        p2d, p3d, e = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        K, ms = np.zeros(4, np.float32), C.c_int32()
        _pchk(self.L.orbp_pnp_get_problem(self.h, _p(p2d), _p(p3d), _p(e), _p(K), C.byref(ms)))
        return p2d[:self.N], p3d[:self.N], e[:self.N], K, ms.value

    @property
    def min_set(self):
        return self._problem()[4]

    def max_errors(self):
        """mvMaxError = sigma2 * th2 as the floats CheckInliers compares with"""
        return self._problem()[2]

    def draw(self, nIterations):
        """The index sets (int32 [k, min_set]) of the iterations a following iterate(nIterations) consumes beyond the queued ones,
        k = max(max_its - iterations, nIterations) - queued because of the reference's `||` loop: drawn now, consumed by iterate()"""
        st, ms = self.ransac_state(), self.min_set
        room = max(st["max_its"] - st["iterations"], nIterations, 1)
        sm = np.zeros((room, ms), np.int32)
        k = _pchk(self.L.orbp_pnp_draw(self.h, nIterations, _p(sm)))
        return sm[:k].copy()

    def queued(self):
        ms = self.min_set
        k = _pchk(self.L.orbp_pnp_queued(self.h, None))
        sm = np.zeros((max(k, 1), ms), np.int32)
        _pchk(self.L.orbp_pnp_queued(self.h, _p(sm)))
        return sm[:k].copy()

    def problem(self):
        """This solver as a problem of ORBmatcher.pnp_hypotheses: its correspondences and its queued samples"""
        p2d, p3d, e, K, ms = self._problem()
        return p2d, p3d, e, K, ms, self.queued()

    def hypothesis(self, sample):
        """One hypothesis on the host -> (R 3x3 float64, t (3) float64, inliers bool[N], nInliers)"""
        sm = np.ascontiguousarray(sample, np.int32).reshape(-1)
        if len(sm) != self.min_set:
            raise OrbxError(ORBX_E_INVALID, "a sample of %d indices for min_set %d" % (len(sm), self.min_set))
        R, t, n = np.zeros(9), np.zeros(3), C.c_int()
        inl = np.zeros(max(self.N, 1), np.uint8)
        _pchk(self.L.orbp_pnp_hypothesis(self.h, _p(sm), _p(R), _p(t), _p(inl), C.byref(n)))
        return R.reshape(3, 3), t, inl[:self.N].astype(bool), n.value

    def hypotheses(self, samples):
        """hypothesis() for each sample, in the layout of ORBmatcher.pnp_hypotheses: (n_inliers [h], Rt [h, 12], masks [h, W])"""
        samples = np.asarray(samples, np.int32).reshape(-1, self.min_set)
        W = (self.N + 31) // 32
        cnt, Rt, masks = np.zeros(len(samples), np.int32), np.zeros((len(samples), 12)), np.zeros((len(samples), W), np.uint32)
        for k, sm in enumerate(samples):
            R, t, inl, n = self.hypothesis(sm)
            cnt[k] = n
            Rt[k, :9], Rt[k, 9:] = R.reshape(9), t
            bits = np.zeros(W * 32, np.uint8)
            bits[:self.N] = inl
            masks[k] = np.packbits(bits, bitorder="little").view("<u4")
        return cnt, Rt, masks

    def attach_results(self, n_inliers, Rt, masks):
        cnt = np.ascontiguousarray(n_inliers, np.int32).reshape(-1)
        Rt = np.ascontiguousarray(Rt, np.float64).reshape(-1)
        masks = np.ascontiguousarray(masks, np.uint32).reshape(-1)
        W = (self.N + 31) // 32
        if len(Rt) != 12 * len(cnt) or len(masks) != W * len(cnt):
            raise OrbxError(ORBX_E_INVALID, "results of %d hypotheses: %d doubles, %d mask words" % (len(cnt), len(Rt), len(masks)))
        _pchk(self.L.orbp_pnp_attach_results(self.h, len(cnt), _p(cnt), _p(Rt), _p(masks)))

    @staticmethod
    def EvaluateAll(solvers, matcher, n_iterations=5):
        """Tracking::Relocalization's batch step: draws for every solver what its next iterate(n_iterations) consumes (solver by
        solver; None entries and solvers with min_set > 8 are skipped and stay on the host), evaluates all of it in ONE
        ORBmatcher.pnp_hypotheses call and attaches the results, so that the iterations that follow are replays."""
        live = [s for s in solvers if s is not None and s.min_set <= ORBM_PNP_MAX_SET]
        for s in live:
            s.draw(n_iterations)
        for s, res in zip(live, matcher.pnp_hypotheses(live)):
            s.attach_results(*res)


class Sim3Solver:
    """Mirror of ORB_SLAM2::Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) over orbp_sim3_*.  The KeyFrame / MapPoint
    arguments of the reference constructor become the arrays it reads from them: x3dc1 / x3dc2 = Rcw*Xw+tcw of the matched pair in
    key frame 1 / 2, sigma2_1 / sigma2_2 = mvLevelSigma2[octave] of its keypoints, K1 / K2 = (fx, fy, cx, cy)."""

    def __init__(self, x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, bFixScale=True, rand=None, rand_max=None):
        self.L = lib()
        self.x1 = np.ascontiguousarray(x3dc1, np.float32).reshape(-1, 3)
        self.x2 = np.ascontiguousarray(x3dc2, np.float32).reshape(-1, 3)
        s1, s2 = np.ascontiguousarray(sigma2_1, np.float32).reshape(-1), np.ascontiguousarray(sigma2_2, np.float32).reshape(-1)
        self.K1, self.K2 = np.ascontiguousarray(K1, np.float32).reshape(4), np.ascontiguousarray(K2, np.float32).reshape(4)
        self.fix_scale = bool(bFixScale)
        self.N = len(self.x1)
        if not (len(self.x2) == len(s1) == len(s2) == self.N):
            raise OrbxError(ORBX_E_INVALID, "array lengths disagree: %d / %d / %d / %d" % (self.N, len(self.x2), len(s1), len(s2)))
        if rand is not None and rand_max is None:
            raise OrbxError(ORBX_E_INVALID, "Sim3Solver: rand needs rand_max, the largest value rand() returns")
        self.W = (self.N + 31) // 32
        self.h = C.c_void_p()
        _pchk(self.L.orbp_sim3_create(C.byref(self.h), self.N, _p(self.x1), _p(self.x2), _p(s1), _p(s2), _p(self.K1), _p(self.K2),
                                      int(self.fix_scale)))
        self._cb = None
        if rand is not None:
            self._cb = RAND_FN(lambda ctx: int(rand()))
            self.L.orbp_sim3_set_rand(self.h, self._cb, None, int(rand_max))

    def close(self):
        if self.h:
            self.L.orbp_sim3_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        _pchk(self.L.orbp_sim3_set_ransac_parameters(self.h, probability, minInliers, maxIterations))

    def ransac_state(self):
        mi, mx, it, nb, ep = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_float()
        self.L.orbp_sim3_get_ransac_state(self.h, C.byref(mi), C.byref(mx), C.byref(ep), C.byref(it), C.byref(nb))
        return {"min_inliers": mi.value, "max_its": mx.value, "epsilon": ep.value, "iterations": it.value, "best_inliers": nb.value}

    def max_errors(self):
        """mvnMaxError1 / mvnMaxError2 as the floats CheckInliers compares with"""
        n = max(self.N, 1)
        x1, x2, e1, e2 = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        K1, K2, fix = np.zeros(4, np.float32), np.zeros(4, np.float32), C.c_int32()
        _pchk(self.L.orbp_sim3_get_problem(self.h, _p(x1), _p(x2), _p(e1), _p(e2), _p(K1), _p(K2), C.byref(fix)))
        return e1[:self.N], e2[:self.N]

    def draw(self, nIterations):
        """The triples of the next nIterations iterations (int32 [k, 3], k capped at what remains): drawn now, consumed by iterate()"""
        tri = np.zeros((max(nIterations, 1), 3), np.int32)
        k = _pchk(self.L.orbp_sim3_draw(self.h, nIterations, _p(tri)))
        return tri[:k].copy()

    def queued(self):
        k = _pchk(self.L.orbp_sim3_queued(self.h, None))
        tri = np.zeros((max(k, 1), 3), np.int32)
        _pchk(self.L.orbp_sim3_queued(self.h, _p(tri)))
        return tri[:k].copy()

    def problem(self):
        """This solver as a problem of ORBmatcher.sim3_hypotheses: its correspondences and its queued triples"""
        e1, e2 = self.max_errors()
        return self.x1, self.x2, e1, e2, self.K1, self.K2, self.fix_scale, self.queued()

    def hypothesis(self, triple):
        """One hypothesis on the host -> (R 3x3, t (3), scale, inliers bool[N], nInliers)"""
        tri = np.ascontiguousarray(triple, np.int32).reshape(3)
        R, t, sc, n = np.zeros(9, np.float32), np.zeros(3, np.float32), C.c_float(), C.c_int()
        inl = np.zeros(max(self.N, 1), np.uint8)
        _pchk(self.L.orbp_sim3_hypothesis(self.h, _p(tri), _p(R), _p(t), C.byref(sc), _p(inl), C.byref(n)))
        return R.reshape(3, 3), t, np.float32(sc.value), inl[:self.N].astype(bool), n.value

    def hypotheses(self, triples):
        """hypothesis() for each triple, in the layout of ORBmatcher.sim3_hypotheses: (n_inliers [h], sRt [h, 13], masks [h, W])"""
        triples = np.asarray(triples, np.int32).reshape(-1, 3)
        cnt, sRt, masks = np.zeros(len(triples), np.int32), np.zeros((len(triples), 13), np.float32), np.zeros((len(triples), self.W), np.uint32)
        for k, tri in enumerate(triples):
            R, t, sc, inl, n = self.hypothesis(tri)
            cnt[k] = n
            sRt[k, 0], sRt[k, 1:10], sRt[k, 10:13] = sc, R.reshape(9), t
            bits = np.zeros(self.W * 32, np.uint8)
            bits[:self.N] = inl
            masks[k] = np.packbits(bits, bitorder="little").view("<u4")
        return cnt, sRt, masks

    def attach_results(self, n_inliers, sRt, masks):
        cnt = np.ascontiguousarray(n_inliers, np.int32).reshape(-1)
        sRt = np.ascontiguousarray(sRt, np.float32).reshape(-1)
        masks = np.ascontiguousarray(masks, np.uint32).reshape(-1)
        if len(sRt) != 13 * len(cnt) or len(masks) != self.W * len(cnt):
            raise OrbxError(ORBX_E_INVALID, "results of %d hypotheses: %d floats, %d mask words" % (len(cnt), len(sRt), len(masks)))
        _pchk(self.L.orbp_sim3_attach_results(self.h, len(cnt), _p(cnt), _p(sRt), _p(masks)))

    def iterate(self, nIterations):
        """-> (T12 4x4 float32 or None, bNoMore, vbInliers bool[N] (all False without a pose), nInliers)"""
        no_more, ninl = C.c_int(), C.c_int()
        inl = np.zeros(max(self.N, 1), np.uint8)
        T = np.zeros(16, np.float32)
        got = _pchk(self.L.orbp_sim3_iterate(self.h, nIterations, C.byref(no_more), _p(inl), C.byref(ninl), _p(T)))
        return (T.reshape(4, 4) if got else None), bool(no_more.value), inl[:self.N].astype(bool), ninl.value

    def find(self):
        ninl = C.c_int()
        inl = np.zeros(max(self.N, 1), np.uint8)
        T = np.zeros(16, np.float32)
        got = _pchk(self.L.orbp_sim3_find(self.h, _p(inl), C.byref(ninl), _p(T)))
        return (T.reshape(4, 4) if got else None), inl[:self.N].astype(bool), ninl.value

    def estimated(self):
        """GetEstimatedRotation / Translation / Scale -> (R 3x3, t (3), scale), or None before the first iteration"""
        R, t, sc = np.zeros(9, np.float32), np.zeros(3, np.float32), C.c_float()
        if not _pchk(self.L.orbp_sim3_get_estimated(self.h, _p(R), _p(t), C.byref(sc))):
            return None
        return R.reshape(3, 3), t, np.float32(sc.value)

    @staticmethod
    def EvaluateAll(solvers, matcher):
        """LoopClosing::ComputeSim3's batch step: draws every solver's remaining triples (None entries are skipped), evaluates all of
        them in ONE ORBmatcher.sim3_hypotheses call and attaches the results, so that every later iterate() is a replay."""
        live = [s for s in solvers if s is not None]
        for s in live:
            s.draw(s.ransac_state()["max_its"])
        for s, res in zip(live, matcher.sim3_hypotheses(live)):
            s.attach_results(*res)


class Initializer:
    """Mirror of ORB_SLAM2::Initializer (include/Initializer.h, src/Initializer.cc) over orbp_init_*.  The Frame arguments of the
    reference become the arrays it reads from them: keys = mvKeysUn[i].pt, K = (fx, fy, cx, cy) of mK."""

    def __init__(self, keys1, K, sigma=1.0, iterations=200, rand=None, rand_max=None):
        self.L = lib()
        self.keys1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        self.K = np.ascontiguousarray(K, np.float32).reshape(4)
        self.n1, self.iterations, self.sigma = len(self.keys1), int(iterations), float(sigma)
        if rand is not None and rand_max is None:
            raise OrbxError(ORBX_E_INVALID, "Initializer: rand needs rand_max, the largest value rand() returns")
        self.h = C.c_void_p()
        _pchk(self.L.orbp_init_create(C.byref(self.h), _p(self.keys1), self.n1, *[float(k) for k in self.K], self.sigma, self.iterations))
        self._cb = None
        if rand is not None:
            self._cb = RAND_FN(lambda ctx: int(rand()))
            self.L.orbp_init_set_rand(self.h, self._cb, None, int(rand_max))
        self.N = self.n2 = 0
        self.use_gpu = True
        self.last_error = ""

    def close(self):
        if self.h:
            self.L.orbp_init_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def SetRand(self, rand, rand_max):
        self._cb = RAND_FN(lambda ctx: int(rand())) if rand is not None else None
        self.L.orbp_init_set_rand(self.h, self._cb if self._cb is not None else C.cast(None, RAND_FN), None, int(rand_max or 0))

    def SetUseGpu(self, on):
        self.use_gpu = bool(on)

    def LastError(self):
        return self.last_error

    def set_current(self, keys2, matches12):
        """Initialize's first lines (:49-63) and both Normalize calls; returns N = mvMatches12.size()"""
        keys2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
        m = np.ascontiguousarray(matches12, np.int32).reshape(-1)
        if len(m) != self.n1:
            raise OrbxError(ORBX_E_INVALID, "matches12 has %d entries for %d reference keys" % (len(m), self.n1))
        self.n2 = len(keys2)
        self.N = _pchk(self.L.orbp_init_set_current(self.h, _p(keys2), self.n2, _p(m)))
        self.W = (self.N + 31) // 32
        return self.N

    def normalized(self):
        """-> (vPn1 [n1, 2], T1 3x3, vPn2 [n2, 2], T2 3x3) of Normalize (:749-795)"""
        pn1, pn2 = np.zeros((max(self.n1, 1), 2), np.float32), np.zeros((max(self.n2, 1), 2), np.float32)
        T1, T2 = np.zeros(9, np.float32), np.zeros(9, np.float32)
        _pchk(self.L.orbp_init_normalized(self.h, _p(pn1), _p(T1), _p(pn2), _p(T2)))
        return pn1[:self.n1], T1.reshape(3, 3), pn2[:self.n2], T2.reshape(3, 3)

    def draw(self):
        """mvSets (:82-97): int32 [iterations, 8]"""
        sets = np.zeros((max(self.iterations, 1), 8), np.int32)
        k = _pchk(self.L.orbp_init_draw(self.h, _p(sets)))
        return sets[:k].copy()

    def _get(self):
        n = max(self.N, 1)
        uv, pn, params = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros(24, np.float32)
        sets, m1, m2 = np.zeros((max(self.iterations, 1), 8), np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        drawn = C.c_int()
        _pchk(self.L.orbp_init_get_sizes(self.h, None, None, None, None, C.byref(drawn)))
        _pchk(self.L.orbp_init_get_problem(self.h, _p(uv), _p(pn), _p(params), _p(sets), _p(m1), _p(m2)))
        return uv[:self.N], pn[:self.N], params, sets[:self.iterations if drawn.value else 0], m1[:self.N], m2[:self.N]

    def matches(self):
        """mvMatches12 as (first int32 [N], second int32 [N])"""
        g = self._get()
        return g[4], g[5]

    def problem(self):
        """This solver as a problem of ORBmatcher.init_hypotheses: the H of every drawn set, then the F"""
        uv, pn, params, sets, _, _ = self._get()
        models = np.repeat(np.array([INIT_MODEL_H, INIT_MODEL_F], np.int32), len(sets))
        return uv, pn, params[:9], params[9:18], params[18], np.concatenate([sets, sets]), models

    def check_rt_inputs(self):
        """-> (uv [N, 4], K (4), th2) of ORBmatcher.init_check_rt"""
        uv, _, params, _, _, _ = self._get()
        return uv, params[19:23].copy(), float(params[23])

    def hypothesis(self, model, set8):
        """One hypothesis on the host -> (M 3x3, score float32, inliers bool[N], nInliers)"""
        st = np.ascontiguousarray(set8, np.int32).reshape(8)
        M, sc, n = np.zeros(9, np.float32), C.c_float(), C.c_int()
        inl = np.zeros(max(self.N, 1), np.uint8)
        _pchk(self.L.orbp_init_hypothesis(self.h, int(model), _p(st), _p(M), C.byref(sc), _p(inl), C.byref(n)))
        return M.reshape(3, 3), np.float32(sc.value), inl[:self.N].astype(bool), n.value

    def hypotheses(self, sets, models):
        """hypothesis() for each (set, model), in the layout of ORBmatcher.init_hypotheses: (score_M [h, 10], n_inliers [h], masks [h, W])"""
        sets = np.asarray(sets, np.int32).reshape(-1, 8)
        models = np.asarray(models, np.int32).reshape(-1)
        sm, cnt, masks = np.zeros((len(sets), 10), np.float32), np.zeros(len(sets), np.int32), np.zeros((len(sets), self.W), np.uint32)
        for k, (st, md) in enumerate(zip(sets, models)):
            M, sc, inl, n = self.hypothesis(md, st)
            cnt[k] = n
            sm[k, 0], sm[k, 1:] = sc, M.reshape(9)
            bits = np.zeros(self.W * 32, np.uint8)
            bits[:self.N] = inl
            masks[k] = np.packbits(bits, bitorder="little").view("<u4")
        return sm, cnt, masks

    def attach_results(self, score_M, n_inliers, masks):
        sm = np.ascontiguousarray(score_M, np.float32).reshape(-1)
        cnt = np.ascontiguousarray(n_inliers, np.int32).reshape(-1)
        masks = np.ascontiguousarray(masks, np.uint32).reshape(-1)
        if len(sm) != 10 * len(cnt) or len(masks) != self.W * len(cnt):
            raise OrbxError(ORBX_E_INVALID, "results of %d hypotheses: %d floats, %d mask words" % (len(cnt), len(sm), len(masks)))
        _pchk(self.L.orbp_init_attach_results(self.h, len(cnt), _p(sm), _p(cnt), _p(masks)))

    def find(self, model):
        """FindHomography (model 0) / FindFundamental (1) -> (M 3x3, score, inliers bool[N], winning iteration or -1)"""
        M, sc, it = np.zeros(9, np.float32), C.c_float(), C.c_int()
        inl = np.zeros(max(self.N, 1), np.uint8)
        _pchk(self.L.orbp_init_find(self.h, int(model), _p(M), C.byref(sc), _p(inl), C.byref(it)))
        return M.reshape(3, 3), np.float32(sc.value), inl[:self.N].astype(bool), it.value

    def motions(self, model, M):
        """-> Rt float32 [k, 12] (R row-major, t): 4 for F, 8 for H, none at ReconstructH's singular-value exit"""
        M = np.ascontiguousarray(M, np.float32).reshape(9)
        Rt, n = np.zeros((8, 12), np.float32), C.c_int()
        _pchk(self.L.orbp_init_motions(self.h, int(model), _p(M), _p(Rt), C.byref(n)))
        return Rt[:n.value].copy()

    def check_rt(self, R, t, inliers):
        """CheckRT on the host -> (nGood, vP3D [n1, 3], vbGood bool[n1], parallax)"""
        R, t = np.ascontiguousarray(R, np.float32).reshape(9), np.ascontiguousarray(t, np.float32).reshape(3)
        inl = np.ascontiguousarray(np.asarray(inliers).astype(np.uint8)).reshape(-1)
        if len(inl) != self.N:
            raise OrbxError(ORBX_E_INVALID, "check_rt: %d flags for %d matches" % (len(inl), self.N))
        inl = np.concatenate([inl, np.zeros(1, np.uint8)])
        p3d, good = np.zeros((max(self.n1, 1), 3), np.float32), np.zeros(max(self.n1, 1), np.uint8)
        par, n = C.c_float(), C.c_int()
        _pchk(self.L.orbp_init_check_rt(self.h, _p(R), _p(t), _p(inl), _p(p3d), _p(good), C.byref(par), C.byref(n)))
        return n.value, p3d[:self.n1], good[:self.n1].astype(bool), np.float32(par.value)

    def check_rt_matches(self, Rt, inliers):
        """The per-match part of CheckRT on the host, in the layout of ORBmatcher.init_check_rt"""
        Rt = np.ascontiguousarray(Rt, np.float32).reshape(-1, 12)
        inl = np.concatenate([np.asarray(inliers).astype(np.uint8).reshape(-1), np.zeros(1, np.uint8)])
        k, n = len(Rt), self.N
        status, cosp, p3d = np.zeros((k, max(n, 1)), np.uint8), np.zeros((k, max(n, 1)), np.float32), np.zeros((k, max(n, 1), 3), np.float32)
        if n:
            _pchk(self.L.orbp_init_check_rt_matches(self.h, k, _p(Rt), _p(inl), _p(status), _p(cosp), _p(p3d)))
        return status[:, :n], cosp[:, :n], p3d[:, :n]

    def attach_check_rt(self, Rt, inliers, status, cos_parallax, p3d):
        Rt = np.ascontiguousarray(Rt, np.float32).reshape(-1, 12)
        inl = np.concatenate([np.asarray(inliers).astype(np.uint8).reshape(-1), np.zeros(1, np.uint8)])
        _pchk(self.L.orbp_init_attach_check_rt(self.h, len(Rt), _p(Rt), _p(inl), _p(np.ascontiguousarray(status, np.uint8)),
                                               _p(np.ascontiguousarray(cos_parallax, np.float32)), _p(np.ascontiguousarray(p3d, np.float32))))

    def plan_check_rt(self):
        """Initialize up to its CheckRT calls -> (model, M 3x3, inliers bool[N], Rt [k, 12]); k = 0: Initialize returns false before them"""
        model, n = C.c_int(), C.c_int()
        M, Rt, inl = np.zeros(9, np.float32), np.zeros((8, 12), np.float32), np.zeros(max(self.N, 1), np.uint8)
        _pchk(self.L.orbp_init_plan_check_rt(self.h, C.byref(model), _p(M), _p(inl), _p(Rt), C.byref(n)))
        return model.value, M.reshape(3, 3), inl[:self.N].astype(bool), Rt[:n.value].copy()

    def initialize(self):
        """orbp_init_initialize on the current pair -> (ok, R21 3x3, t21 (3), vP3D [n1, 3], vbTriangulated bool[n1])"""
        R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
        p3d, tri = np.zeros((max(self.n1, 1), 3), np.float32), np.zeros(max(self.n1, 1), np.uint8)
        ok = _pchk(self.L.orbp_init_initialize(self.h, _p(R), _p(t), _p(p3d), _p(tri)))
        return bool(ok), R.reshape(3, 3), t, p3d[:self.n1], tri[:self.n1].astype(bool)

    def Initialize(self, keys2, matches12, matcher=None):
        """Initializer::Initialize (:44-121) -> (ok, R21, t21, vP3D, vbTriangulated).  With a matcher (and SetUseGpu(True)) the
        hypotheses and the CheckRT passes are one GPU call each; when a GPU call fails the host path gives the same bytes and
        LastError() says why."""
        self.set_current(keys2, matches12)
        self.draw()
        self.last_error = ""
        if matcher is not None and self.use_gpu:
            try:
                self.attach_results(*matcher.init_hypotheses([self])[0])
                model, M, inl, Rt = self.plan_check_rt()
                if len(Rt):
                    uv, K, th2 = self.check_rt_inputs()
                    self.attach_check_rt(Rt, inl, *matcher.init_check_rt(uv, inl, K, th2, Rt))
            except OrbxError as e:
                self.last_error = str(e)
        return self.initialize()


def epnp(pws, us, fu, fv, uc, vc):
    """PnPsolver::compute_pose (src/PnPsolver.cc:458-508) on all given correspondences -> (R, t, mean reprojection error)."""
    pws = np.ascontiguousarray(pws, np.float64).reshape(-1, 3)
    us = np.ascontiguousarray(us, np.float64).reshape(-1, 2)
    R, t = np.zeros((3, 3)), np.zeros(3)
    err = lib().orbp_epnp(len(pws), _p(pws), _p(us), fu, fv, uc, vc, _p(R), _p(t))
    if err < 0:
        raise OrbxError(ORBX_E_INVALID, lib().orbp_last_error().decode())
    return R, t, err


def sim3_from_rts(R, t, s):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) (src/LoopClosing.cc:326) -> float64 [8] in the order of
    g2o::Sim3::operator[]: qx, qy, qz, qw, tx, ty, tz, s."""
    R = np.ascontiguousarray(R, np.float32).reshape(9)
    t = np.ascontiguousarray(t, np.float32).reshape(3)
    out = np.zeros(8, np.float64)
    _pchk(lib().orbp_sim3_from_rts(_p(R), _p(t), s, _p(out)))
    return out


def OptimizeSim3(x1c, x2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2, th2, fix_scale, S12):
    """Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) on the host -> (S12 float64 [8], flags bool[n], nIn).  x1c / x2c:
    R1w*P3D1w+t1w and R2w*P3D2w+t2w of the gathered correspondences, obs1 / obs2 their key points, K1 / K2 = (fx, fy, cx, cy), S12 =
    g2oS12 as sim3_from_rts() orders it.  flags marks the correspondences the reference sets to NULL in vpMatches1."""
    x1c = np.ascontiguousarray(x1c, np.float32).reshape(-1, 3)
    x2c = np.ascontiguousarray(x2c, np.float32).reshape(-1, 3)
    obs1 = np.ascontiguousarray(obs1, np.float32).reshape(-1, 2)
    obs2 = np.ascontiguousarray(obs2, np.float32).reshape(-1, 2)
    s1 = np.ascontiguousarray(inv_sigma2_1, np.float32).reshape(-1)
    s2 = np.ascontiguousarray(inv_sigma2_2, np.float32).reshape(-1)
    n = len(x1c)
    if not (len(x2c) == len(obs1) == len(obs2) == len(s1) == len(s2) == n):
        raise OrbxError(ORBX_E_INVALID, "OptimizeSim3: array lengths disagree")
    K1 = np.ascontiguousarray(K1, np.float32).reshape(4)
    K2 = np.ascontiguousarray(K2, np.float32).reshape(4)
    S = np.ascontiguousarray(S12, np.float64).reshape(8).copy()
    flags = np.zeros(max(n, 1), np.uint8)
    n_in = _pchk(lib().orbp_optimize_sim3(n, _p(x1c), _p(x2c), _p(obs1), _p(obs2), _p(s1), _p(s2), _p(K1), _p(K2), th2,
                                          1 if fix_scale else 0, _p(S), _p(flags)))
    return S, flags[:n].astype(bool), n_in


def PoseOptimization(obs, inv_sigma2, xw, fx, fy, cx, cy, Tcw, u_right=None, bf=0.0):
    """Optimizer::PoseOptimization (src/Optimizer.cc:239-451) -> (Tcw 4x4 float32, mvbOutlier bool[n], n_inliers)."""
    obs = np.ascontiguousarray(obs, np.float32).reshape(-1, 2)
    inv_sigma2 = np.ascontiguousarray(inv_sigma2, np.float32)
    xw = np.ascontiguousarray(xw, np.float32).reshape(-1, 3)
    ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16).copy()
    out = np.zeros(max(len(obs), 1), np.uint8)
    n = _pchk(lib().orbp_pose_optimization(len(obs), _p(obs), _p(ur), _p(inv_sigma2), _p(xw), fx, fy, cx, cy, bf, _p(T), _p(out)))
    return T.reshape(4, 4), out[:len(obs)].astype(bool), n


class LbaProblem(C.Structure):
    """orbp_lba_problem (include/orbp.h)"""
    _fields_ = [("n_local", C.c_int32), ("n_fixed", C.c_int32), ("n_points", C.c_int32), ("local_fixed", C.c_void_p),
                ("Tcw", C.c_void_p), ("cam", C.c_void_p), ("edge_off", C.c_void_p), ("edge_kf", C.c_void_p), ("obs", C.c_void_p),
                ("u_right", C.c_void_p), ("inv_sigma2", C.c_void_p)]


class LbaStats(C.Structure):
    """orbp_lba_stats (include/orbp.h)"""
    _fields_ = [("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("lambda_", C.c_double), ("chi2", C.c_double),
                ("n_level1", C.c_int32), ("second_round", C.c_int32)]

    def as_dict(self):
        return {"iterations": tuple(self.iterations), "trials": tuple(self.trials), "lambda": self.lambda_, "chi2": self.chi2,
                "n_level1": self.n_level1, "second_round": self.second_round}


ORBP_LBA_DONE, ORBP_LBA_STOPPED = 0, 1


def pack_lba_problem(problem):
    """The flat arrays of orbp_local_bundle_adjustment / orbm_local_bundle_adjustment from a dict gathered as
    Optimizer::LocalBundleAdjustment walks (src/Optimizer.cc:455-653): local_fixed uint8 [n_local] (mnId == 0), Tcw float32
    [n_local + n_fixed, 4, 4] and cam float32 [n_local + n_fixed, 5] = (fx, fy, cx, cy, bf), local key frames first; xw float32
    [n_points, 3]; edge_off int32 [n_points + 1]; per edge edge_kf int32, obs float32 [E, 2], u_right float32 (< 0: monocular),
    inv_sigma2 float32.  -> (LbaProblem, arrays): the struct points into `arrays` (a dict of contiguous copies, xw among them),
    which must outlive it."""
    a = {"local_fixed": np.ascontiguousarray(problem["local_fixed"], np.uint8).reshape(-1),
         "Tcw": np.ascontiguousarray(problem["Tcw"], np.float32).reshape(-1, 16),
         "cam": np.ascontiguousarray(problem["cam"], np.float32).reshape(-1, 5),
         "xw": np.array(problem["xw"], np.float32).reshape(-1, 3),
         "edge_off": np.ascontiguousarray(problem["edge_off"], np.int32).reshape(-1),
         "edge_kf": np.ascontiguousarray(problem["edge_kf"], np.int32).reshape(-1),
         "obs": np.ascontiguousarray(problem["obs"], np.float32).reshape(-1, 2),
         "u_right": np.ascontiguousarray(problem["u_right"], np.float32).reshape(-1),
         "inv_sigma2": np.ascontiguousarray(problem["inv_sigma2"], np.float32).reshape(-1)}
    n_local, n_kf, n_points, E = len(a["local_fixed"]), len(a["Tcw"]), len(a["xw"]), len(a["edge_kf"])
    if len(a["cam"]) != n_kf or n_kf < n_local or len(a["edge_off"]) != n_points + 1:
        raise OrbxError(ORBX_E_INVALID, "pack_lba_problem: key frame / point array lengths disagree")
    if not (len(a["obs"]) == len(a["u_right"]) == len(a["inv_sigma2"]) == E) or (E and int(a["edge_off"][-1]) != E):
        raise OrbxError(ORBX_E_INVALID, "pack_lba_problem: edge array lengths disagree")
    s = LbaProblem(n_local, n_kf - n_local, n_points, *[a[k].ctypes.data if a[k].size else None for k in
                                                        ("local_fixed", "Tcw", "cam", "edge_off", "edge_kf", "obs", "u_right", "inv_sigma2")])
    s.edge_off = a["edge_off"].ctypes.data
    return s, a


def _lba_call(fn, problem, stop):
    s, a = pack_lba_problem(problem)
    E = len(a["edge_kf"])
    Tcw = np.zeros((max(s.n_local, 1), 4, 4), np.float32)
    erase = np.zeros(max(E, 1), np.uint8)
    stats = LbaStats()
    stop_arr = None if stop is None else np.ascontiguousarray(stop, np.uint8).reshape(1)
    rc = fn(C.byref(s), _p(Tcw), _p(a["xw"]), _p(erase), _p(stop_arr), C.byref(stats))
    return rc, Tcw[:s.n_local], a["xw"], erase[:E].astype(bool), stats.as_dict()


def LocalBundleAdjustment(problem, stop=None):
    """Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778) on the host over a pack_lba_problem() dict -> (code, Tcw float32
    [n_local, 4, 4], xw float32 [n_points, 3], erase bool [E], stats dict).  code: ORBP_LBA_DONE, or ORBP_LBA_STOPPED when `stop`
    (a uint8 [1], as pbStopFlag) was set at entry: the outputs are then zeros and the input points."""
    rc, Tcw, xw, erase, stats = _lba_call(lib().orbp_local_bundle_adjustment, problem, stop)
    return _pchk(rc), Tcw, xw, erase, stats


class BaStats(C.Structure):
    """orbp_ba_stats (include/orbp.h)"""
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("lambda_", C.c_double), ("chi2", C.c_double)]

    def as_dict(self):
        return {"iterations": self.iterations, "trials": self.trials, "lambda": self.lambda_, "chi2": self.chi2}


ORBP_BA_MAX_ITERATIONS = 100
ORBM_BA_MAX_KFS, ORBM_BA_MAX_TABLE, ORBM_SPD_MAX_N = 512, 1 << 26, 3072


def _ba_call(fn, problem, n_iterations, robust, stop):
    s, a = pack_lba_problem(problem)
    Tcw = np.zeros((max(s.n_local, 1), 4, 4), np.float32)
    stats = BaStats()
    stop_arr = None if stop is None else np.ascontiguousarray(stop, np.uint8).reshape(1)
    rc = fn(C.byref(s), int(n_iterations), 1 if robust else 0, _p(Tcw), _p(a["xw"]), _p(stop_arr), C.byref(stats))
    return rc, Tcw[:s.n_local], a["xw"], stats.as_dict()


def BundleAdjustment(problem, n_iterations=5, robust=True, stop=None):
    """Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (src/Optimizer.cc:41-237) on the host over a pack_lba_problem() dict
    gathered as :71-184 walks (the non-bad key frames as the "local" ones, local_fixed for mnId == 0) -> (0, Tcw float32 [n_local, 4,
    4], xw float32 [n_points, 3], stats dict: iterations, trials, lambda, chi2).  robust: Huber with sqrt(5.99) / sqrt(7.815), else no
    kernel.  stop (a uint8 [1], as pbStopFlag) is read at every iteration's top and in the trial loop; there is no entry check.  The
    reduced system is dense: the host path is meant for the initial map and for machines without a GPU."""
    rc, Tcw, xw, stats = _ba_call(lib().orbp_bundle_adjustment, problem, n_iterations, robust, stop)
    return _pchk(rc), Tcw, xw, stats


class EgProblem(C.Structure):
    """orbp_eg_problem (include/orbp.h)"""
    _fields_ = [("n_kfs", C.c_int32), ("Scw", C.c_void_p), ("Snc", C.c_void_p), ("fixed", C.c_int32), ("fix_scale", C.c_int32),
                ("n_edges", C.c_int32), ("edge_i", C.c_void_p), ("edge_j", C.c_void_p), ("edge_corrected", C.c_void_p),
                ("n_points", C.c_int32), ("ref", C.c_void_p)]


class EgStats(C.Structure):
    """orbp_eg_stats (include/orbp.h)"""
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("lambda_", C.c_double), ("chi2_initial", C.c_double),
                ("chi2_final", C.c_double)]

    def as_dict(self):
        return {"iterations": self.iterations, "trials": self.trials, "lambda": self.lambda_, "chi2_initial": self.chi2_initial,
                "chi2_final": self.chi2_final}


ORBM_EG_MAX_KFS = 438


def pack_eg_problem(problem):
    """The flat arrays of orbp_optimize_essential_graph / orbm_optimize_essential_graph from a dict gathered as
    Optimizer::OptimizeEssentialGraph walks (src/Optimizer.cc:797-983): Scw float64 [n_kfs, 8] in Sim3::operator[] order (qx qy qz
    qw tx ty tz s), Snc the same (absent: a copy of Scw), fixed (an index or -1), fix_scale; per edge edge_i, edge_j int32 and
    edge_corrected uint8; xw float32 [n_points, 3] and ref int32 [n_points] (-1: leave the point alone).  -> (EgProblem, arrays):
    the struct points into `arrays` (a dict of contiguous copies, xw among them), which must outlive it."""
    a = {"Scw": np.ascontiguousarray(problem["Scw"], np.float64).reshape(-1, 8),
         "edge_i": np.ascontiguousarray(problem["edge_i"], np.int32).reshape(-1),
         "edge_j": np.ascontiguousarray(problem["edge_j"], np.int32).reshape(-1),
         "edge_corrected": np.ascontiguousarray(problem["edge_corrected"], np.uint8).reshape(-1),
         "xw": np.array(problem.get("xw", np.zeros((0, 3))), np.float32).reshape(-1, 3),
         "ref": np.ascontiguousarray(problem.get("ref", np.zeros(0)), np.int32).reshape(-1)}
    a["Snc"] = np.ascontiguousarray(problem["Snc"] if problem.get("Snc") is not None else a["Scw"], np.float64).reshape(-1, 8)
    if len(a["Snc"]) != len(a["Scw"]) or not (len(a["edge_i"]) == len(a["edge_j"]) == len(a["edge_corrected"])) or len(a["ref"]) != len(a["xw"]):
        raise OrbxError(ORBX_E_INVALID, "pack_eg_problem: array lengths disagree")
    ptr = {k: (v.ctypes.data if v.size else None) for k, v in a.items()}
    s = EgProblem(len(a["Scw"]), ptr["Scw"], ptr["Snc"], int(problem.get("fixed", -1)), 1 if problem.get("fix_scale") else 0,
                  len(a["edge_i"]), ptr["edge_i"], ptr["edge_j"], ptr["edge_corrected"], len(a["xw"]), ptr["ref"])
    return s, a


def _eg_call(fn, problem, n_iterations):
    s, a = pack_eg_problem(problem)
    Tcw = np.zeros((max(s.n_kfs, 1), 4, 4), np.float32)
    Scw = np.zeros((max(s.n_kfs, 1), 8), np.float64)
    stats = EgStats()
    rc = fn(C.byref(s), int(n_iterations), _p(Tcw), _p(a["xw"]), _p(Scw), C.byref(stats))
    return rc, Tcw[:s.n_kfs], a["xw"], Scw[:s.n_kfs], stats.as_dict()


def optimize_essential_graph(problem, n_iterations=20):
    """Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044) on the host over a pack_eg_problem() dict -> (0, Tcw float32
    [n_kfs, 4, 4] = [R | t / s], xw float32 [n_points, 3], Scw float64 [n_kfs, 8] = the optimised Sim3, stats dict: iterations,
    trials, lambda, chi2_initial, chi2_final).  The 7N x 7N system is an envelope Cholesky: there is no cap on n_kfs."""
    rc, Tcw, xw, Scw, stats = _eg_call(lib().orbp_optimize_essential_graph, problem, n_iterations)
    return _pchk(rc), Tcw, xw, Scw, stats
