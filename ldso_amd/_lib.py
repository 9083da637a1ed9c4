"""ctypes bindings of the C ABI in include/ldso_ba.h.

The product path is the HIP library ``ldso_amd/lib/libldso_ba.so`` (built in-tree by
``__graft_entry__.build()``).  There is no CPU fallback: if the library is missing the import
fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.environ.get("LDSO_BA_LIB") or os.path.join(LIB_DIR, "libldso_ba.so")  # override: A/B builds only
SYNTH_PATH = os.path.join(LIB_DIR, "libldso_synth.so")

PATTERN_NUM = 8
CPARS = 4
MAX_FRAMES = 16
PRECALC_STRIDE = 48
POINT_STRIDE = 24
RES_IN, RES_OOB, RES_OUTLIER = 0, 1, 2
FLAG_ACTIVE, FLAG_NEW = 1, 2

i32p = C.POINTER(C.c_int32)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
i8p = C.POINTER(C.c_int8)
u8p = C.POINTER(C.c_uint8)
i64p = C.POINTER(C.c_int64)

FRAME_STATE_DTYPE = np.dtype(
    [
        ("world_to_cam_evalpt", np.float64, (12,)),
        ("state", np.float64, (10,)),
        ("state_zero", np.float64, (10,)),
        ("ab_exposure", np.float64),
        ("is_first_frame", np.int32),
        ("pad_", np.int32),
    ],
    align=True,
)
assert FRAME_STATE_DTYPE.itemsize == 272


ABI_VERSION = 7

# setting_solverMode bits (Settings.h:14-25) and ldso_ba_optimize's per-window outcome
SOLVER_SVD, SOLVER_ORTHOGONALIZE_SYSTEM, SOLVER_ORTHOGONALIZE_POINTMARG, SOLVER_ORTHOGONALIZE_FULL = 1, 2, 4, 8
SOLVER_SVD_CUT7, SOLVER_REMOVE_POSEPRIOR, SOLVER_USE_GN, SOLVER_FIX_LAMBDA = 16, 32, 64, 128
SOLVER_ORTHOGONALIZE_X, SOLVER_MOMENTUM, SOLVER_STEPMOMENTUM, SOLVER_ORTHOGONALIZE_X_LATER = 256, 512, 1024, 2048
SOLVER_DEFAULT = SOLVER_FIX_LAMBDA | SOLVER_ORTHOGONALIZE_X_LATER
OPT_RAN_ALL, OPT_CONVERGED, OPT_LOST = 0, 1, 2


class OptSettings(C.Structure):
    """ldso_ba_opt_settings: setting_solverMode, setting_forceAceptStep, setting_minOptIterations,
    setting_thOptIterations, setting_affineOptModeA / B, setting_vi_enable (Setting.cc:23, 36-38, 65-66,
    73, 152)."""
    _fields_ = [("solver_mode", C.c_int32), ("force_accept_step", C.c_int32), ("min_opt_iterations", C.c_int32),
                ("th_opt_iterations", C.c_float), ("affine_opt_mode_a", C.c_float), ("affine_opt_mode_b", C.c_float),
                ("vi_enable", C.c_int32), ("reserved_", C.c_int32)]

    @classmethod
    def default(cls, **kw):
        s = cls(SOLVER_DEFAULT, 1, 1, 1.2, 1e12, 1e8, 0, 0)
        for k, v in kw.items():
            setattr(s, k, v)
        return s


# setting_affineOptModeA / B of the reference's drivers (the library default is Setting.cc:65-66)
AFFINE_MODES = {
    "default": (1e12, 1e8),     # Setting.cc:65-66
    "kitti_euroc": (0.0, 0.0),  # run_dso_kitti.cc:299-300, run_dso_euroc.cc:291-292, TUM-Mono mode 1
    "fixed": (-1.0, -1.0),      # run_dso_tum_mono.cc:291-292 (mode 2: a and b fixed)
}


class LdsoBaWindow(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int32),
        ("n_points", C.c_int32),
        ("n_residuals", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("calib", C.c_float * 4),
        ("dI", f32p),
        ("frame_energy_th", f32p),
        ("precalc", f32p),
        ("ad_host", f64p),
        ("ad_target", f64p),
        ("c_prior", f64p),
        ("c_delta", f32p),
        ("frame_prior", f64p),
        ("frame_delta_prior", f64p),
        ("point_host", i32p),
        ("point_data", f32p),
        ("point_res_begin", i32p),
        ("res_target", i32p),
        ("res_state", i8p),
        ("res_energy", f32p),
        ("res_flags", u8p),
        ("point_rank", i32p),
    ]


class LdsoBaEdit(C.Structure):
    """ldso_ba_edit (include/ldso_ba.h)"""
    _fields_ = [("after", C.POINTER(LdsoBaWindow)), ("frame_ids", i64p), ("frame_src", i32p), ("point_src", i32p),
                ("res_src", i32p)]


# Point::PointStatus as ldso_ba_flag_points leaves it (LDSO_BA_PT_*)
PT_ACTIVE, PT_OUTLIER, PT_OUT, PT_MARGINALIZED = 0, 1, 2, 3


class FlagParams(C.Structure):
    """ldso_ba_flag_params: setting_minGoodActiveResForMarg, setting_minGoodResForMarg,
    setting_minIdepthH_marg (Setting.cc: 3, 4, 50)."""
    _fields_ = [("min_good_active_res_for_marg", C.c_int32), ("min_good_res_for_marg", C.c_int32),
                ("min_idepth_h_marg", C.c_float), ("reserved_", C.c_int32)]

    @classmethod
    def default(cls, **kw):
        s = cls()
        lib().ldso_ba_default_flag_params(C.byref(s))
        for k, v in kw.items():
            setattr(s, k, v)
        return s


def source_sha256() -> str | None:
    """sha256 over the sources libldso_ba.so is built from (ldso_amd/csrc, include/ldso_ba.h,
    include/ldso_ct.h, include/ldso_lc.h): the identity of a build that survives a rebuild on another machine (the .so
    bytes do not)."""
    import glob
    import hashlib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "ldso_amd", "csrc", "*.hip")) +
                   glob.glob(os.path.join(root, "ldso_amd", "csrc", "*.h")) +
                   glob.glob(os.path.join(root, "ldso_amd", "csrc", "*.cpp")) +
                   [os.path.join(root, "ldso_amd", "csrc", "Makefile"), os.path.join(root, "include", "ldso_ba.h"),
                    os.path.join(root, "include", "ldso_ct.h"), os.path.join(root, "include", "ldso_lc.h")])
    h = hashlib.sha256()
    try:
        for f in files:
            h.update(os.path.relpath(f, root).encode())
            with open(f, "rb") as fh:
                h.update(hashlib.sha256(fh.read()).digest())
    except OSError:
        return None
    return h.hexdigest()


def ptr(a, t):
    if a is None:
        return C.cast(None, t)
    assert a.flags["C_CONTIGUOUS"], "arrays handed to the C ABI must be C-contiguous"
    assert a.dtype == np.dtype(t._type_), f"array of {a.dtype} handed as {t.__name__}"
    return a.ctypes.data_as(t)


# (name, restype, argtypes) of every entry point declared in include/ldso_ba.h
ABI = [
    ("ldso_ba_abi_version", C.c_int, []),
    ("ldso_ba_last_error", C.c_char_p, []),
    ("ldso_ba_frame_precalc", C.c_int, [C.c_int32, C.c_void_p, f32p, f32p]),
    ("ldso_ba_set_adjoints", C.c_int, [C.c_int32, C.c_void_p, f64p, f64p, f64p]),
    ("ldso_ba_adjoints_diagonal", C.c_int, [C.c_int32, f64p]),
    ("ldso_ba_frame_take_data", C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, f64p, f64p, f64p]),
    ("ldso_ba_solve_system", C.c_int,
     [C.c_void_p, C.c_int32, C.c_int32, C.c_double, f64p, f64p, f64p, f64p, f64p, f64p, f64p, f64p, f64p, C.c_int32,
      f64p]),
    ("ldso_ba_nullspaces", C.c_int, [C.c_int32, C.c_void_p, f64p]),
    ("ldso_ba_validate_window", C.c_int, [C.POINTER(LdsoBaWindow)]),
    ("ldso_ba_create", C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    ("ldso_ba_destroy", None, [C.c_void_p]),
    ("ldso_ba_stream", C.c_void_p, [C.c_void_p]),
    ("ldso_ba_load", C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LdsoBaWindow), C.c_int32, C.c_int32]),
    ("ldso_ba_update", C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LdsoBaWindow)]),
    ("ldso_ba_reset_oob", C.c_int, [C.c_void_p, C.c_int32]),
    ("ldso_ba_update_points", C.c_int, [C.c_void_p, C.c_int32, f32p]),
    ("ldso_ba_update_residuals", C.c_int, [C.c_void_p, C.c_int32, i8p, f32p, f32p, u8p]),
    ("ldso_ba_linearize_residuals", C.c_int, [C.c_void_p, C.c_int32, i8p, f32p, f32p, f32p, u8p, f32p]),
    ("ldso_ba_linearize", C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    ("ldso_ba_sync", C.c_int, [C.c_void_p]),
    ("ldso_ba_get_energy", C.c_int, [C.c_void_p, C.c_int32, f64p]),
    ("ldso_ba_get_system", C.c_int, [C.c_void_p, C.c_int32, f64p, f64p, f64p, f64p, f64p, f64p]),
    ("ldso_ba_get_residuals", C.c_int, [C.c_void_p, C.c_int32, i8p, i8p, f32p, f32p, f32p, u8p, f32p, f32p]),
    ("ldso_ba_get_points", C.c_int, [C.c_void_p, C.c_int32, f32p, f32p, f32p, f32p, f32p, f32p]),
    ("ldso_ba_get_frame_energy_th", C.c_int, [C.c_void_p, C.c_int32, f32p]),
    ("ldso_ba_solve", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, f64p, C.c_int32, f64p]),
    ("ldso_ba_resubstitute", C.c_int, [C.c_void_p, C.c_int32, f64p, C.c_double, f32p]),
    ("ldso_ba_solve_device", C.c_int, [C.c_void_p, C.c_int32, C.c_double, f64p, C.c_int32, f64p]),
    ("ldso_ba_resubstitute_device", C.c_int, [C.c_void_p, C.c_double, f32p]),
    ("ldso_ba_iterate", C.c_int, [C.c_void_p, C.c_int32, C.c_double, f64p, C.c_int32, f64p, f32p, f64p]),
    ("ldso_ba_packed_system", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), i64p, i64p]),
    ("ldso_ba_unpack_system", C.c_int, [C.c_void_p]),
    ("ldso_ba_copy_packed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    ("ldso_ba_newest_stride", C.c_int, [C.c_void_p, i64p]),
    ("ldso_ba_export_newest", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("ldso_ba_frame_threshold_gathered", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]),
    ("ldso_ba_shard_points", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, i32p, i32p]),
    ("ldso_ba_pack_upper", C.c_int, [C.c_int32, f64p, f64p, f64p, f64p, f64p]),
    ("ldso_ba_unpack_upper", C.c_int, [C.c_int32, f64p, f64p, f64p, f64p, f64p]),
    ("ldso_ba_frame_threshold", C.c_int, [f32p, C.c_int64, f32p]),
    ("ldso_ba_comm_unique_id", C.c_int, [C.c_void_p]),
    ("ldso_ba_comm_init", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    ("ldso_ba_check_settings", C.c_int, [C.c_void_p]),
    ("ldso_ba_default_settings", None, [C.c_void_p]),
    ("ldso_ba_set_settings", C.c_int, [C.c_void_p, C.c_void_p]),
    ("ldso_ba_get_settings", C.c_int, [C.c_void_p, C.c_void_p]),
    ("ldso_ba_optimize", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, f64p, f64p, f64p, f64p, C.c_void_p,
                                   f64p, f32p, i32p, i32p]),
    ("ldso_ba_get_loop_state", C.c_int, [C.c_void_p, C.c_int32, f64p, f32p, f64p]),
    ("ldso_ba_frame_step", C.c_int, [C.c_int32, C.c_void_p, f64p, C.c_void_p, f64p, f64p, f32p, f32p]),
    ("ldso_ba_step_canbreak", C.c_int, [C.c_int32, f64p, C.c_float, C.c_float, C.c_float, i32p]),
    ("ldso_ba_set_kernel_timing", C.c_int, [C.c_void_p, C.c_int32]),
    ("ldso_ba_set_tuning", C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    ("ldso_ba_get_kernel_times", C.c_int, [C.c_void_p, f64p, i64p, C.c_int32]),
    ("ldso_ba_kernel_name", C.c_char_p, [C.c_int32]),
    ("ldso_ba_num_kernels", C.c_int32, []),
    ("ldso_ba_stats", C.c_int, [C.c_void_p, i64p, i64p, i64p]),
    ("ldso_ba_marginalize_frame", C.c_int, [C.c_int32, C.c_int32, f64p, f64p, f64p, f64p, f64p, f64p]),
    ("ldso_ba_ad_ht_delta", C.c_int, [C.c_int32, f64p, f64p, f64p, f32p]),
    ("ldso_ba_calc_m_energy", C.c_int, [C.c_int32, f64p, f64p, f32p, f64p, f64p]),
    ("ldso_ba_calc_l_energy", C.c_int, [C.c_int32, f64p, f64p, f64p, f32p, C.c_int32, f32p, f32p, f64p]),
    ("ldso_ba_load_marginalization", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(LdsoBaWindow)]),
    ("ldso_ba_marginalize_points", C.c_int, [C.c_void_p, f32p, f64p, f64p]),
    ("ldso_ba_activate_points", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    ("ldso_ba_activate_points_tracker", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    # device-resident frame store
    ("ldso_ba_frames_reserve", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    ("ldso_ba_frame_put", C.c_int, [C.c_void_p, C.c_int64, f32p]),
    ("ldso_ba_frame_put_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ldso_ba_frame_put_tracker", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    ("ldso_ba_frame_put_initializer", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    ("ldso_ba_frame_drop", C.c_int, [C.c_void_p, C.c_int64]),
    ("ldso_ba_frame_get", C.c_int, [C.c_void_p, C.c_int64, f32p, f32p]),
    ("ldso_ba_load_frames", C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LdsoBaWindow), i64p, C.c_int32, C.c_int32]),
    ("ldso_ba_transfer_stats", C.c_int, [C.c_void_p, i64p]),
    # editing a loaded window in place
    ("ldso_ba_edit_window", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    ("ldso_ba_get_point_data", C.c_int, [C.c_void_p, C.c_int32, f32p]),
    ("ldso_ba_edit_stats", C.c_int, [C.c_void_p, f64p]),
    ("ldso_ba_edit_plan_check", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, i32p, i32p, i32p, i32p, i32p,
                                          i32p, i32p]),
    # closing a keyframe on the device
    ("ldso_ba_default_flag_params", None, [C.c_void_p]),
    ("ldso_ba_flag_points", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, u8p, i32p, i32p, i8p, i8p, u8p, i32p, i8p, i32p]),
    ("ldso_ba_load_marginalization_device", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(LdsoBaWindow), C.c_int32, i32p, u8p]),
    ("ldso_ba_marg_plan_check", C.c_int, [C.c_void_p, C.c_int32, i32p, u8p, C.c_int32, C.c_int32, i32p, i32p, i32p, i32p]),
]
ERR_FRAME_STORE, ERR_GRADIENT_MISMATCH = -4, -5

f32pp = C.POINTER(f32p)

# ldso_ct_immature (include/ldso_ct.h): one ImmaturePoint, 128 bytes
IMMATURE_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("idepth_min", "<f4"), ("idepth_max", "<f4"),
                           ("quality", "<f4"), ("energy_th", "<f4"), ("color", "<f4", (8,)),
                           ("weights", "<f4", (8,)), ("grad_h", "<f4", (4,)), ("host", "<i4"),
                           ("last_status", "<i4"), ("last_uv", "<f4", (2,)), ("last_interval", "<f4"),
                           ("type", "<f4")])
assert IMMATURE_DTYPE.itemsize == 128
# ldso_ba_activation (include/ldso_ba.h)
ACTIVATION_DTYPE = np.dtype([("idepth", "<f4"), ("status", "<i4"), ("in_mask", "<u4"), ("energy", "<f4")])
IPS_NAMES = ("GOOD", "OOB", "OUTLIER", "SKIPPED", "BADCONDITION", "UNINITIALIZED")  # ImmaturePoint.h:31-38



class LdsoCtSelectParams(C.Structure):
    """ldso_ct_select_params (include/ldso_ct.h)"""
    _fields_ = [("density", C.c_float), ("recursions", C.c_int32), ("th_factor", C.c_float),
                ("min_grad_hist_cut", C.c_float), ("min_grad_hist_add", C.c_float),
                ("grad_downweight_per_level", C.c_float), ("select_direction_distribution", C.c_int32)]


class LdsoCtTrackParams(C.Structure):
    """ldso_ct_track_params (include/ldso_ct.h)"""
    _fields_ = [("coarse_cutoff_th", C.c_float), ("lambda_increase", C.c_double), ("lambda_decrease", C.c_double),
                ("affine_opt_mode_a", C.c_float), ("affine_opt_mode_b", C.c_float), ("max_iterations", C.c_int32 * 5),
                ("solve", C.c_int32)]


class LdsoCtActselParams(C.Structure):
    """ldso_ct_actsel_params (include/ldso_ct.h); the defaults are LDSO_CT_ACTSEL_PARAMS_INIT"""
    _fields_ = [("current_min_act_dist", C.c_float), ("min_trace_quality", C.c_float), ("newest_host", C.c_int32)]


ACT_KEEP, ACT_DELETE, ACT_OPTIMIZE = 0, 1, 2  # LDSO_CT_ACT_*
ACTSEL_COUNTS = ("kept", "deleted", "selected", "rejected_by_distance")
TRACK_SOLVE_FULL, TRACK_SOLVE_REFERENCE = 0, 1  # LDSO_CT_TRACK_SOLVE_*
# ldso_ct_track_result / ldso_ct_track_step (include/ldso_ct.h)
TRACK_RESULT_DTYPE = np.dtype([("ref_to_new", "<f8", (12,)), ("aff", "<f8", (2,)), ("last_residuals", "<f8", (5,)),
                               ("flow", "<f8", (3,)), ("ok", "<i4"), ("reason", "<i4"), ("abort_level", "<i4"),
                               ("iterations", "<i4", (5,)), ("repeated_level", "<i4")], align=True)
TRACK_STEP_DTYPE = np.dtype([("lvl", "<i4"), ("iteration", "<i4"), ("accepted", "<i4"), ("cutoff_th", "<f4"),
                             ("lambda", "<f8"), ("pose", "<f8", (12,)), ("aff", "<f8", (2,)), ("rs", "<f8", (6,)),
                             ("inc", "<f8", (8,))], align=True)
assert TRACK_RESULT_DTYPE.itemsize == 216 and TRACK_STEP_DTYPE.itemsize == 248 and C.sizeof(LdsoCtTrackParams) == 56

SELECT_STATS = ("num", "n2", "n3", "n4", "potential_used", "potential_next", "passes")  # LDSO_CT_SELECT_STATS
# ldso_ct_feature (include/ldso_ct.h): what DetectCorners leaves on a Feature, 48 bytes
FEATURE_DTYPE = np.dtype([("score", "<f4"), ("angle", "<f4"), ("is_corner", "<i4"), ("level", "<i4"),
                          ("descriptor", "u1", (32,))])
assert FEATURE_DTYPE.itemsize == 48
CORNER_STATS = ("gridsize", "k", "candidates", "features", "corners", "max_score_bits")  # LDSO_CT_CORNER_STATS



class LdsoCtInitParams(C.Structure):
    """ldso_ct_init_params (include/ldso_ct.h)"""
    _fields_ = [("alpha_k", C.c_float), ("alpha_w", C.c_float), ("reg_weight", C.c_float),
                ("coupling_weight", C.c_float), ("max_iterations", C.c_int32 * 5), ("fix_affine", C.c_int32),
                ("huber_th", C.c_float)]


class LdsoCtUndistortDesc(C.Structure):
    """ldso_ct_undistort_desc (include/ldso_ct.h)"""
    _fields_ = [("w_org", C.c_int32), ("h_org", C.c_int32), ("remap_x", f32p), ("remap_y", f32p), ("g", f32p),
                ("g_depth", C.c_int32), ("vignette_inv", f32p), ("photometric_mode", C.c_int32),
                ("use_exposure", C.c_int32)]


UNDISTORT_MODELS = ("fov", "radtan", "equidistant", "kannala_brandt", "pinhole")  # LDSO_CT_UNDISTORT_*
UNDISTORT_OUT = ("crop", "none", "calib", "full")  # LDSO_CT_UNDISTORT_OUT_*

# ldso_ct_init_point / _result / _step (include/ldso_ct.h): the coarse initializer's records
INIT_POINT_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("idepth", "<f4"), ("ir", "<f4"), ("idepth_new", "<f4"),
                             ("energy", "<f4", (2,)), ("energy_new", "<f4", (2,)), ("last_hessian", "<f4"),
                             ("last_hessian_new", "<f4"), ("maxstep", "<f4"), ("outlier_th", "<f4"),
                             ("my_type", "<f4"), ("ir_sum_num", "<f4"), ("is_good", "<i4"), ("is_good_new", "<i4"),
                             ("parent", "<i4"), ("neighbours", "<i4", (10,))])
INIT_RESULT_DTYPE = np.dtype([("this_to_next", "<f8", (12,)), ("this_to_next_aff", "<f8", (2,)),
                              ("latest_res", "<f4", (3,)), ("snapped", "<i4"), ("frame_id", "<i4"),
                              ("snapped_at", "<i4"), ("ret", "<i4"), ("iterations", "<i4", (5,)),
                              ("phase_us", "<f4", (4,))], align=True)
INIT_PHASES = ("evaluations", "rank_sweeps", "point_phases", "lane0")  # ldso_ct_init_result.phase_us
INIT_STEP_DTYPE = np.dtype([("pose", "<f8", (12,)), ("aff", "<f8", (2,)), ("lvl", "<i4"), ("iteration", "<i4"),
                            ("accepted", "<i4"), ("alpha_capped", "<i4"), ("snapped", "<i4"), ("lambda", "<f4"),
                            ("inc", "<f4", (8,)), ("res", "<f4", (3,)), ("reg_energy", "<f4", (3,))], align=True)
assert INIT_POINT_DTYPE.itemsize == 112 and INIT_RESULT_DTYPE.itemsize == 176 and INIT_STEP_DTYPE.itemsize == 192
assert C.sizeof(LdsoCtInitParams) == 44
init_point_pp = C.POINTER(C.c_void_p)

# (name, restype, argtypes) of every entry point declared in include/ldso_ct.h (coarse tracker)
CT_ABI = [
    ("ldso_ct_create", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), i32p]),
    ("ldso_ct_destroy", None, [C.c_void_p]),
    ("ldso_ct_make_k", C.c_int, [C.c_void_p, f32p, f32p]),
    ("ldso_ct_set_new_frame", C.c_int, [C.c_void_p, f32p, C.c_double, f32p]),
    ("ldso_ct_get_frame_level", C.c_int, [C.c_void_p, C.c_int32, f32p, f32p]),
    ("ldso_ct_set_reference", C.c_int,
     [C.c_void_p, i32p, f32pp, f32pp, f32pp, f32pp, C.c_double, C.c_double, C.c_double]),
    ("ldso_ct_make_reference", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_int32, f32p, f32p, C.c_double, C.c_double, C.c_double, i32p]),
    ("ldso_ct_make_reference_ba", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, i32p]),
    ("ldso_ct_get_reference", C.c_int, [C.c_void_p, C.c_int32, i32p, f32p, C.c_int32]),
    ("ldso_ct_calc_res", C.c_int, [C.c_void_p, C.c_int32, f64p, C.c_double, C.c_double, C.c_float, f64p]),
    ("ldso_ct_calc_res_batch", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, f64p, f64p, C.c_float, f64p]),
    ("ldso_ct_calc_gs", C.c_int, [C.c_void_p, C.c_int32, f64p, C.c_double, C.c_double, f64p, f64p]),
    ("ldso_ct_calc_res_gs", C.c_int,
     [C.c_void_p, C.c_int32, f64p, C.c_double, C.c_double, C.c_float, f64p, f64p, f64p]),
    ("ldso_ct_get_warped", C.c_int, [C.c_void_p, i32p, f32p, C.c_int32]),
    ("ldso_ct_track_default_params", None, [C.c_void_p]),
    ("ldso_ct_track", C.c_int, [C.c_void_p, C.c_int32, f64p, f64p, C.c_int32, f64p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int32, i32p]),
    ("ldso_ct_lm_step", C.c_int, [f64p, f64p, C.c_double, f64p, f64p, C.c_void_p, f64p, f64p, f64p]),
    ("ldso_ct_make_immature", C.c_int, [C.c_void_p, C.c_int32, f32p, C.c_float, C.c_int32, C.c_void_p]),
    ("ldso_ct_immature_upload", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    ("ldso_ct_immature_download", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    ("ldso_ct_trace", C.c_int, [C.c_void_p, C.c_int32, f32p, f32p, f32p, i32p]),
    ("ldso_ct_make_distance_map", C.c_int, [C.c_void_p, C.c_int32, f32p, f32p, C.c_int32, f32p, i32p, f32p]),
    ("ldso_ct_make_distance_map_ba", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, f32p, f32p, f32p]),
    ("ldso_ct_select_activation", C.c_int, [C.c_void_p, C.c_void_p, u8p, C.c_int32, i32p, i32p, i32p, i32p]),
    ("ldso_ct_selection_download", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    ("ldso_ct_immature_append", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    ("ldso_ct_select_default_params", None, [C.c_void_p]),
    ("ldso_ct_select_init", C.c_int, [C.c_void_p, u8p, C.c_int32]),
    ("ldso_ct_select_potential", C.c_int, [C.c_void_p, i32p]),
    ("ldso_ct_select_pixels", C.c_int, [C.c_void_p, C.c_void_p, f32p, i32p]),
    ("ldso_ct_make_new_traces", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, i32p, i32p]),
    ("ldso_ct_corners_init", C.c_int, [C.c_void_p, i32p]),
    ("ldso_ct_detect_corners", C.c_int,
     [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, i32p, i32p]),
    ("ldso_ct_init_default_params", None, [C.c_void_p]),
    ("ldso_ct_init_check_points", C.c_int, [C.c_int32, C.c_int32, C.c_int32, i32p, init_point_pp]),
    ("ldso_ct_init_set_first", C.c_int, [C.c_void_p, i32p, init_point_pp]),
    ("ldso_ct_init_get_points", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, i32p]),
    ("ldso_ct_init_set_points", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ("ldso_ct_init_eval", C.c_int, [C.c_void_p, C.c_int32, f64p, f64p, C.c_void_p, f32p, f32p, f32p, f32p, f32p, i32p]),
    ("ldso_ct_init_lm_step", C.c_int, [f32p, f32p, f32p, f32p, C.c_float, C.c_int32, C.c_int32, f64p, f64p,
                                       C.c_void_p, f32p, f64p, f64p]),
    ("ldso_ct_init_opt_reg", C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_int32]),
    ("ldso_ct_init_track_frame", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, i32p]),
    ("ldso_ct_init_rank_counts", C.c_int, [C.c_void_p, i32p]),
    ("ldso_ct_undistort_init", C.c_int, [C.c_void_p, C.c_void_p, i32p]),
    ("ldso_ct_set_new_frame_raw", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, f32p, f32p]),
    ("ldso_ct_set_new_frame_raw_device", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, f32p, C.c_void_p, f32p]),
    ("ldso_ct_get_undistorted", C.c_int, [C.c_void_p, f32p]),
    ("ldso_ct_undistort_make_remap", C.c_int, [C.c_int32, f64p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               f32p, f64p, f32p, f32p, i32p]),
    ("ldso_ct_undistort_make_photometric", C.c_int, [f32p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                     f32p, f32p]),
    ("ldso_ct_set_kernel_timing", C.c_int, [C.c_void_p, C.c_int32]),
    ("ldso_ct_get_kernel_times", C.c_int, [C.c_void_p, f64p, i64p, C.c_int32]),
    ("ldso_ct_kernel_name", C.c_char_p, [C.c_int32]),
    ("ldso_ct_num_kernels", C.c_int32, []),
]

# ldso_lc_feature / _match / _projection (include/ldso_lc.h): the loop closer's records
LC_ABI_VERSION = 1
LC_FEATURE_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("angle", "<f4"), ("inv_d", "<f4"), ("is_corner", "<i4"),
                             ("usable", "<i4"), ("descriptor", "u1", (32,))])
LC_MATCH_DTYPE = np.dtype([("index1", "<i4"), ("index2", "<i4"), ("dist", "<i4")])
LC_PROJECTION_DTYPE = np.dtype([("index_cand", "<i4"), ("index_cur", "<i4"), ("dist", "<i4"), ("reserved_", "<i4"),
                                ("p_ref", "<f8", (3,)), ("p_curr", "<f8", (3,)), ("pixel", "<f8", (2,))])
assert LC_FEATURE_DTYPE.itemsize == 56 and LC_MATCH_DTYPE.itemsize == 12 and LC_PROJECTION_DTYPE.itemsize == 80

# (name, restype, argtypes) of every entry point declared in include/ldso_lc.h (loop closing's matching)
LC_ABI = [
    ("ldso_lc_abi_version", C.c_int, []),
    ("ldso_lc_create", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ("ldso_lc_destroy", None, [C.c_void_p]),
    ("ldso_lc_keyframe_put", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    ("ldso_lc_keyframe_put_tracker", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    ("ldso_lc_keyframe_update", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, f32p, i32p]),
    ("ldso_lc_keyframe_set_bow", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, i32p, i32p, i32p]),
    ("ldso_lc_keyframe_get", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, i32p]),
    ("ldso_lc_keyframe_drop", C.c_int, [C.c_void_p, C.c_int64]),
    ("ldso_lc_search_brute_force", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, i32p]),
    ("ldso_lc_search_brute_force_many", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, i64p, C.c_int32, i32p, i32p, i32p]),
    ("ldso_lc_search_by_bow", C.c_int,
     [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_int32, C.c_void_p, i32p]),
    ("ldso_lc_make_idepth_map_ba", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, f32p]),
    ("ldso_lc_make_idepth_map", C.c_int, [C.c_void_p, C.c_int32, f32p]),
    ("ldso_lc_get_idepth_map", C.c_int, [C.c_void_p, f32p]),
    ("ldso_lc_search_by_projection", C.c_int,
     [C.c_void_p, C.c_int64, C.c_int64, f32p, f64p, C.c_float, C.c_int32, C.c_int32, C.c_void_p, i32p]),
]

_lib = None
_synth = None


def lib():
    """The product library.  Raises if it has not been built (no fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C ldso_amd/csrc). The HIP path has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, res, args in ABI + CT_ABI + LC_ABI:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        if L.ldso_ba_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI {L.ldso_ba_abi_version()}, these bindings expect {ABI_VERSION}: "
                               "rebuild it (make -C ldso_amd/csrc)")
        if L.ldso_lc_abi_version() != LC_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has loop-closing ABI {L.ldso_lc_abi_version()}, these bindings expect "
                               f"{LC_ABI_VERSION}: rebuild it (make -C ldso_amd/csrc)")
        _lib = L
    return _lib


class LdsoError(RuntimeError):
    """A negative return of the C ABI; ``code`` is that return."""

    def __init__(self, code, msg):
        super().__init__(f"ldso_ba error {code}: {msg}")
        self.code = int(code)


def check(rc):
    if rc != 0:
        raise LdsoError(rc, lib().ldso_ba_last_error().decode())
    return rc


def synth_lib():
    global _synth
    if _synth is None:
        if not os.path.exists(SYNTH_PATH):
            raise RuntimeError(f"{SYNTH_PATH} missing: run make -C ldso_amd/csrc")
        S = C.CDLL(SYNTH_PATH)
        S.ldso_synth_fill.restype = C.c_int
        S.ldso_synth_fill.argtypes = [C.c_void_p, C.c_void_p, f32p, f32p, f32p, i32p, f32p, i32p, i32p, i8p, f32p, u8p]
        _synth = S
    return _synth
