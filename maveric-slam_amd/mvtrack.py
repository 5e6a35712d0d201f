"""mvtrack -- Python front-end over libmaveric_hip.so (the C ABI of include/*.h).

The product is the C/HIP library; this module only marshals numpy arrays and
torch device tensors into it (ctypes), for tests, smoke() and bench.py.
It never computes anything itself and never falls back to the CPU: if the
library or a gfx950 device is missing, every call raises.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MV_LIB: an alternate in-tree build of the same library (a tracing or A/B variant built on the
# CPU by tools/build_variant.sh); the default is the shipping build
LIB_PATH = os.environ.get("MV_LIB") or os.path.join(HERE, "libmaveric_hip.so")
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")

MV_OK = 0
MV_ERR_INVALID_ARG = -1
MV_ERR_CAPACITY = -2
MV_ERR_HIP = -3
MV_ERR_NO_DEVICE = -4
MV_ERR_NO_POINTS = -5
MV_ERR_OUT_OF_MEMORY = -6
MV_ERR_DEGENERATE = -7
MV_ERR_IO = -8
AS_BUILT = 0
AS_INTENDED = 1

_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float
_D = ctypes.c_double


SCREENS = {"i8": 0, "f16": 1, "i8s": 2}  # mv_allpairs_screen (i8s: int8 against a staged image)


class MVError(RuntimeError):
    pass


class WindowParams(ctypes.Structure):
    _fields_ = [("shift_x", _I), ("shift_y", _I), ("radius", _I), ("max_matches", _I), ("semantics", _I),
                ("match_thresh_sq", _D), ("prob_thresh", _D)]


class PoseParams(ctypes.Structure):
    _fields_ = [("fx", _F), ("fy", _F), ("cx", _F), ("cy", _F), ("semantics", _I), ("hypotheses", _I),
                ("inlier_thresh", _F), ("refine_iters", _I), ("seed", ctypes.c_ulonglong)]


class KpParams(ctypes.Structure):
    _fields_ = [("conf_thresh", _F), ("nms_dist", _I), ("border", _I)]


class SpLayer(ctypes.Structure):
    _fields_ = [("w", _P), ("bias", _P), ("cin", _I), ("cout", _I), ("k", _I), ("w_scale", _D), ("out_scale", _D)]


class SpWeights(ctypes.Structure):
    _fields_ = [("in_scale", _D), ("layer", SpLayer * 12)]


class TrackParams(ctypes.Structure):
    _fields_ = [("window", WindowParams), ("pose", PoseParams), ("top_n", _I), ("valid_cap", _I)]


class LandmarkParams(ctypes.Structure):
    """mv_landmark_params (include/feature_tracks.h)."""
    _fields_ = [("cos_min_parallax", _D), ("min_depth", _D), ("max_reproj_px", _D)]


class BaParams(ctypes.Structure):
    """mv_ba_params (include/bundle_adjust.h)."""
    _fields_ = [("max_iters", _I), ("lambda_init", _D), ("lambda_up", _D), ("lambda_down", _D), ("lambda_min", _D),
                ("lambda_max", _D), ("diag_floor", _D), ("rel_tol", _D), ("huber_px", _D)]


class PgParams(ctypes.Structure):
    """mv_pg_params (include/pose_graph.h)."""
    _fields_ = [("max_iters", _I), ("lambda_init", _D), ("lambda_up", _D), ("lambda_down", _D), ("lambda_min", _D),
                ("lambda_max", _D), ("diag_floor", _D), ("rel_tol", _D), ("huber", _D)]


class PnpParams(ctypes.Structure):
    """mv_pnp_params (include/absolute_pose.h)."""
    _fields_ = [("hypotheses", _I), ("refine_rounds", _I), ("min_inliers", _I), ("max_iters", _I),
                ("seed", ctypes.c_ulonglong), ("inlier_thresh_px", _D), ("min_depth", _D), ("lambda_init", _D),
                ("lambda_up", _D), ("lambda_down", _D), ("lambda_min", _D), ("lambda_max", _D), ("diag_floor", _D),
                ("rel_tol", _D), ("huber_px", _D)]


class BaWindowParams(ctypes.Structure):
    """mv_ba_window_params (include/ba_window.h)."""
    _fields_ = [("min_shared", _I), ("n_fixed", _I), ("min_obs", _I)]


class MapParams(ctypes.Structure):
    """mv_map_params (include/map_match.h)."""
    _fields_ = [("radius_px", _D), ("min_depth", _D), ("thresh", _D), ("ratio", _D), ("width", _I), ("height", _I)]


class MapCorrectParams(ctypes.Structure):
    """mv_map_correct_params (include/map_correct.h)."""
    _fields_ = [("split_rel", _D)]


class MapCullParams(ctypes.Structure):
    """mv_map_cull_params (include/map_cull.h)."""
    _fields_ = [("max_reproj_px", _D), ("min_depth", _D), ("worst_only", _I), ("min_obs", _I), ("stale_age", _I),
                ("stale_min_obs", _I), ("min_views", _I), ("redundant_num", _I), ("redundant_den", _I)]


BA_MAX_POSES = 16  # MV_BA_MAX_POSES
PNP_MAX_CAP = 1024  # MV_PNP_MAX_CAP
PG_MAX_NODES = 512  # MV_PG_MAX_NODES
PG_EDGE_SE3, PG_EDGE_DIRECTION = 0, 1
LDMK_LOW_PARALLAX, LDMK_BEHIND, LDMK_REPROJ, LDMK_DEGENERATE = 1, 2, 4, 8
TRACKS_MAX_CAP = 8192  # MV_TRACKS_MAX_CAP


def build(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-s", "-C", CSRC, "-j8"]
    if force:
        subprocess.run(["make", "-s", "-C", CSRC, "clean"], check=True)
    subprocess.run(cmd, check=True)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        # PyTorch-ROCm bundles its own libamdhip64 (same SONAME, different file name in
        # its NEEDED entries).  Load it first so this library binds to the SAME HIP
        # runtime; loading ours first would make torch pull in a second runtime copy.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        sig = {
            "mv_version": (_I, []),
            "mv_status_string": (ctypes.c_char_p, [_I]),
            "mv_last_status": (_I, []),
            "mv_last_error_message": (ctypes.c_char_p, []),
            "mv_device_count": (_I, []),
            "mv_context_create": (_I, [_I, ctypes.POINTER(_P)]),
            "mv_context_destroy": (_I, [_P]),
            "mv_context_set_stream": (_I, [_P, _P]),
            "mv_context_use_own_stream": (_I, [_P]),
            "mv_context_set_allpairs_screen": (_I, [_P, _I]),
            "mv_context_allpairs_screen": (_I, [_P]),
            "mv_context_stream": (_P, [_P]),
            "mv_context_synchronize": (_I, [_P]),
            "mv_context_reserve": (_I, [_P, _I, _I]),
            "mv_default_context": (_P, []),
            "mv_profile_enable": (_I, [_I]),
            "mv_profile_query": (_I, [ctypes.c_char_p, ctypes.POINTER(_D), ctypes.POINTER(_I)]),
            "mv_window_params_default": (None, [_P]),
            "mv_pose_params_default": (None, [_P, _I]),
            "mv_track_params_default": (None, [_P, _I]),
            "mv_scale_as_built": (_F, [_F]),
            "mv_softmax_host": (_I, [_P, _F, _P, _I, _P, _P, _P]),
            "mv_top_n_host": (_I, [_P, _F, _P, _I, _I, _I, _P, _P, _P, _P]),
            "mv_window_match_host": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
            "mv_softmax_batch_dev": (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
            "mv_top_n_select_batch_dev": (_I, [_P, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
            "mv_window_match_batch_dev": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P,
                                               _P]),
            "mv_match_allpairs_f32_dev": (_I, [_P, _I, _I, _P, _P, _P, _P, _D, _P, _P]),
            "mv_match_allpairs_f32_prepare_dev": (_I, [_P, _I, _I, _P, _P]),
            "mv_match_allpairs_f32_run_dev": (_I, [_P, _I, _I, _P, _P, _P, _P, _D, _P, _P]),
            "mv_match_allpairs_f32_run_prepare_dev": (_I, [_P, _I, _I, _P, _P, _P, _P, _D, _P, _P, _I, _I, _P, _P]),
            "mv_match_sequence_f32_dev": (_I, [_P, _I, _I, _P, _P, _D, _P, _P]),
            "mv_match_sequence_f32_run_prepare_dev": (_I, [_P, _I, _I, _P, _P, _D, _P, _P, _I, _I, _P, _P]),
            "mv_match_allpairs_i8_dev": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P]),
            "mv_match_two_way_f32_dev": (_I, [_P, _I, _I, _P, _P, _P, _P, _D, _P, _P]),
            "mv_run_nms_batch_dev": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
            "mv_projection_factors_dev": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
            "mv_pose_normal_equations_dev": (_I, [_P, _I, _P, _P, _P, _P, _P]),
            "mv_lba_schur_dev": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
            "mv_pose_batch_dev": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
            "mv_superpoint_create": (_I, [_P, _P, ctypes.POINTER(_P)]),
            "mv_superpoint_destroy": (_I, [_P]),
            "mv_superpoint_forward_dev": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
            "mv_superpoint_forward_raw_dev": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
            "mv_pose_from_matches_dev": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
            "mv_ransac_stub_host": (_I, [_P, _I, _P, _P, _F, _P, _P, _P]),
            "mv_recover_pose_host": (_I, [_P, _P, _P, _P, _P]),
            "mv_svd3_host": (_I, [_P, _P, _P, _P, _P]),
            "mv_track_pair_host": (_I, [_P, _P, _I, _I, _F, _P, _P, _F, _P, _P, _P, _P, _P, _P]),
            "compute_top_N": (None, [_F, _P, _I, _P, _P, _P, _P]),
            "compute_softmax": (None, [_F, _P, _P, _P, _P]),
            "normalize_points": (None, [_I, _P, _P, _P]),
            "compute_essential_matrix": (None, [_I, _P, _P, _P]),
            "compute_reprojection_error": (_F, [_P, _P, _P]),
            "ransac_essential_matrix": (None, [_I, _P, _P, _P, _I, _F, _P, _P, _P]),
            "recover_pose_from_essential_matrix": (None, [_P, _P, _P, _P]),
            "track": (_I, [_P, _P, _I, _I, _I, _F, _P]),
            "mv_kp_params_default": (None, [_P]),
            "mv_keypoints_dev": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
            "mv_keypoints_host": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P]),
            "mv_trajectory_chain_dev": (_I, [_P, _I, _I, _P, _P, _P, _I, _P]),
            "mv_trajectory_rebase_dev": (_I, [_P, _I, _I, _P, _I, _P]),
            "mv_trajectory_chain_host": (_I, [_P, _I, _P, _P, _P, _I, _P]),
            "mv_write_pose_txt": (_I, [ctypes.c_char_p, _P]),
            "mv_write_trajectory_ply": (_I, [ctypes.c_char_p, _I, _P]),
            "mv_read_transform_npy": (_I, [ctypes.c_char_p, _P]),
            "mv_compute_trajectory": (_I, [_P, _I, _I, ctypes.c_char_p, ctypes.c_char_p, _I, ctypes.POINTER(_I)]),
            "mv_local_feature_init": (None, [_P]),
            "mv_local_feature_init_with_id": (None, [_P, _I, _I]),
            "mv_local_feature_update": (None, [_P, _I]),
            "mv_local_feature_remove_old_frame": (ctypes.c_bool, [_P, _I]),
            "mv_local_feature_pool_init": (None, [_P]),
            "mv_local_feature_pool_insert": (_I, [_P, _I, _P, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_bool)]),
            "mv_local_feature_pool_delete": (_I, [_P, _I]),
            "mv_local_feature_pool_remove_old": (_I, [_P, _I]),
            "mv_local_feature_pool_valid_keys": (None, [_P, ctypes.POINTER(_I), _P]),
            "mv_local_feature_pool_load_factor": (_F, [_P]),
            "mv_local_feature_pool_check_invariant": (_I, [_P, _I]),
            "mv_local_feature_pool_track_frame": (_I, [_P, _I, _I, _P]),
            "mv_vocabulary_create": (_I, [_P, _I, _I, _P, _P, _P, _P, ctypes.POINTER(_P)]),
            "mv_vocabulary_destroy": (_I, [_P]),
            "mv_bow_words_batch_dev": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
            "mv_bow_words_host": (_I, [_P, _P, _I, _F, _P, _I, _P, _P, _P, _P, _P, _P]),
            "mv_word_set_stride": (_I, [_I]),
            "mv_word_sets_batch_dev": (_I, [_P, _I, _I, _I, _P, _P, _P]),
            "mv_lcd_overlap_dev": (_I, [_P, _I, _I, _P, _I, _P, _P]),
            "mv_lcd_best_dev": (_I, [_P, _I, _I, _P, _I, _P, _P, _P, _P]),
            "mv_lcd_overlap_sorted_host": (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _P]),
            "mv_landmark_params_default": (None, [_P]),
            "mv_tracks_link_dev": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
            "mv_tracks_triangulate_dev": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
            "mv_tracks_factors_dev": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
            "mv_ba_params_default": (None, [_P]),
            "mv_ba_solve_dev": (_I, [_P, _P, _I, _I, _I, _I] + [_P] * 14),
            "mv_pg_params_default": (None, [_P]),
            "mv_pg_solve_dev": (_I, [_P, _P, _I, _I, _I, _I] + [_P] * 13),
            "mv_pg_envelope_host": (_I, [_I, _I, _P, _P, _P]),
            "mv_pg_edges_from_transforms_dev": (_I, [_P, _I, _P, _P]),
            "mv_pnp_params_default": (None, [_P]),
            "mv_pnp_correspondences_dev": (_I, [_P, _I, _I, _I, _P, ctypes.c_long] + [_P] * 9),
            "mv_pnp_solve_dev": (_I, [_P, _P, _I, _I] + [_P] * 11),
            "mv_map_params_default": (None, [_P]),
            "mv_map_descriptors_dev": (_I, [_P, _I, _I, _I, _I] + [_P] * 5),
            "mv_map_match_dev": (_I, [_P, _P, _I, _I, _I] + [_P] * 17),
            "mv_map_index_dev": (_I, [_P, _I, _I, _I, _I, _I] + [_P] * 7),
            "mv_map_extend_dev": (_I, [_P, _I, _I, _I, _I, _I] + [_P] * 19),
            "mv_map_triangulate_dev": (_I, [_P, _P, _I, _I, _I, _I, _I] + [_P] * 11),
            "mv_ba_window_params_default": (None, [_P]),
            "mv_map_covisibility_dev": (_I, [_P, _I, _I, _I, _I, _I] + [_P] * 6),
            "mv_ba_window_select_dev": (_I, [_P, _P, _I, _I, _I, _I] + [_P] * 7),
            "mv_ba_window_factors_dev": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I] + [_P] * 15),
            "mv_ba_window_scatter_dev": (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
            "mv_map_correct_params_default": (None, [_P]),
            "mv_map_move_landmarks_dev": (_I, [_P, _P, _I, _I, _I, _I, _I] + [_P] * 10),
            "mv_map_fuse_pairs_dev": (_I, [_P, _I, _I, _I, _I, _I] + [_P] * 12),
            "mv_map_fuse_dev": (_I, [_P, _I, _I, _I, _I, _I, _I] + [_P] * 17),
            "mv_map_cull_params_default": (None, [_P]),
            "mv_map_screen_obs_dev": (_I, [_P, _P, _I, _I, _I, _I, _I] + [_P] * 12),
            "mv_map_stale_tracks_dev": (_I, [_P, _P, _I, _I, _I, _I, _I] + [_P] * 6),
            "mv_map_cull_frames_dev": (_I, [_P, _P, _I, _I, _I, _I, _I] + [_P] * 8),
            "mv_map_cull_dev": (_I, [_P, _P, _I, _I, _I, _I, _I] + [_P] * 17),
            "mv_map_compact_dev": (_I, [_P, _I, _I, _I, _I] + [_P] * 11),
        }
        for name, (res, args) in sig.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                # an alternate build (MV_LIB) may predate an entry point: A/B runs that do not use it
                # still load; using it raises AttributeError.  The shipping build must have them all.
                if os.environ.get("MV_LIB"):
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _np(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _params(cls, default_fn_name, kw):
    """A params struct of `cls` filled by the library's `default_fn_name`, then the overrides in kw."""
    p = cls()
    getattr(lib(), default_fn_name)(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def kp_params(**kw):
    """mv_kp_params (conf_thresh 0.015, nms_dist 4, border 4 -- pairwise_pnp.py:589-591, :99)."""
    return _params(KpParams, "mv_kp_params_default", kw)


# ---------------- trajectory (include/trajectory.h; python/compute_trajectory.py) ----------------
CHAIN_AS_BUILT, CHAIN_COMPOSE = 0, 1


def write_pose_txt(path, pose):
    """np.savetxt(pose[:3, :], fmt='%.6f') (compute_trajectory.py:49-51), in C."""
    p = np.ascontiguousarray(pose, np.float64).reshape(-1)[:12].copy()
    check(lib().mv_write_pose_txt(os.fsencode(path), _np(p)), "write_pose_txt")


def write_trajectory_ply(path, xyz):
    """write_ply (compute_trajectory.py:6-43), in C."""
    x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    check(lib().mv_write_trajectory_ply(os.fsencode(path), x.shape[0], _np(x)), "write_trajectory_ply")


def read_transform_npy(path):
    """A (3, 4) float64 .npy read by the library's C reader -> (status, [3, 4])."""
    T = np.zeros(12, np.float64)
    st = lib().mv_read_transform_npy(os.fsencode(path), _np(T))
    return st, T.reshape(3, 4)


def sequence_shard(frames, world, rank):
    """Frames [lo, hi) of a track of `frames` frames that `rank` of `world` matches in sequence
    mode: the frames - 1 pairs (b, b + 1) are split into contiguous, near-equal ranges, and a
    rank's frames run one past its last pair, so neighbouring ranks share one boundary frame
    and every pair is matched by exactly one rank -- no data-path collective.  A rank with no
    pair gets lo == hi."""
    if frames < 2 or world < 1 or not 0 <= rank < world:
        raise ValueError("sequence_shard: frames >= 2, 0 <= rank < world")
    pairs = frames - 1
    p_lo = rank * pairs // world
    p_hi = (rank + 1) * pairs // world
    return (p_lo, p_hi + 1) if p_hi > p_lo else (p_lo, p_lo)


def chain_sharded(chain_local, rebase, gather, rank, rel_local, mode):
    """A sequence sharded over ranks in order (rank r holds transforms [k_r, k_{r+1})):
    each rank chains its shard from the identity (chain_local(rel) -> poses [len+1, 3, 4]),
    the ranks exchange their shard's end pose (gather(last) -> [world] list, rank order:
    the RCCL all-gather on GPUs), every rank folds the ends of the ranks before it into its
    start pose (host, world x 3x4) and re-bases its poses on it (rebase(poses, start)).
    Returns this rank's poses [len+1, 3, 4]; its pose 0 is the previous rank's last pose."""
    import numpy as _n

    poses = chain_local(rel_local)
    ends = gather(_n.asarray(poses[-1], _n.float64))
    start = _n.eye(4)[:3].copy()
    for r in range(rank):  # start <- end_r applied after start (the chain rule, k_rebase order)
        E = _n.asarray(ends[r], _n.float64)
        nxt = _n.zeros((3, 4))
        for i in range(3):
            for c in range(4):
                v = E[i, 0] * start[0, c]
                v = v + E[i, 1] * start[1, c]
                v = v + E[i, 2] * start[2, c]
                if c == 3:
                    v = v + E[i, 3] if mode == CHAIN_COMPOSE else E[i, 3] + start[i, 3]
                nxt[i, c] = v
        start = nxt
    if rank == 0:
        return poses
    return rebase(poses, start)


# ---------------- local feature pool (include/feature_pool.h; include/local_feature_pool.h) ----------------
MAX_LOCAL_FRAMES, LOCAL_FEATURE_POOL_CAPACITY = 8, 3000


class LocalFeature(ctypes.Structure):
    """mv_local_feature = the reference's LocalFeature (local_feature_pool.h:16-22)."""
    _fields_ = [("word_id", _I), ("frame_ptr", _I), ("num_frames", _I), ("frames", _I * MAX_LOCAL_FRAMES),
                ("coords_3D", _F * 3)]


class _LfpEntry(ctypes.Structure):
    _fields_ = [("key", _I), ("value", LocalFeature), ("is_occupied", ctypes.c_bool)]


class _LfpPool(ctypes.Structure):
    _fields_ = [("entries", _LfpEntry * LOCAL_FEATURE_POOL_CAPACITY), ("size", _I), ("capacity", _I)]


class LocalFeaturePool:
    """The local feature pool (host, C): the reference's LocalFeaturePool API with error codes
    in place of its exit() calls.  table() -> int32 [capacity, 13] (key, occupied, word_id,
    frame_ptr, num_frames, frames[8]), the layout the parity tests compare slot by slot."""

    def __init__(self):
        self._p = _LfpPool()
        ctypes.memset(ctypes.byref(self._p), 0, ctypes.sizeof(self._p))
        lib().mv_local_feature_pool_init(ctypes.byref(self._p))

    @property
    def size(self):
        return self._p.size

    @property
    def capacity(self):
        return self._p.capacity

    def insert(self, key, frame_num):
        """local_feature_pool_insert of a feature first seen at frame_num -> (status,
        inserted, the entry's LocalFeature or None)"""
        f = LocalFeature()
        lib().mv_local_feature_init_with_id(ctypes.byref(f), key, frame_num)
        out = _P()
        ins = ctypes.c_bool(False)
        st = lib().mv_local_feature_pool_insert(ctypes.byref(self._p), key, ctypes.byref(f), ctypes.byref(out),
                                                ctypes.byref(ins))
        feat = ctypes.cast(out, ctypes.POINTER(LocalFeature)).contents if out.value else None
        return st, ins.value, feat

    def delete(self, key):
        return lib().mv_local_feature_pool_delete(ctypes.byref(self._p), key)

    def remove_old(self, current_frame_num):
        return lib().mv_local_feature_pool_remove_old(ctypes.byref(self._p), current_frame_num)

    def valid_keys(self):
        keys = np.zeros(LOCAL_FEATURE_POOL_CAPACITY, np.int32)
        n = _I(0)
        lib().mv_local_feature_pool_valid_keys(ctypes.byref(self._p), ctypes.byref(n), _np(keys))
        return keys[:n.value].copy()

    def load_factor(self):
        return float(lib().mv_local_feature_pool_load_factor(ctypes.byref(self._p)))

    def check_invariant(self, cur_frame):
        return lib().mv_local_feature_pool_check_invariant(ctypes.byref(self._p), cur_frame)

    def track_frame(self, frame_num, word_ids):
        ids = np.ascontiguousarray(word_ids, np.int32)
        return lib().mv_local_feature_pool_track_frame(ctypes.byref(self._p), frame_num, ids.size, _np(ids))

    def table(self):
        # an entry is 16 words: key, word_id, frame_ptr, num_frames, frames[8], coords[3],
        # is_occupied (byte 0 of word 15)
        assert ctypes.sizeof(_LfpEntry) == 64
        raw = np.frombuffer(self._p, dtype=np.int32, count=LOCAL_FEATURE_POOL_CAPACITY * 16).reshape(-1, 16)
        t = np.empty((self._p.capacity, 13), np.int32)
        t[:, 0] = raw[:, 0]
        t[:, 1] = raw[:, 15] & 0xFF
        t[:, 2:13] = raw[:, 1:12]
        return t


def _t(x):
    """device pointer of a torch tensor (or None)"""
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def check(st, what=""):
    if st != MV_OK:
        L = lib()
        raise MVError("%s: %s (%s)" % (what, L.mv_status_string(st).decode(), L.mv_last_error_message().decode()))


def device_count():
    return lib().mv_device_count()


def profile_enable(on=True):
    check(lib().mv_profile_enable(1 if on else 0), "profile_enable")


def profile_query(kernel):
    """(total device ms, launches) of `kernel` since profile_enable(True)."""
    ms = ctypes.c_double(0)
    n = ctypes.c_int(0)
    check(lib().mv_profile_query(kernel.encode(), ctypes.byref(ms), ctypes.byref(n)), "profile_query")
    return ms.value, n.value


def window_params(semantics=AS_BUILT, **kw):
    p = WindowParams()
    lib().mv_window_params_default(ctypes.byref(p))
    p.semantics = semantics
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def pose_params(semantics=AS_INTENDED, **kw):
    p = PoseParams()
    lib().mv_pose_params_default(ctypes.byref(p), semantics)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def track_params(semantics=AS_BUILT):
    p = TrackParams()
    lib().mv_track_params_default(ctypes.byref(p), semantics)
    return p


def landmark_params(**kw):
    """mv_landmark_params (cos_min_parallax cos(1 degree), min_depth 0.1, max_reproj_px 2)."""
    return _params(LandmarkParams, "mv_landmark_params_default", kw)


def ba_params(**kw):
    """mv_ba_params with its defaults (max_iters 10, lambda_init 1e-4, up 10, down 0.1, min 1e-10,
    max 1e10, diag_floor 1e-6, rel_tol 1e-6, huber_px 0)."""
    return _params(BaParams, "mv_ba_params_default", kw)


def pg_params(**kw):
    """mv_pg_params with its defaults (max_iters 10, lambda_init 1e-4, up 10, down 0.1, min 1e-10,
    max 1e10, diag_floor 1e-6, rel_tol 1e-6, huber 0)."""
    return _params(PgParams, "mv_pg_params_default", kw)


def pnp_params(**kw):
    """mv_pnp_params with its defaults (hypotheses 256, refine_rounds 2, min_inliers 6, max_iters 10,
    inlier_thresh_px 2, min_depth 0.1 and mv_ba_params' LM fields)."""
    return _params(PnpParams, "mv_pnp_params_default", kw)


def map_params(**kw):
    """mv_map_params with its defaults (radius_px 16, min_depth 0.1, thresh 0.8, ratio 0 = off, and
    the width / height binning hint)."""
    return _params(MapParams, "mv_map_params_default", kw)


def ba_window_params(**kw):
    """mv_ba_window_params with its defaults (min_shared 15, n_fixed 2, min_obs 2)."""
    return _params(BaWindowParams, "mv_ba_window_params_default", kw)


def map_correct_params(**kw):
    """mv_map_correct_params with its default (split_rel 1e-2)."""
    return _params(MapCorrectParams, "mv_map_correct_params_default", kw)


def map_cull_params(**kw):
    """mv_map_cull_params with its defaults (max_reproj_px 2, min_depth 0.1, worst_only 0, min_obs 2,
    stale_age 2, stale_min_obs 3, min_views 3, redundant 9 / 10)."""
    return _params(MapCullParams, "mv_map_cull_params_default", kw)


def pg_envelope(nodes, edge_i, edge_j, node_fixed=None):
    """The row envelope of one pose graph in 6 x 6 blocks (mv_pg_envelope_host), to size pg_solve's
    env_cap: edge_i / edge_j with local node ids in [0, nodes), node_fixed [nodes] (None: node 0 is
    held).  Host, no device; raises MVError for an id outside the graph or i == j."""
    ei, ej = np.ascontiguousarray(edge_i, np.int32), np.ascontiguousarray(edge_j, np.int32)
    assert ei.shape == ej.shape and ei.ndim == 1
    fx = None if node_fixed is None else np.ascontiguousarray(node_fixed, np.int32)
    assert fx is None or fx.shape == (int(nodes),)
    r = lib().mv_pg_envelope_host(int(nodes), ei.shape[0], _np(ei), _np(ej), None if fx is None else _np(fx))
    if r < 0:
        raise MVError("pg_envelope: %s" % lib().mv_status_string(r).decode())
    return r


def poses_to_q7(poses12):
    """[F][3][4] float64 camera-from-world poses [R | t], as trajectory_chain(..., mode=CHAIN_COMPOSE)
    gives them, -> [F][7] float32 (qw, qx, qy, qz, tx, ty, tz) with qw >= 0, the pose layout of
    include/factors.h and Context.tracks_triangulate.  Host, numpy only (not on the hot path).
    A monocular chain is built from per-pair translations of unit length, so its translations
    carry no metric scale: the caller supplies the scale (multiply each pair's t before chaining,
    or the chained t here) -- landmarks triangulated from the poses inherit it, and Context.pnp_solve
    (include/absolute_pose.h) carries it on to a new frame."""
    P = np.asarray(poses12, np.float64).reshape(-1, 3, 4)
    out = np.zeros((P.shape[0], 7), np.float64)
    for k in range(P.shape[0]):
        R = P[k, :, :3]
        # the largest of the four squared components first (Shepperd): no cancellation
        d = np.array([1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1.0 + R[0, 0] - R[1, 1] - R[2, 2],
                      1.0 - R[0, 0] + R[1, 1] - R[2, 2], 1.0 - R[0, 0] - R[1, 1] + R[2, 2]])
        c = int(np.argmax(d))
        s = 2.0 * np.sqrt(d[c])
        if c == 0:
            q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
        elif c == 1:
            q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
        elif c == 2:
            q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
        else:
            q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
        q = np.array(q)
        q /= np.sqrt((q * q).sum())
        if q[0] < 0:
            q = -q
        out[k, :4] = q
        out[k, 4:] = P[k, :, 3]
    return out.astype(np.float32)


def scale_as_built(scale):
    return float(lib().mv_scale_as_built(float(scale)))


class Context:
    """An mv_context on one device.  `stream` may be a torch.cuda.Stream."""

    def __init__(self, device=0):
        L = lib()
        h = ctypes.c_void_p()
        check(L.mv_context_create(device, ctypes.byref(h)), "mv_context_create")
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            lib().mv_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream):
        """Run later calls on `stream` (a torch.cuda.Stream -- torch's default stream is HIP's null
        stream, handle 0, and is used as such); None: back to the context's own stream."""
        if stream is None:
            check(lib().mv_context_use_own_stream(self.h), "use_own_stream")
        else:
            check(lib().mv_context_set_stream(self.h, ctypes.c_void_p(stream.cuda_stream)), "set_stream")

    def set_allpairs_screen(self, screen):
        """'i8' (default: one pass, frame 1 quantised in-kernel), 'f16' or 'i8s' (int8 against a
        staged image): how the fp32 all-pairs match screens before its exact re-score."""
        check(lib().mv_context_set_allpairs_screen(self.h, SCREENS[screen]), "set_allpairs_screen")

    def allpairs_screen(self):
        r = lib().mv_context_allpairs_screen(self.h)
        if r < 0:
            check(r, "allpairs_screen")
        return {v: k for k, v in SCREENS.items()}[r]

    def synchronize(self):
        check(lib().mv_context_synchronize(self.h), "synchronize")

    def reserve(self, batch, cap):
        check(lib().mv_context_reserve(self.h, batch, cap), "reserve")

    # ---------------- host-pointer calls (numpy) ----------------
    def softmax_host(self, scale, semi):
        semi = np.ascontiguousarray(semi, np.int8)
        cells = semi.shape[0]
        nv = ctypes.c_int(0)
        mi = np.zeros(cells, np.int32)
        pr = np.zeros(cells, np.float32)
        check(lib().mv_softmax_host(self.h, float(scale), _np(semi), cells, ctypes.byref(nv), _np(mi), _np(pr)),
              "softmax_host")
        return nv.value, mi, pr

    def top_n_host(self, scale, semi, N, cap=1000):
        semi = np.ascontiguousarray(semi, np.int8)
        ns = ctypes.c_int(0)
        pa = np.zeros(N, np.int32)
        ix = np.zeros(N, np.int32)
        pr = np.zeros(N, np.float32)
        st = lib().mv_top_n_host(self.h, float(scale), _np(semi), semi.shape[0], N, cap, ctypes.byref(ns), _np(pa),
                                 _np(ix), _np(pr))
        n = max(ns.value, 0)
        return st, pa[:n].copy(), ix[:n].copy(), pr[:n].copy()

    def window_match_host(self, params, rows, cols, desc0, max_idx0, probs0, desc1, patches1, indices1):
        desc0 = np.ascontiguousarray(desc0, np.int8)
        desc1 = np.ascontiguousarray(desc1, np.int8)
        max_idx0 = np.ascontiguousarray(max_idx0, np.int32)
        probs0 = np.ascontiguousarray(probs0, np.float32)
        patches1 = np.ascontiguousarray(patches1, np.int32)
        indices1 = np.ascontiguousarray(indices1, np.int32)
        M = params.max_matches
        p1 = np.zeros((M, 2), np.float32)
        p2 = np.zeros((M, 2), np.float32)
        q = np.zeros(M, np.int32)
        nm = ctypes.c_int(0)
        check(lib().mv_window_match_host(self.h, ctypes.byref(params), rows, cols, _np(desc0), _np(max_idx0),
                                         _np(probs0), _np(desc1), len(patches1), _np(patches1), _np(indices1),
                                         ctypes.byref(nm), _np(p1), _np(p2), _np(q)), "window_match_host")
        n = nm.value
        return p1[:n].copy(), p2[:n].copy(), q[:n].copy()

    def ransac_stub_host(self, pts1, pts2, thresh=1.1):
        pts1 = np.ascontiguousarray(pts1, np.float32)
        pts2 = np.ascontiguousarray(pts2, np.float32)
        n = pts1.shape[0]
        E = np.zeros(9, np.float32)
        inl = np.zeros(max(n, 1000), np.int32)
        ni = ctypes.c_int(0)
        check(lib().mv_ransac_stub_host(self.h, n, _np(pts1), _np(pts2), float(thresh), _np(E), _np(inl),
                                        ctypes.byref(ni)), "ransac_stub_host")
        return E.reshape(3, 3), inl[:ni.value].copy(), ni.value

    def recover_pose_host(self, E):
        E = np.ascontiguousarray(E, np.float32).reshape(9)
        R1 = np.zeros(9, np.float32)
        R2 = np.zeros(9, np.float32)
        t = np.zeros(3, np.float32)
        check(lib().mv_recover_pose_host(self.h, _np(E), _np(R1), _np(R2), _np(t)), "recover_pose_host")
        return R1.reshape(3, 3), R2.reshape(3, 3), t

    def svd3_host(self, A):
        A = np.ascontiguousarray(A, np.float32).reshape(9)
        U = np.zeros(9, np.float32)
        S = np.zeros(3, np.float32)
        V = np.zeros(9, np.float32)
        check(lib().mv_svd3_host(self.h, _np(A), _np(U), _np(S), _np(V)), "svd3_host")
        return U.reshape(3, 3), S, V.reshape(3, 3)

    def track_pair_host(self, params, rows, cols, f0, f1):
        """f = dict(semi_scale, semi [cells,65] i8, desc [cells,256] i8)"""
        s0 = np.ascontiguousarray(f0["semi"], np.int8)
        d0 = np.ascontiguousarray(f0["desc"], np.int8)
        s1 = np.ascontiguousarray(f1["semi"], np.int8)
        d1 = np.ascontiguousarray(f1["desc"], np.int8)
        M = params.window.max_matches
        T = np.zeros((3, 4), np.float32)
        p1 = np.zeros((M, 2), np.float32)
        p2 = np.zeros((M, 2), np.float32)
        nm = ctypes.c_int(0)
        st = lib().mv_track_pair_host(self.h, ctypes.byref(params), rows, cols, float(f0["semi_scale"]), _np(s0),
                                      _np(d0), float(f1["semi_scale"]), _np(s1), _np(d1), _np(T), ctypes.byref(nm),
                                      _np(p1), _np(p2))
        n = nm.value
        return st, T, p1[:n].copy(), p2[:n].copy()

    # ---------------- batched device calls (torch tensors on this device) ----------------
    def softmax_batch(self, scales, semi, max_idx, probs, num_valid):
        B, cells = semi.shape[0], semi.shape[1]
        check(lib().mv_softmax_batch_dev(self.h, B, cells, _t(scales), _t(semi), _t(max_idx), _t(probs),
                                         _t(num_valid)), "softmax_batch")

    def projection_factors(self, landmarks, poses, cameras, ldmk_id, pose_id, meas, err, J=None, H=None):
        """Device tensors (include/factors.h): err [F, 2], J [F, 20], H [F, 100]."""
        check(lib().mv_projection_factors_dev(self.h, ldmk_id.shape[0], _t(landmarks), _t(poses), _t(cameras),
                                              _t(ldmk_id), _t(pose_id), _t(meas), _t(err), _t(J), _t(H)),
              "projection_factors")

    def pose_normal_equations(self, pose_offsets, J, HPP, g, ee):
        check(lib().mv_pose_normal_equations_dev(self.h, pose_offsets.shape[0] - 1, _t(pose_offsets), _t(J), _t(HPP),
                                                 _t(g), _t(ee)), "pose_normal_equations")

    def lba_schur(self, num_poses, num_ldmks, chunk, J, C, semantics=AS_INTENDED):
        """local-BA Schur back-end on device tensors J [B, chunks, P*chunk, 20], C [B, S*S]."""
        check(lib().mv_lba_schur_dev(self.h, J.shape[0], num_poses, num_ldmks, chunk, int(semantics), _t(J), _t(C)),
              "lba_schur")

    def run_nms_batch(self, rows, cols, max_idx, probs, num_kp, kp):
        """src/run_nms.c cell NMS on device tensors max_idx/probs [B, cells] (in place)."""
        check(lib().mv_run_nms_batch_dev(self.h, max_idx.shape[0], rows, cols, _t(max_idx), _t(probs), _t(num_kp),
                                         _t(kp)), "run_nms_batch")

    def top_n_select_batch(self, max_idx, probs, N, cap, num_sel, patches, indices, sel_probs, status):
        B, cells = max_idx.shape[0], max_idx.shape[1]
        check(lib().mv_top_n_select_batch_dev(self.h, B, cells, _t(max_idx), _t(probs), N, cap, _t(num_sel),
                                              _t(patches), _t(indices), _t(sel_probs), _t(status)),
              "top_n_select_batch")

    def window_match_batch(self, params, rows, cols, desc0, max_idx0, probs0, desc1, num_sel, patches1, indices1,
                           num_matches, points1, points2, query_of_match=None):
        B, N = patches1.shape[0], patches1.shape[1]
        check(lib().mv_window_match_batch_dev(self.h, ctypes.byref(params), B, rows, cols, _t(desc0), _t(max_idx0),
                                              _t(probs0), _t(desc1), N, _t(num_sel), _t(patches1), _t(indices1),
                                              _t(num_matches), _t(points1), _t(points2), _t(query_of_match)),
              "window_match_batch")

    def match_allpairs_f32(self, desc0, desc1, n0, n1, match_idx, match_score, thresh=0.8):
        B, cap = desc0.shape[0], desc0.shape[1]
        check(lib().mv_match_allpairs_f32_dev(self.h, B, cap, _t(n0), _t(n1), _t(desc0), _t(desc1), float(thresh),
                                              _t(match_idx), _t(match_score)), "match_allpairs_f32")

    def match_allpairs_f32_prepare(self, desc1, n1):
        """Stage frame 1 of a batch on the auxiliary stream (see mv_match_allpairs_f32_prepare_dev)."""
        B, cap = desc1.shape[0], desc1.shape[1]
        check(lib().mv_match_allpairs_f32_prepare_dev(self.h, B, cap, _t(n1), _t(desc1)), "match_allpairs_f32_prepare")

    def match_allpairs_f32_run(self, desc0, desc1, n0, n1, match_idx, match_score, thresh=0.8):
        """Match a batch staged by match_allpairs_f32_prepare(desc1, n1)."""
        B, cap = desc0.shape[0], desc0.shape[1]
        check(lib().mv_match_allpairs_f32_run_dev(self.h, B, cap, _t(n0), _t(n1), _t(desc0), _t(desc1), float(thresh),
                                                  _t(match_idx), _t(match_score)), "match_allpairs_f32_run")

    def match_allpairs_f32_run_prepare(self, desc0, desc1, n0, n1, match_idx, match_score, next_desc1, next_n1,
                                       thresh=0.8):
        """Match the prepared batch (desc1, n1) and stage the next batch's frame 1 in the same
        launch (mv_match_allpairs_f32_run_prepare_dev); the next batch is then the prepared one."""
        B, cap = desc0.shape[0], desc0.shape[1]
        nB, ncap = next_desc1.shape[0], next_desc1.shape[1]
        check(lib().mv_match_allpairs_f32_run_prepare_dev(self.h, B, cap, _t(n0), _t(n1), _t(desc0), _t(desc1),
                                                          float(thresh), _t(match_idx), _t(match_score), nB, ncap,
                                                          _t(next_n1), _t(next_desc1)), "match_allpairs_f32_run_prepare")

    def keypoints(self, semi, coarse_desc, H, W, num_kp, kp, conf, desc, status, heat=None, params=None):
        """Device tensors: semi [B, 65, Hc, Wc], coarse_desc [B, 256, Hc, Wc] (network outputs)
        -> num_kp [B], kp [B, cap, 2], conf [B, cap], desc [B, cap, 256], status [B]
        (SuperPointFrontend.run after the forward; include/keypoints.h)."""
        B, Hc, Wc = semi.shape[0], semi.shape[2], semi.shape[3]
        p = params or kp_params()
        check(lib().mv_keypoints_dev(self.h, ctypes.byref(p), B, Hc, Wc, int(H), int(W), _t(semi), _t(coarse_desc),
                                     kp.shape[1], _t(num_kp), _t(kp), _t(conf), _t(desc), _t(heat), _t(status)),
              "keypoints")

    def keypoints_host(self, semi, coarse_desc, H, W, cap=4096, params=None):
        """numpy, one frame: semi [65, Hc, Wc], coarse_desc [256, Hc, Wc] -> (pts [n, 3] (x, y,
        conf), desc [n, 256], status)."""
        semi = np.ascontiguousarray(semi, np.float32)
        cd = np.ascontiguousarray(coarse_desc, np.float32)
        Hc, Wc = semi.shape[1], semi.shape[2]
        kp = np.zeros((cap, 2), np.float32)
        conf = np.zeros(cap, np.float32)
        desc = np.zeros((cap, 256), np.float32)
        n = ctypes.c_int(0)
        p = params or kp_params()
        st = lib().mv_keypoints_host(self.h, ctypes.byref(p), Hc, Wc, int(H), int(W), _np(semi), _np(cd), cap,
                                     ctypes.byref(n), _np(kp), _np(conf), _np(desc))
        if st not in (MV_OK, MV_ERR_CAPACITY):
            check(st, "keypoints_host")
        k = n.value
        return np.concatenate([kp[:k], conf[:k, None]], axis=1), desc[:k].copy(), st

    def trajectory_chain(self, rel, poses, present=None, start=None, mode=CHAIN_AS_BUILT):
        """Device tensors: rel [B, len, 3, 4] float64 -> poses [B, len + 1, 3, 4] (k_chain)."""
        B, n = rel.shape[0], rel.shape[1]
        check(lib().mv_trajectory_chain_dev(self.h, B, n, _t(rel), _t(present), _t(start), int(mode), _t(poses)),
              "trajectory_chain")

    def trajectory_rebase(self, base, poses, mode=CHAIN_AS_BUILT):
        """Device tensors: poses [B, len1, 3, 4] re-based on base [B, 3, 4] in place (k_rebase)."""
        check(lib().mv_trajectory_rebase_dev(self.h, poses.shape[0], poses.shape[1], _t(base), int(mode), _t(poses)),
              "trajectory_rebase")

    def trajectory_chain_host(self, rel, present=None, start=None, mode=CHAIN_AS_BUILT):
        """numpy: one sequence rel [len, 3, 4] float64 -> poses [len + 1, 3, 4] (on the GPU)."""
        r = np.ascontiguousarray(rel, np.float64).reshape(-1, 12)
        out = np.zeros((r.shape[0] + 1, 12), np.float64)
        pr = None if present is None else np.ascontiguousarray(present, np.int32)
        st = None if start is None else np.ascontiguousarray(start, np.float64).reshape(12)
        check(lib().mv_trajectory_chain_host(self.h, r.shape[0], _np(r), None if pr is None else _np(pr),
                                             None if st is None else _np(st), int(mode), _np(out)),
              "trajectory_chain_host")
        return out.reshape(-1, 3, 4)

    def compute_trajectory(self, start_frame, end_frame, pose_dir, out_dir, mode=CHAIN_AS_BUILT):
        """compute_trajectory.py main() with the chain on the GPU; returns poses written."""
        n = ctypes.c_int(0)
        check(lib().mv_compute_trajectory(self.h, int(start_frame), int(end_frame), os.fsencode(pose_dir),
                                          os.fsencode(out_dir), int(mode), ctypes.byref(n)), "compute_trajectory")
        return n.value

    def match_two_way_f32(self, desc0, desc1, n0, n1, match_idx, match_dist=None, nn_thresh=0.7):
        """nn_match_two_way (pairwise_pnp.py:281-323) on device tensors: match_idx [B, cap]."""
        B, cap = desc0.shape[0], desc0.shape[1]
        check(lib().mv_match_two_way_f32_dev(self.h, B, cap, _t(n0), _t(n1), _t(desc0), _t(desc1), float(nn_thresh),
                                             _t(match_idx), _t(match_dist)), "match_two_way_f32")

    def match_allpairs_i8(self, desc0, desc1, n0, n1, match_idx, match_dot):
        B, cap = desc0.shape[0], desc0.shape[1]
        check(lib().mv_match_allpairs_i8_dev(self.h, B, cap, _t(n0), _t(n1), _t(desc0), _t(desc1), _t(match_idx),
                                             _t(match_dot)), "match_allpairs_i8")

    def pose_batch(self, params, n, pts0, pts1, T, num_inliers, status):
        B, cap = pts0.shape[0], pts0.shape[1]
        check(lib().mv_pose_batch_dev(self.h, ctypes.byref(params), B, cap, _t(n), _t(pts0), _t(pts1), _t(T),
                                      _t(num_inliers), _t(status)), "pose_batch")

    def match_sequence_f32(self, desc, n, match_idx, match_score, thresh=0.8):
        """Consecutive frames desc[F][cap][256] -> pairs (b, b + 1): match_idx[F-1][cap]
        (mv_match_sequence_f32_dev; every frame quantised once)."""
        F, cap = desc.shape[0], desc.shape[1]
        check(lib().mv_match_sequence_f32_dev(self.h, F, cap, _t(n), _t(desc), float(thresh), _t(match_idx),
                                              _t(match_score)), "match_sequence_f32")

    def match_sequence_f32_run_prepare(self, desc, n, match_idx, match_score, next_desc, next_n, thresh=0.8):
        """Match the prepared chunk desc[F] (pairs b, b + 1) and stage the next chunk's frames in the
        same launch (mv_match_sequence_f32_run_prepare_dev); prepare the first chunk with
        match_allpairs_f32_prepare(desc, n)."""
        F, cap = desc.shape[0], desc.shape[1]
        nF, ncap = next_desc.shape[0], next_desc.shape[1]
        check(lib().mv_match_sequence_f32_run_prepare_dev(self.h, F, cap, _t(n), _t(desc), float(thresh),
                                                          _t(match_idx), _t(match_score), nF, ncap, _t(next_n),
                                                          _t(next_desc)), "match_sequence_f32_run_prepare")

    def pose_from_matches(self, params, n0, match_idx, kp0, kp1, T, num_matches, num_inliers, status):
        B, cap = kp0.shape[0], kp0.shape[1]
        check(lib().mv_pose_from_matches_dev(self.h, ctypes.byref(params), B, cap, _t(n0), _t(match_idx), _t(kp0),
                                             _t(kp1), _t(T), _t(num_matches), _t(num_inliers), _t(status)),
              "pose_from_matches")

    # ---------------- tracks, landmarks, factors (include/feature_tracks.h) ----------------
    landmark_params = staticmethod(landmark_params)  # also reachable as ctx.landmark_params(**kw)

    def tracks_link(self, n, match_idx, match_score, track_id, num_tracks, track_first, track_len, status, min_len=2):
        """Device tensors: n [B, F], match_idx / match_score [B, F-1, cap] (match_score may be None)
        -> track_id [B, F, cap], num_tracks [B], track_first / track_len [B, track_cap], status [B]."""
        B, F, cap = track_id.shape
        check(lib().mv_tracks_link_dev(self.h, B, F, cap, _t(n), _t(match_idx), _t(match_score), int(min_len),
                                       track_first.shape[1], _t(track_id), _t(num_tracks), _t(track_first),
                                       _t(track_len), _t(status)), "tracks_link")

    def tracks_triangulate(self, poses, cameras, kp, match_idx, num_tracks, track_first, track_len, status, landmarks,
                           ldmk_flags, params=None):
        """Device tensors: poses [B, F, 7], cameras [B, F, 4], kp [B, F, cap, 2] and tracks_link's
        outputs -> landmarks [B, track_cap, 3] float32, ldmk_flags [B, track_cap] int32 (0 = usable)."""
        B, F, cap = kp.shape[0], kp.shape[1], kp.shape[2]
        p = params or landmark_params()
        check(lib().mv_tracks_triangulate_dev(self.h, ctypes.byref(p), B, F, cap, track_first.shape[1], _t(poses),
                                              _t(cameras), _t(kp), _t(match_idx), _t(num_tracks), _t(track_first),
                                              _t(track_len), _t(status), _t(landmarks), _t(ldmk_flags)),
              "tracks_triangulate")

    def tracks_factors(self, kp, track_id, ldmk_flags, ldmk_id, pose_id, meas, pose_offsets, status):
        """Device tensors: kp [B, F, cap, 2], track_id [B, F, cap], ldmk_flags [B, track_cap] ->
        ldmk_id / pose_id [factor_cap], meas [factor_cap, 2], pose_offsets [B * F + 1], status [1]:
        the factor list of projection_factors / pose_normal_equations."""
        B, F, cap = track_id.shape
        check(lib().mv_tracks_factors_dev(self.h, B, F, cap, ldmk_flags.shape[1], ldmk_id.shape[0], _t(kp),
                                          _t(track_id), _t(ldmk_flags), _t(ldmk_id), _t(pose_id), _t(meas),
                                          _t(pose_offsets), _t(status)), "tracks_factors")

    # ---------------- windowed bundle adjustment (include/bundle_adjust.h) ----------------
    ba_params = staticmethod(ba_params)

    def ba_solve(self, poses, landmarks, cameras, ldmk_id, pose_id, meas, pose_offsets, track_cap, poses_out,
                 landmarks_out, cost_initial, cost_final, iters, status, pose_fixed=None, params=None):
        """Device tensors: poses [B, F, 7], landmarks [B, track_cap, 3], cameras [B, F, 4] and
        tracks_factors' outputs (ldmk_id / pose_id [stored], meas [stored, 2], pose_offsets [B * F + 1])
        -> poses_out, landmarks_out (may be the inputs themselves), cost_initial / cost_final [B]
        float64, iters / status [B] int32.  pose_fixed [B, F] int32 (None: pose 0 of every window)."""
        B, F = poses.shape[0], poses.shape[1]
        p = params or ba_params()
        check(lib().mv_ba_solve_dev(self.h, ctypes.byref(p), B, F, int(track_cap), ldmk_id.shape[0], _t(poses),
                                    _t(landmarks), _t(cameras), _t(ldmk_id), _t(pose_id), _t(meas), _t(pose_offsets),
                                    _t(pose_fixed), _t(poses_out), _t(landmarks_out), _t(cost_initial),
                                    _t(cost_final), _t(iters), _t(status)), "ba_solve")

    # ---------------- pose-graph optimisation (include/pose_graph.h) ----------------
    pg_params = staticmethod(pg_params)

    def pg_solve(self, poses, edge_offsets, edge_i, edge_j, edge_kind, edge_z, edge_w, env_cap, poses_out,
                 cost_initial, cost_final, iters, status, node_fixed=None, params=None):
        """Device tensors: poses [B, N, 7] float32, edge_offsets [B + 1] int32, edge_i / edge_j /
        edge_kind [stored] int32 (global node ids g * N + n; PG_EDGE_SE3 or PG_EDGE_DIRECTION), edge_z
        [stored, 7] float32 (the measured T_j T_i^-1), edge_w [stored, 2] float32 (w_rot, w_trans) ->
        poses_out (may be poses itself), cost_initial / cost_final [B] float64, iters / status [B]
        int32.  env_cap: the largest envelope of a graph in blocks (pg_envelope).  node_fixed [B, N]
        int32 (None: node 0 of every graph)."""
        B, N = poses.shape[0], poses.shape[1]
        p = params or pg_params()
        check(lib().mv_pg_solve_dev(self.h, ctypes.byref(p), B, N, edge_i.shape[0], int(env_cap), _t(poses),
                                    _t(edge_offsets), _t(edge_i), _t(edge_j), _t(edge_kind), _t(edge_z), _t(edge_w),
                                    _t(node_fixed), _t(poses_out), _t(cost_initial), _t(cost_final), _t(iters),
                                    _t(status)), "pg_solve")

    def pg_edges_from_transforms(self, T, z):
        """Device tensors: T [E, 3, 4] float32 ([R | t], what pose_from_matches gives) -> z [E, 7]
        float32 edge measurements, by poses_to_q7's arithmetic on the device."""
        check(lib().mv_pg_edges_from_transforms_dev(self.h, T.shape[0], _t(T), _t(z)), "pg_edges_from_transforms")

    # ---------------- map localisation (include/absolute_pose.h) ----------------
    pnp_params = staticmethod(pnp_params)

    def pnp_correspondences(self, track_id, ldmk_flags, landmarks, match_idx, n_prev, n_new, kp_new, pts3, pts2,
                            count):
        """Device tensors: track_id [B, cap] int32, the last map frame's row of tracks_link's track_id
        (a view such as track_id[:, F - 1] goes in in place: rows contiguous, any stride between
        problems), ldmk_flags [B, track_cap], landmarks [B, track_cap, 3], match_idx [B, cap] (last map
        frame -> new frame), n_prev / n_new [B], kp_new [B, cap, 2] -> pts3 [B, cap, 3], pts2
        [B, cap, 2] float32, count [B] int32: the 3D-2D pairs of pnp_solve."""
        B, cap = match_idx.shape
        assert track_id.shape == (B, cap) and (cap == 1 or track_id.stride(1) == 1)
        check(lib().mv_pnp_correspondences_dev(self.h, B, cap, ldmk_flags.shape[1], _t(track_id),
                                               track_id.stride(0) if B > 1 else cap, _t(ldmk_flags), _t(landmarks),
                                               _t(match_idx), _t(n_prev), _t(n_new), _t(kp_new), _t(pts3), _t(pts2),
                                               _t(count)), "pnp_correspondences")

    def pnp_solve(self, n, pts3, pts2, cameras, pose_out, inlier, num_inliers, best_hyp, status, cost,
                  pose_prior=None, params=None):
        """Device tensors: n [B] int32, pts3 [B, cap, 3], pts2 [B, cap, 2], cameras [B, 4] float32,
        pose_prior [B, 7] float32 or None -> pose_out [B, 7] float32 (camera-from-world, the map's
        scale), inlier [B, cap], num_inliers / best_hyp / status [B] int32, cost [B] float64."""
        B, cap = pts3.shape[0], pts3.shape[1]
        p = params or pnp_params()
        check(lib().mv_pnp_solve_dev(self.h, ctypes.byref(p), B, cap, _t(n), _t(pts3), _t(pts2), _t(cameras),
                                     _t(pose_prior), _t(pose_out), _t(inlier), _t(num_inliers), _t(best_hyp),
                                     _t(status), _t(cost)), "pnp_solve")

    # ---------------- map matching by projection (include/map_match.h) ----------------
    map_params = staticmethod(map_params)

    def map_descriptors(self, track_id, ldmk_flags, desc, ldmk_obs, ldmk_desc):
        """Device tensors: track_id [B, F, cap] int32 (tracks_link), ldmk_flags [B, track_cap] int32,
        desc [B, F, cap, 256] float32 -> ldmk_obs [B, track_cap] int32 (f * cap + i of the usable track's
        last observation, -1 otherwise), ldmk_desc [B, track_cap, 256] float32 (that row, or zeros)."""
        B, F, cap = track_id.shape
        assert desc.shape == (B, F, cap, 256) and ldmk_desc.shape == (B, ldmk_flags.shape[1], 256)
        check(lib().mv_map_descriptors_dev(self.h, B, F, cap, ldmk_flags.shape[1], _t(track_id), _t(ldmk_flags),
                                           _t(desc), _t(ldmk_obs), _t(ldmk_desc)), "map_descriptors")

    def map_match(self, n_ldmk, landmarks, ldmk_flags, ldmk_desc, pose_prior, cameras, n_new, kp_new, desc_new,
                  proj, ncand, match_idx, match_score, pts3, pts2, pair_ldmk, count, params=None):
        """Device tensors: n_ldmk [B] int32, landmarks [B, L, 3], ldmk_flags [B, L] int32, ldmk_desc
        [B, L, 256], pose_prior [B, 7], cameras [B, 4], n_new [B] int32, kp_new [B, cap, 2], desc_new
        [B, cap, 256] -> proj [B, L, 2] float32, ncand / match_idx [B, L] int32, match_score [B, L] float32,
        and the pairs in pnp_solve's layout: pts3 [B, cap, 3], pts2 [B, cap, 2], pair_ldmk [B, cap], count [B]."""
        B, L = ldmk_flags.shape
        cap = kp_new.shape[1]
        assert ldmk_desc.shape == (B, L, 256) and desc_new.shape == (B, cap, 256) and landmarks.shape == (B, L, 3)
        p = params or map_params()
        check(lib().mv_map_match_dev(self.h, ctypes.byref(p), B, L, cap, _t(n_ldmk), _t(landmarks), _t(ldmk_flags),
                                     _t(ldmk_desc), _t(pose_prior), _t(cameras), _t(n_new), _t(kp_new), _t(desc_new),
                                     _t(proj), _t(ncand), _t(match_idx), _t(match_score), _t(pts3), _t(pts2),
                                     _t(pair_ldmk), _t(count)), "map_match")

    # ---------------- map update (include/map_update.h) ----------------
    def map_index(self, track_id, num_tracks, status, track_first, track_len, next_obs, track_last, f_count=None):
        """Device tensors: track_id [B, F, cap], num_tracks / status [B] (tracks_link; rows of frames not
        yet used hold -1) -> track_first / track_len / track_last [B, track_cap], next_obs [B, F, cap]:
        the observation chains of the frames below f_count (None: all F)."""
        B, F, cap = track_id.shape
        assert next_obs.shape == (B, F, cap) and track_last.shape == track_first.shape == track_len.shape
        check(lib().mv_map_index_dev(self.h, B, F, cap, track_first.shape[1], F if f_count is None else int(f_count),
                                     _t(track_id), _t(num_tracks), _t(status), _t(track_first), _t(track_len),
                                     _t(next_obs), _t(track_last)), "map_index")

    def map_extend(self, f_new, n_prev, n_new, match_idx, match_score, status, track_id, num_tracks, track_first,
                   track_len, next_obs, track_last, touched, n_extended, n_created, ext_status, pair_ldmk=None,
                   pair_count=None, map_idx=None, inlier=None):
        """Appends frame f_new to the map state (track_id [B, F, cap], num_tracks [B], track_first /
        track_len / track_last [B, track_cap], next_obs [B, F, cap], all updated in place).  Device
        tensors: n_prev / n_new [B], match_idx / match_score [B, cap] from frame f_new - 1 to f_new
        (match_score may be None), status [B]; optionally map_match's pair_ldmk [B, cap], pair_count [B]
        and match_idx [B, track_cap] (map_idx) with pnp_solve's inlier [B, cap] -- all four or none ->
        touched [B, track_cap], n_extended / n_created / ext_status [B] int32."""
        B, F, cap = track_id.shape
        assert match_idx.shape == (B, cap) and next_obs.shape == (B, F, cap)
        assert touched.shape == track_last.shape == track_first.shape == track_len.shape
        check(lib().mv_map_extend_dev(self.h, B, F, cap, track_first.shape[1], int(f_new), _t(n_prev), _t(n_new),
                                      _t(match_idx), _t(match_score), _t(pair_ldmk), _t(pair_count), _t(map_idx),
                                      _t(inlier), _t(status), _t(track_id), _t(num_tracks), _t(track_first),
                                      _t(track_len), _t(next_obs), _t(track_last), _t(touched), _t(n_extended),
                                      _t(n_created), _t(ext_status)), "map_extend")

    def map_triangulate(self, poses, cameras, kp, num_tracks, track_first, track_len, next_obs, status, landmarks,
                        ldmk_flags, f_count=None, select=None, params=None):
        """Device tensors: poses [B, F, 7], cameras [B, F, 4], kp [B, F, cap, 2] and the map state ->
        landmarks [B, track_cap, 3] float32, ldmk_flags [B, track_cap] int32 from the observation chains
        of the frames below f_count (None: all F).  select [B, track_cap] int32 (map_extend's touched):
        only the entries with a nonzero select are recomputed; None: all."""
        B, F, cap = next_obs.shape
        assert kp.shape == (B, F, cap, 2) and (select is None or select.shape == ldmk_flags.shape)
        p = params or landmark_params()
        check(lib().mv_map_triangulate_dev(self.h, ctypes.byref(p), B, F, cap, track_first.shape[1],
                                           F if f_count is None else int(f_count), _t(poses), _t(cameras), _t(kp),
                                           _t(num_tracks), _t(track_first), _t(track_len), _t(next_obs), _t(status),
                                           _t(select), _t(landmarks), _t(ldmk_flags)), "map_triangulate")

    # ---------------- map loop correction (include/map_correct.h) ----------------
    map_correct_params = staticmethod(map_correct_params)

    def map_move_landmarks(self, poses_old, poses_new, num_tracks, track_first, track_len, track_last, status,
                           ldmk_flags, landmarks, retri, cap, f_count=None, params=None):
        """Device tensors: poses_old / poses_new [B, F, 7] (the poses the landmarks were made with and
        the corrected ones), the map state with cap keypoint slots per frame, ldmk_flags [B, track_cap]
        -> landmarks [B, track_cap, 3] carried with their anchor frames in place, retri [B, track_cap]
        int32: 1 where the track straddles the correction (map_triangulate's select)."""
        B, F = poses_old.shape[0], poses_old.shape[1]
        assert poses_new.shape == poses_old.shape == (B, F, 7) and landmarks.shape == (B, ldmk_flags.shape[1], 3)
        assert retri.shape == ldmk_flags.shape == track_first.shape == track_len.shape == track_last.shape
        p = params or map_correct_params()
        check(lib().mv_map_move_landmarks_dev(self.h, ctypes.byref(p), B, F, int(cap), ldmk_flags.shape[1],
                                              F if f_count is None else int(f_count), _t(poses_old), _t(poses_new),
                                              _t(num_tracks), _t(track_first), _t(track_len), _t(track_last),
                                              _t(status), _t(ldmk_flags), _t(landmarks), _t(retri)),
              "map_move_landmarks")

    def map_fuse_pairs(self, f_q, n_q, track_id, num_tracks, status, map_idx, pair_a, pair_b, count, f_count=None,
                       pair_ldmk=None, pair_count=None, inlier=None):
        """Device tensors: f_q / n_q [B] (the matched frame and its keypoint count), track_id
        [B, F, cap], num_tracks / status [B], map_idx [B, track_cap] (map_match's match_idx for frame
        f_q); optionally map_match's pair_ldmk [B, cap] and pair_count [B] with pnp_solve's inlier
        [B, cap] -- all three or none -> pair_a / pair_b [B, cap] (landmark, the track that owns its
        keypoint; ascending landmark, the tail -1), count [B] int32."""
        B, F, cap = track_id.shape
        assert pair_a.shape == pair_b.shape == (B, cap) and map_idx.shape[0] == B
        check(lib().mv_map_fuse_pairs_dev(self.h, B, F, cap, map_idx.shape[1], F if f_count is None else int(f_count),
                                          _t(f_q), _t(n_q), _t(track_id), _t(num_tracks), _t(status), _t(map_idx),
                                          _t(pair_ldmk), _t(pair_count), _t(inlier), _t(pair_a), _t(pair_b),
                                          _t(count)), "map_fuse_pairs")

    def map_fuse(self, pair_a, pair_b, pair_count, status, num_tracks, track_id, track_first, track_len, next_obs,
                 track_last, landmarks, ldmk_flags, touched, fused_into, n_fused, n_rejected, fuse_status,
                 f_count=None):
        """Merges the tracks of one point in the map state (track_id / next_obs [B, F, cap], track_first /
        track_len / track_last [B, track_cap], landmarks [B, track_cap, 3], ldmk_flags [B, track_cap], all
        updated in place).  Device tensors: pair_a / pair_b [B, pair_cap], pair_count [B] (map_fuse_pairs,
        or any other source), status / num_tracks [B] -> touched [B, track_cap] (1 at each kept track:
        map_triangulate's select), fused_into [B, track_cap] (the kept track at each dropped one, else
        -1), n_fused / n_rejected / fuse_status [B] int32."""
        B, F, cap = track_id.shape
        assert next_obs.shape == (B, F, cap) and pair_a.shape == pair_b.shape and pair_a.shape[0] == B
        assert touched.shape == fused_into.shape == ldmk_flags.shape == track_first.shape == track_last.shape
        check(lib().mv_map_fuse_dev(self.h, B, F, cap, track_first.shape[1], F if f_count is None else int(f_count),
                                    pair_a.shape[1], _t(pair_a), _t(pair_b), _t(pair_count), _t(status),
                                    _t(num_tracks), _t(track_id), _t(track_first), _t(track_len), _t(next_obs),
                                    _t(track_last), _t(landmarks), _t(ldmk_flags), _t(touched), _t(fused_into),
                                    _t(n_fused), _t(n_rejected), _t(fuse_status)), "map_fuse")

    # ---------------- map culling (include/map_cull.h) ----------------
    map_cull_params = staticmethod(map_cull_params)

    def map_screen_observations(self, poses, cameras, kp, num_tracks, track_first, track_len, next_obs, status,
                                landmarks, ldmk_flags, remove, n_bad, f_count=None, params=None):
        """Device tensors: poses [B, F, 7], cameras [B, F, 4], kp [B, F, cap, 2], the map state and its
        landmarks [B, track_cap, 3] / ldmk_flags [B, track_cap] -> remove [B, F, cap] int32 (1 at every
        observation that disagrees with its landmark; with params.worst_only only each track's worst),
        n_bad [B] int32."""
        B, F, cap = next_obs.shape
        assert kp.shape == (B, F, cap, 2) and remove.shape == (B, F, cap) and n_bad.shape == (B,)
        assert landmarks.shape == (B, ldmk_flags.shape[1], 3) and track_first.shape == ldmk_flags.shape
        p = params or map_cull_params()
        check(lib().mv_map_screen_obs_dev(self.h, ctypes.byref(p), B, F, cap, track_first.shape[1],
                                          F if f_count is None else int(f_count), _t(poses), _t(cameras), _t(kp),
                                          _t(num_tracks), _t(track_first), _t(track_len), _t(next_obs), _t(status),
                                          _t(landmarks), _t(ldmk_flags), _t(remove), _t(n_bad)),
              "map_screen_observations")

    def map_stale_tracks(self, num_tracks, track_len, track_last, status, ldmk_flags, drop, frames, cap, f_count=None,
                         params=None):
        """Device tensors: num_tracks / status [B], track_len / track_last / ldmk_flags [B, track_cap] of a
        map with `frames` frames of `cap` slots -> drop [B, track_cap] int32: 1 at every track that ended
        more than params.stale_age frames ago and is flagged or shorter than params.stale_min_obs."""
        B, L = track_len.shape
        assert drop.shape == track_last.shape == ldmk_flags.shape == (B, L)
        p = params or map_cull_params()
        check(lib().mv_map_stale_tracks_dev(self.h, ctypes.byref(p), B, int(frames), int(cap), L,
                                            int(frames) if f_count is None else int(f_count), _t(num_tracks),
                                            _t(track_len), _t(track_last), _t(status), _t(ldmk_flags), _t(drop)),
              "map_stale_tracks")

    def map_cull_frames(self, track_id, num_tracks, status, ldmk_flags, remove, frame_culled, n_culled, protect=None,
                        f_count=None, params=None):
        """The greedy keyframe cull.  Device tensors: track_id [B, F, cap], num_tracks / status [B],
        ldmk_flags [B, track_cap], optionally protect [B, F] (nonzero: never culled); remove [B, F, cap]
        is in/out (the mask so far; the culled frames' slots are added) -> frame_culled [B, F], n_culled
        [B] int32."""
        B, F, cap = track_id.shape
        assert remove.shape == (B, F, cap) and frame_culled.shape == (B, F) and n_culled.shape == (B,)
        assert protect is None or protect.shape == (B, F)
        p = params or map_cull_params()
        check(lib().mv_map_cull_frames_dev(self.h, ctypes.byref(p), B, F, cap, ldmk_flags.shape[1],
                                           F if f_count is None else int(f_count), _t(track_id), _t(num_tracks),
                                           _t(status), _t(ldmk_flags), _t(protect), _t(remove), _t(frame_culled),
                                           _t(n_culled)), "map_cull_frames")

    def map_cull(self, remove, drop, status, num_tracks, track_id, track_first, track_len, next_obs, track_last,
                 landmarks, ldmk_flags, touched, dropped, n_obs_removed, n_dropped, n_rejected, cull_status,
                 f_count=None, params=None):
        """Takes the marked observations (remove [B, F, cap] or None) and tracks (drop [B, track_cap] or
        None) out of the map state (track_id / next_obs [B, F, cap], track_first / track_len / track_last
        [B, track_cap], landmarks [B, track_cap, 3], ldmk_flags [B, track_cap], all updated in place) ->
        touched [B, track_cap] (1 at each shortened track: map_triangulate's select), dropped
        [B, track_cap], n_obs_removed / n_dropped / n_rejected / cull_status [B] int32."""
        B, F, cap = track_id.shape
        assert next_obs.shape == (B, F, cap) and (remove is None or remove.shape == (B, F, cap))
        assert touched.shape == dropped.shape == ldmk_flags.shape == track_first.shape == track_last.shape
        assert drop is None or drop.shape == touched.shape
        p = params or map_cull_params()
        check(lib().mv_map_cull_dev(self.h, ctypes.byref(p), B, F, cap, track_first.shape[1],
                                    F if f_count is None else int(f_count), _t(remove), _t(drop), _t(status),
                                    _t(num_tracks), _t(track_id), _t(track_first), _t(track_len), _t(next_obs),
                                    _t(track_last), _t(landmarks), _t(ldmk_flags), _t(touched), _t(dropped),
                                    _t(n_obs_removed), _t(n_dropped), _t(n_rejected), _t(cull_status)), "map_cull")

    def map_compact(self, status, track_id, num_tracks, track_first, track_len, track_last, landmarks, ldmk_flags,
                    new_id, old_id, n_live):
        """Renumbers the live tracks 0, 1, ... in place (track_id [B, F, cap], num_tracks [B], track_first /
        track_len / track_last / ldmk_flags [B, track_cap], landmarks [B, track_cap, 3]; next_obs holds
        slots and stays) -> new_id / old_id [B, track_cap] (mutually inverse, -1 elsewhere; per-track
        data of the caller's moves as x[old_id]), n_live [B] int32."""
        B, F, cap = track_id.shape
        assert new_id.shape == old_id.shape == ldmk_flags.shape == track_first.shape == track_last.shape
        assert landmarks.shape == (B, track_first.shape[1], 3) and n_live.shape == (B,)
        check(lib().mv_map_compact_dev(self.h, B, F, cap, track_first.shape[1], _t(status), _t(track_id),
                                       _t(num_tracks), _t(track_first), _t(track_len), _t(track_last), _t(landmarks),
                                       _t(ldmk_flags), _t(new_id), _t(old_id), _t(n_live)), "map_compact")

    # ---------------- local BA windows (include/ba_window.h) ----------------
    ba_window_params = staticmethod(ba_window_params)

    def map_covisibility(self, track_id, num_tracks, status, ldmk_flags, f_q, covis, f_count=None):
        """Device tensors: the map state track_id [B, F, cap], num_tracks / status [B], ldmk_flags
        [B, track_cap] and the query frames f_q [B] int32 -> covis [B, F] int32: the usable landmarks
        every frame below f_count (None: all F) shares with frame f_q."""
        B, F, cap = track_id.shape
        assert covis.shape == (B, F) and f_q.shape == (B,)
        check(lib().mv_map_covisibility_dev(self.h, B, F, cap, ldmk_flags.shape[1],
                                            F if f_count is None else int(f_count), _t(track_id), _t(num_tracks),
                                            _t(status), _t(ldmk_flags), _t(f_q), _t(covis)), "map_covisibility")

    def ba_window_select(self, covis, f_q, status, win_frames, win_count, pose_fixed, f_count=None, eligible=None,
                         params=None):
        """Device tensors: covis [B, F], f_q / status [B], eligible [B, F] int32 or None -> win_frames
        [B, W] (ascending frames, the tail -1), win_count [B], pose_fixed [B, W] int32: the W - 1 most
        covisible frames and f_q, the n_fixed oldest of them held."""
        B, F = covis.shape
        W = win_frames.shape[1]
        assert pose_fixed.shape == (B, W) and (eligible is None or eligible.shape == (B, F))
        p = params or ba_window_params()
        check(lib().mv_ba_window_select_dev(self.h, ctypes.byref(p), B, F, F if f_count is None else int(f_count), W,
                                            _t(covis), _t(f_q), _t(status), _t(eligible), _t(win_frames),
                                            _t(win_count), _t(pose_fixed)), "ba_window_select")

    def ba_window_factors(self, kp, poses, cameras, track_id, num_tracks, ldmk_flags, win_frames, win_obs, ldmk_id,
                          pose_id, meas, pose_offsets, status, poses_w, cameras_w, f_count=None, params=None):
        """Device tensors: kp [B, F, cap, 2], poses [B, F, 7], cameras [B, F, 4], the map state and
        win_frames [B, W] -> win_obs [B, track_cap], the factor list of ba_solve with frames = W (ldmk_id /
        pose_id [factor_cap], meas [factor_cap, 2], pose_offsets [B * W + 1], status [1]) and poses_w
        [B, W, 7], cameras_w [B, W, 4]."""
        B, F, cap = track_id.shape
        W = win_frames.shape[1]
        assert kp.shape == (B, F, cap, 2) and poses_w.shape == (B, W, 7) and cameras_w.shape == (B, W, 4)
        assert win_obs.shape == ldmk_flags.shape and pose_offsets.shape == (B * W + 1,)
        p = params or ba_window_params()
        check(lib().mv_ba_window_factors_dev(self.h, ctypes.byref(p), B, F, cap, ldmk_flags.shape[1],
                                             F if f_count is None else int(f_count), W, ldmk_id.shape[0], _t(kp),
                                             _t(poses), _t(cameras), _t(track_id), _t(num_tracks), _t(ldmk_flags),
                                             _t(win_frames), _t(win_obs), _t(ldmk_id), _t(pose_id), _t(meas),
                                             _t(pose_offsets), _t(status), _t(poses_w), _t(cameras_w)),
              "ba_window_factors")

    def ba_window_scatter(self, win_frames, poses_w, poses, f_count=None):
        """Device tensors: win_frames [B, W], poses_w [B, W, 7] (ba_solve's poses_out) -> poses [B, F, 7],
        the window's frames overwritten in place, every other pose untouched."""
        B, F = poses.shape[0], poses.shape[1]
        W = win_frames.shape[1]
        assert poses_w.shape == (B, W, 7) and win_frames.shape[0] == B
        check(lib().mv_ba_window_scatter_dev(self.h, B, F, F if f_count is None else int(f_count), W, _t(win_frames),
                                             _t(poses_w), _t(poses)), "ba_window_scatter")

    # ---------------- loop closure (include/loop_closure.h) ----------------
    def bow_words(self, voc, desc_scales, desc, num_sel, patches, base, wid, word_id, best_match, scores=None):
        """Device tensors: desc [B, cells, 256] int8, desc_scales / num_sel [B], patches [B, N];
        outputs [B, N] int32 and scores [B, N, nb] float32 (or None)."""
        B, cells, N = desc.shape[0], desc.shape[1], patches.shape[1]
        check(lib().mv_bow_words_batch_dev(self.h, voc.h, B, cells, N, _t(desc_scales), _t(desc), _t(num_sel),
                                           _t(patches), _t(base), _t(wid), _t(word_id), _t(best_match), _t(scores)),
              "bow_words")

    def bow_words_host(self, voc, desc_scale, desc, patches, want_scores=True):
        """One frame, numpy in and out -> dict(base, wid, word_id, best_match[, scores])."""
        desc = np.ascontiguousarray(desc, np.int8)
        patches = np.ascontiguousarray(patches, np.int32)
        n = patches.size
        out = {k: np.zeros(n, np.int32) for k in ("base", "wid", "word_id", "best_match")}
        sc = np.zeros((n, voc.num_base), np.float32) if want_scores else None
        check(lib().mv_bow_words_host(self.h, voc.h, desc.shape[0], float(desc_scale), _np(desc), n, _np(patches),
                                      _np(out["base"]), _np(out["wid"]), _np(out["word_id"]), _np(out["best_match"]),
                                      _np(sc) if want_scores else None), "bow_words_host")
        if want_scores:
            out["scores"] = sc
        return out

    def word_sets(self, num_words, word_id, bits, distinct):
        """word_id [B, N] int32 -> bits [B, word_set_stride(num_words)] int32, distinct [B]."""
        B, N = word_id.shape[0], word_id.shape[1]
        check(lib().mv_word_sets_batch_dev(self.h, num_words, B, N, _t(word_id), _t(bits), _t(distinct)), "word_sets")

    def lcd_overlap(self, num_words, q_bits, db_bits, counts):
        """counts [Q, F] int32 = popcount(q_bits[q] & db_bits[f])."""
        check(lib().mv_lcd_overlap_dev(self.h, num_words, q_bits.shape[0], _t(q_bits), db_bits.shape[0], _t(db_bits),
                                       _t(counts)), "lcd_overlap")

    def lcd_best(self, num_words, q_bits, db_bits, limit, best_frame, best_count, F=None):
        """Per query the best database frame f < min(limit[q], F) (lowest f on ties; (-1, 0) when
        none).  F: the rows of db_bits in use (default: all)."""
        check(lib().mv_lcd_best_dev(self.h, num_words, q_bits.shape[0], _t(q_bits),
                                    db_bits.shape[0] if F is None else F, _t(db_bits), _t(limit), _t(best_frame),
                                    _t(best_count)), "lcd_best")

    def lcd_overlap_sorted_host(self, num_words, prev_lists, cur_list):
        """lcd_main.c's shape: strictly ascending id lists of F previous frames and the current
        one -> counts [F] (sets built and compared on the device)."""
        F = len(prev_lists)
        cap = max([len(p) for p in prev_lists] + [len(cur_list), 1])
        prev_n = np.array([len(p) for p in prev_lists], np.int32)
        prev = np.full((F, cap), -1, np.int32)
        for f, p in enumerate(prev_lists):
            prev[f, :len(p)] = p
        cur = np.ascontiguousarray(cur_list, np.int32)
        counts = np.zeros(F, np.int32)
        check(lib().mv_lcd_overlap_sorted_host(self.h, num_words, F, cap, _np(prev_n), _np(prev), cur.size, _np(cur),
                                               _np(counts)), "lcd_overlap_sorted_host")
        return counts


# ---------------- loop closure: vocabulary and place database ----------------
VOCABULARY_FIELDS = ("num_base", "words_per_base", "scale", "bias", "base_desc", "leaf")


def word_set_stride(num_words):
    """uint32 words per bitset row (a multiple of 4: rows are read 128 bits at a time)."""
    return lib().mv_word_set_stride(int(num_words))


def _c_int(tok):
    t = tok.strip().lower()
    return int(t[2:], 2) if t.startswith("0b") else int(t)


def vocabulary_from_header(path):
    """The arrays of a vocabulary.h-format header (include/data/LCD/vocabulary.h: `const T
    name[dims] = {literals};` with decimal and 0b... literals) as a dict of VOCABULARY_FIELDS.
    A text parser of the data format only -- nothing is compiled or executed.  Integer literals
    wrap to the declared type as a C compiler wraps them (int8_t 243 -> -13)."""
    import re

    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    decl = {}
    for m in re.finditer(r"const\s+(\w+)\s+(\w+)\s*((?:\[\s*\d+\s*\])*)\s*=\s*([^;]*);", src):
        ctype, name, dims, body = m.groups()
        shape = tuple(int(d) for d in re.findall(r"\d+", dims))
        toks = [t for t in re.split(r"[\s,{}]+", body) if t]
        if ctype == "float":
            val = np.array([float(t.rstrip("fF")) for t in toks], np.float64).astype(np.float32)
        else:
            val = np.array([_c_int(t) for t in toks], np.int64)
        n = int(np.prod(shape)) if shape else 1
        if val.size != n:
            raise MVError("%s: %d values for shape %s" % (name, val.size, shape))
        decl[name] = val.reshape(shape) if shape else val.reshape(())
    need = ("num_base_nodes", "scale_arr", "bias_arr", "base_descriptors", "words_per_base_node", "leaf_descriptors")
    for k in need:
        if k not in decl:
            raise MVError("%s: no %s" % (path, k))
    nb, wpb = int(decl["num_base_nodes"]), int(decl["words_per_base_node"])
    out = {"num_base": np.int32(nb), "words_per_base": np.int32(wpb),
           "scale": decl["scale_arr"].astype(np.float32), "bias": decl["bias_arr"].astype(np.float32),
           "base_desc": (decl["base_descriptors"] & 0xFF).astype(np.uint8).view(np.int8),
           "leaf": (decl["leaf_descriptors"] & 0xFFFFFFFF).astype(np.uint32)}
    if (out["scale"].shape != (nb,) or out["bias"].shape != (nb,) or out["base_desc"].shape != (256, nb)
            or out["leaf"].shape != (nb, wpb, 4)):
        raise MVError("%s: array shapes do not fit num_base_nodes = %d, words_per_base_node = %d" % (path, nb, wpb))
    return out


class Vocabulary:
    """A vocabulary on the device (mv_vocabulary_*): owns the handle, close() / __del__ like SuperPoint."""

    def __init__(self, ctx, arrays):
        self.num_base, self.words_per_base = int(arrays["num_base"]), int(arrays["words_per_base"])
        self.num_words = self.num_base * self.words_per_base
        sc = np.ascontiguousarray(arrays["scale"], np.float32)
        bi = np.ascontiguousarray(arrays["bias"], np.float32)
        bd = np.ascontiguousarray(arrays["base_desc"], np.int8)
        lf = np.ascontiguousarray(arrays["leaf"], np.uint32)
        if (sc.shape != (self.num_base,) or bi.shape != (self.num_base,) or bd.shape != (256, self.num_base)
                or lf.shape != (self.num_base, self.words_per_base, 4)):
            raise MVError("vocabulary: array shapes do not fit num_base / words_per_base")
        h = _P()
        check(lib().mv_vocabulary_create(ctx.h, self.num_base, self.words_per_base, _np(sc), _np(bi), _np(bd), _np(lf),
                                         ctypes.byref(h)), "vocabulary_create")
        self.h, self.ctx = h, ctx

    def close(self):
        if self.h:
            lib().mv_vocabulary_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_vocabulary(npz_path):
    """dict of VOCABULARY_FIELDS from an .npz of that layout (tests/golden/vocabulary.npz)."""
    d = np.load(npz_path, allow_pickle=False)
    return {k: d[k] for k in VOCABULARY_FIELDS}


class PlaceDatabase:
    """A preallocated device ring of frame word sets [capacity][stride]: add(bits_row) -> index,
    query(bits, min_gap) -> (best_frame, best_count) among the frames added at least min_gap
    before the newest (limit = size - min_gap).  Runs on the context's current stream."""

    def __init__(self, ctx, num_words, capacity):
        import torch

        self.ctx, self.num_words, self.capacity = ctx, int(num_words), int(capacity)
        self.stride = word_set_stride(num_words)
        if self.stride <= 0 or self.capacity <= 0:
            raise MVError("PlaceDatabase: num_words and capacity must be positive")
        self.dev = torch.device("cuda:%d" % ctx.device)
        self.bits = torch.zeros((self.capacity, self.stride), dtype=torch.int32, device=self.dev)
        self.size = 0
        self._limit = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._best = torch.zeros(2, dtype=torch.int32, device=self.dev)

    def _stream(self):
        import torch

        h = lib().mv_context_stream(self.ctx.h)  # None: HIP's null stream, torch's default stream
        return torch.cuda.ExternalStream(h, device=self.dev) if h else torch.cuda.default_stream(self.dev)

    def add(self, bits_row):
        import torch

        if self.size >= self.capacity:
            raise MVError("PlaceDatabase is full (%d frames)" % self.capacity)
        with torch.cuda.stream(self._stream()):
            self.bits[self.size].copy_(bits_row.reshape(self.stride), non_blocking=True)
        self.size += 1
        return self.size - 1

    def query(self, bits, min_gap=0):
        import torch

        if self.size == 0:
            return -1, 0
        q = bits.reshape(1, self.stride)
        with torch.cuda.stream(self._stream()):
            self._limit.fill_(self.size - int(min_gap))
            self.ctx.lcd_best(self.num_words, q, self.bits, self._limit, self._best[0:1], self._best[1:2],
                              F=self.size)
            bf, bc = self._best.cpu().tolist()
        return bf, bc


# ---------------- quantized SuperPoint front-end (include/superpoint.h) ----------------
SP_LAYERS = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b",
             "convPa", "convPb", "convDa", "convDb")


def superpoint_weights(src):
    """Weights dict (<layer>_w, <layer>_bias, <layer>_meta = [w_scale, w_zp, out_scale, out_zp],
    input_scale) from the reference's TorchScript archive (read without unpickling or running it:
    sp_weights.load_superpoint), from an .npz of that layout, or from such a dict."""
    if isinstance(src, dict):
        return src
    if str(src).endswith(".npz"):
        return dict(np.load(src, allow_pickle=False))
    import sp_weights

    L = sp_weights.load_superpoint(src)
    out = {"input_scale": np.float64(L["input"]["scale"])}
    for n in SP_LAYERS:
        d = L[n]
        if d["w_zp"] != 0 or d["out_zp"] != 0:
            raise MVError("%s: non-zero zero points are not supported" % n)
        out[n + "_w"], out[n + "_bias"] = d["w"], d["bias"]
        out[n + "_meta"] = np.array([d["w_scale"], d["w_zp"], d["out_scale"], d["out_zp"]], np.float64)
    return out


class SuperPoint:
    """The quantized SuperPoint network on the GPU (mv_superpoint_*): uint8 frames [B][H][W] ->
    Frame-layout int8 semi [B][cells][65], desc [B][cells][256] and their run() scales."""

    def __init__(self, ctx, weights):
        W = superpoint_weights(weights)
        sw = SpWeights()
        sw.in_scale = float(W["input_scale"])
        keep = []
        for i, n in enumerate(SP_LAYERS):
            w = np.ascontiguousarray(W[n + "_w"], np.int8)
            b = np.ascontiguousarray(W[n + "_bias"], np.float32)
            meta = W[n + "_meta"]
            keep += [w, b]
            L = sw.layer[i]
            L.w, L.bias = w.ctypes.data, b.ctypes.data
            L.cout, L.cin, L.k = w.shape[0], w.shape[1], w.shape[2]
            L.w_scale, L.out_scale = float(meta[0]), float(meta[2])
        h = _P()
        check(lib().mv_superpoint_create(ctx.h, ctypes.byref(sw), ctypes.byref(h)), "superpoint_create")
        self.h, self.ctx = h, ctx

    def close(self):
        if self.h:
            lib().mv_superpoint_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, images, oh=192, ow=640, out=None, ctx=None):
        """images: torch uint8 [B][H][W] on the context's device; returns (semi, desc,
        semi_scale, desc_scale) torch tensors (or fills `out`, the same four).  ctx: run on another
        context's stream (default: the one the net was created with)"""
        import torch

        B, H, W = images.shape
        cells = (oh // 8) * (ow // 8)
        if out is None:
            dev = images.device
            out = (torch.empty((B, cells, 65), dtype=torch.int8, device=dev),
                   torch.empty((B, cells, 256), dtype=torch.int8, device=dev),
                   torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
        semi, desc, ss, ds = out
        check(lib().mv_superpoint_forward_dev((ctx or self.ctx).h, self.h, B, H, W, oh, ow, _t(images), _t(semi), _t(desc),
                                              _t(ss), _t(ds)), "superpoint_forward")
        return semi, desc, ss, ds

    def forward_raw(self, images, oh=192, ow=640, out=None, ctx=None):
        """images: torch uint8 [B][H][W] -> the network's float outputs as pairwise_pnp.py's
        run() receives them (semi [B, 65, oh/8, ow/8], coarse_desc [B, 256, oh/8, ow/8] float32
        NCHW: code x the head's output scale), the input of Context.keypoints"""
        import torch

        B, H, W = images.shape
        hc, wc = oh // 8, ow // 8
        if out is None:
            dev = images.device
            out = (torch.empty((B, 65, hc, wc), dtype=torch.float32, device=dev),
                   torch.empty((B, 256, hc, wc), dtype=torch.float32, device=dev))
        semi, cdesc = out
        check(lib().mv_superpoint_forward_raw_dev((ctx or self.ctx).h, self.h, B, H, W, oh, ow, _t(images),
                                                  _t(semi), _t(cdesc)), "superpoint_forward_raw")
        return semi, cdesc


class SuperPointFrontend:
    """Mirror of SuperPointFrontend (python/superpoint_inference.py:86-208) on the GPU: the
    network from the same archive (read without unpickling), run() on one frame.  run() takes the
    8-bit grayscale frame as decoded (the driver's / 255 and resize to 192 x 640,
    superpoint_inference.py:613-628, happen on the GPU) and returns run()'s
    (scale0, q_outs0 [1, 65, Hc, Wc], scale1, q_outs1 [1, 256, Hc, Wc], None): the int8 codes as
    torch int32 tensors like the reference's .int(); the float network outputs are not kept."""

    def __init__(self, weights_path, nms_dist=4, conf_thresh=0.015, nn_thresh=0.7, cuda=True, ctx=None, size=(192, 640)):
        self.name = "SuperPoint"
        self.nms_dist, self.conf_thresh, self.nn_thresh = nms_dist, conf_thresh, nn_thresh
        self.cell, self.border_remove = 8, 4
        self.ctx = ctx or Context(0)
        self.net = SuperPoint(self.ctx, weights_path)
        self.size = size

    def run(self, img):
        import torch

        img = torch.as_tensor(np.ascontiguousarray(img, np.uint8)).cuda()
        oh, ow = self.size
        stream = torch.cuda.current_stream()
        self.ctx.set_stream(stream)
        semi, desc, ss, ds = self.net.forward(img[None], oh, ow)
        torch.cuda.synchronize()
        hc, wc = oh // 8, ow // 8
        q0 = semi[0].view(wc, hc, 65).permute(2, 1, 0)[None].int()
        q1 = desc[0].view(wc, hc, 256).permute(2, 1, 0)[None].int()
        return float(ss[0].item()), q0, float(ds[0].item()), q1, None
