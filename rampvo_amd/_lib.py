"""ctypes binding of libramp_hip.so (C ABI declared in include/ramp_hip.h).

There is no CPU fallback: every operator of this package runs its HIP kernel
or raises.  ``lib()`` raises ``RuntimeError`` if the shared library has not been
built (``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C rampvo_amd/csrc``).
"""
import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("RAMP_HIP_LIB") or os.path.join(CSRC, "libramp_hip.so")   # env: kernel A/B builds

RAMP_F32, RAMP_F16 = 0, 1
RAMP_EUNSUPPORTED = -4
RAMP_CONV_FP8 = 0x40
RAMP_IN_F32, RAMP_CONV_DIRECT, RAMP_CORR_MFMA32, RAMP_CORR_X2 = 0x10, 0x20, 0x40, 0x80
RAMP_CONV_X3 = 0x80
RAMP_TILE_FP8, RAMP_TILE_TAIL, RAMP_TILE_SINGLE, RAMP_TILE_PAIRED = 1, 2, 4, 8
RAMP_NCHW, RAMP_NHWC, RAMP_NHWC32 = 0, 1, 2
RAMP_INTERP_EXTRAPOLATE, RAMP_INTERP_ROW_STORES, RAMP_INTERP_BAD_TIMES = 1, 2, 1
RAMP_WARP_DEPTH_SCALAR, RAMP_WARP_DEPTH_MAP, RAMP_WARP_IDENTITY, RAMP_WARP_MIN_Z = 0, 4, 8, 0.2
RAMP_DEPTHMAP_CONF_IS_VARIANCE, RAMP_DEPTHMAP_PRIOR_RELATIVE, RAMP_DEPTHMAP_BAD_CAM = 1, 2, 1
RAMP_CONTRAST_UNSIGNED, RAMP_CONTRAST_BAD_CORRECTION = 16, 2
RAMP_ALIGN_ITERS, RAMP_ALIGN_STALLED, RAMP_ALIGN_FLAT, RAMP_ALIGN_BUDGET = 1, 2, 3, 4
RAMP_ALIGN_MAX_ITERS, RAMP_ALIGN_TRIALS = 65536, 9
RAMP_VOXEL_NORMALIZE, RAMP_VOXEL_SUBPIXEL, RAMP_VOXEL_BAD_OFFSETS, RAMP_VOXEL_BAD_TIMES = 1, 2, 1, 2
# the camera record of csrc/rectify.hip: word offsets, models, flags, value modes
RAMP_CAMERA_WORDS, RAMP_CAMERA_RAW, RAMP_CAMERA_MODEL, RAMP_CAMERA_COEFFS, RAMP_CAMERA_ROTATION, RAMP_CAMERA_NEW = 32, 0, 4, 5, 12, 24
RAMP_CAM_PINHOLE, RAMP_CAM_RADTAN, RAMP_CAM_EQUIDISTANT = 0, 1, 2
RAMP_RECTIFY_ITERS, RAMP_RECTIFY_TOL = 8, 2.0 ** -6
RAMP_RECTIFY_XY_I32, RAMP_RECTIFY_SRC_U8, RAMP_RECTIFY_BAD_CAMERA = 1, 2, 1
RAMP_RECTIFY_NORM_NONE, RAMP_RECTIFY_NORM_HALF, RAMP_RECTIFY_NORM_UNIT = 0, 1, 2
RAMP_FILTER_XY_I32, RAMP_FILTER_BAD_ORDER = 1, 1
RAMP_IMU_F64, RAMP_IMU_PREINT_WORDS, RAMP_IMU_MAX_GYRO_STEPS = 1, 24, 16
RAMP_IMU_BAD_ORDER, RAMP_IMU_GYRO_FAILED, RAMP_IMU_SCALE_FAILED = 1, 2, 4
RAMP_IMU_FEW_TRIPLES, RAMP_IMU_SINGULAR, RAMP_IMU_BAD_SCALE = 8, 16, 32
RAMP_IMU_ANCHOR_WORDS, RAMP_IMU_BAD_ANCHOR, RAMP_IMU_NO_START = 24, 64, 128
KPLANE = 32            # channels per plane of the packed correlation target maps: [h][128 / KPLANE][w][KPLANE]


def kplane(dtype):
    """channels per plane of the packed correlation target maps for a feature dtype: 64 bytes per pixel and plane
    ([h][4][w][32] fp16, [h][8][w][16] fp32).  fp32 features in the split form (corr_f32_mode() == 2) keep the fp32 CONTAINER
    [h][8][w][16] float32 -- the same 512 bytes per pixel -- whose bytes are [h][4][2][w][32] fp16 parts (RAMP_CORR_X2)"""
    import torch
    return KPLANE if dtype == torch.float16 else KPLANE // 2


def corr_f32_mode():
    """how the tracker computes the correlation volume of fp32 features (RAMP_CORR_F32_MFMA, switches.read()): 2 (default)
    split fp16 pairs on the f16 matrix cores (corr_mfma_kernel<CorrX2>, chunked planes of pairs); 1 the fp32 matrix cores
    (corr_mfma_kernel<float>, chunked fp32 planes); 0 corr_kernel<float>, the reference kernel's summation order, plain planes"""
    from . import switches
    return switches.read().corr_f32_mfma

_ERR = {-1: "RAMP_EINVAL (bad argument)", -2: "RAMP_ELAUNCH (HIP launch/runtime error)",
        -3: "RAMP_EWORKSPACE (workspace too small)", -4: "RAMP_EUNSUPPORTED (size/shape not supported)"}

c_p, c_i, c_i64, c_sz, c_f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float


class CorrLevel(ctypes.Structure):
    _fields_ = [("fmap", c_p), ("H2", c_i), ("W2", c_i), ("coord_div", c_f)]


def _ptr_fields(names):
    return [(n, c_p) for n in names]


class TrackWeights(ctypes.Structure):
    """ramp_track_weights"""
    _fields_ = (_ptr_fields(["corr_w1", "corr_w2", "corr_w3", "corr_b1", "corr_b2", "corr_b3", "corr_ln_w", "corr_ln_b",
                             "norm_w", "norm_b", "c1_wa", "c1_wb", "c2_wa", "c2_wb", "c1_ba", "c1_bb", "c2_ba", "c2_bb",
                             "kk_wf", "kk_wg", "kk_wh", "ij_wf", "ij_wg", "ij_wh", "kk_bf", "kk_bg", "kk_bh", "ij_bf",
                             "ij_bg", "ij_bh", "ln1_w", "ln1_b", "ln2_w", "ln2_b"])
                + [("gru_w", c_p * 6), ("gru_b", c_p * 6), ("heads_w", c_p), ("heads_b", c_p)]
                + [(n, c_f) for n in ("corr_ln_eps", "norm_eps", "ln1_eps", "ln2_eps")])


class UpdateArgs(ctypes.Structure):
    """ramp_update_args"""
    _fields_ = ([("w", ctypes.POINTER(TrackWeights))]
                + _ptr_fields(["corr", "net_prev", "net_map", "inp", "inp_idx"]) + [("inp_mod", ctypes.c_long), ("state", c_p * 2)]
                + _ptr_fields(["net_out", "relu_out", "coords", "target", "weight", "kk_order", "kk_gid", "kk_seg",
                               "kk_ngroups", "ij_order", "ij_gid", "ij_seg", "ij_ngroups", "ix", "jx", "sagg_frag", "fg",
                               "ykk", "yij", "hkk", "hij"])
                + [(n, c_i) for n in ("kk_cap", "ij_cap", "E", "E_hint", "P", "fp32")] + [("wd", c_f), ("ht", c_f)])


# name -> (restype, argtypes); also the list the CPU test checks for export
SIGNATURES = {
    "ramp_version": (ctypes.c_char_p, []),
    "ramp_corr_kplane": (c_i, []),
    "ramp_patchify_fwd": (c_i, [c_p, c_p, c_p] + [c_i] * 10 + [c_p]),
    "ramp_frame_gather": (c_i, [c_p] * 9 + [c_i] * 8 + [c_p]),
    "ramp_corr_fwd": (c_i, [c_p, ctypes.POINTER(CorrLevel), c_i, c_p, c_p, c_p, c_p] + [c_i] * 8 + [c_p]),
    "ramp_ms_lstm_superstate": (c_i, [c_p, c_p, ctypes.POINTER(c_p), c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "ramp_ms_lstm_superstate_mfma": (c_i, [c_p] * 6 + [c_i] * 5 + [c_p]),
    "ramp_conv2d_stats_blocks": (c_i, [c_i] * 7),
    "ramp_conv2d_tiled": (c_i, [c_i] * 5),
    "ramp_conv2d_tile_rows": (c_i, []),
    "ramp_conv2d_tile_row": (c_i, [c_i] + [ctypes.POINTER(c_i)] * 7),
    "ramp_conv2d_multi_row": (c_i, [c_p] + [c_i] * 7),
    "ramp_graph_edit_host": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_p]),
    "ramp_event_stack_workspace_bytes": (c_sz, [c_i, c_i, c_i]),
    "ramp_event_stack": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_sz, c_p]),
    "ramp_depth_median_fill": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    "ramp_depth_median": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    "ramp_depth_median_rows": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p]),
    "ramp_event_topk_workspace_bytes": (c_sz, [c_i, c_i]),
    "ramp_event_topk": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_sz, c_p]),
    "ramp_pyramid_pack": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "ramp_corr_fwd_ordered": (c_i, [c_p, ctypes.POINTER(CorrLevel), c_i, c_p, c_p, c_p, c_p, c_p, c_i, ctypes.c_long,
                                    ctypes.c_long] + [c_i] * 8 + [c_p]),
    "ramp_se3_exp": (c_i, [c_p, c_p, c_i, c_p]),
    "ramp_se3_log": (c_i, [c_p, c_p, c_i, c_p]),
    "ramp_se3_inv": (c_i, [c_p, c_p, c_i, c_p]),
    "ramp_se3_mul": (c_i, [c_p, c_p, c_p, c_i, c_p]),
    "ramp_se3_act4": (c_i, [c_p, c_p, c_p, c_i, c_p]),
    "ramp_se3_adj": (c_i, [c_p, c_p, c_p, c_i, c_p]),
    "ramp_se3_adjT": (c_i, [c_p, c_p, c_p, c_i, c_p]),
    "ramp_transform": (c_i, [c_p] * 7 + [c_i, c_i, c_i, c_p]),
    "ramp_reproject": (c_i, [c_p] * 7 + [c_i, c_i, c_p]),
    "ramp_point_cloud": (c_i, [c_p] * 5 + [c_i, c_i, c_p]),
    "ramp_multi_copy": (c_i, [c_p, c_p, c_p, c_i, c_p]),
    "ramp_shift_rows": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "ramp_motionmag": (c_i, [c_p] * 10 + [c_i64, c_i64, c_f, c_p, c_i, c_p]),
    "ramp_motion_model": (c_i, [c_p, c_i, c_f, c_p]),
    "ramp_frame_commit": (c_i, [c_p, c_i, c_i, c_f, c_p, c_i64, c_p, c_i64, c_p, c_i, c_p, c_i, c_i, c_i, c_p, c_i,
                                ctypes.POINTER(c_p), ctypes.POINTER(c_p), ctypes.POINTER(ctypes.c_long), c_p, c_p]),
    "ramp_frame_begin": (c_i, [c_p, c_i, c_i, c_f, c_p, c_i64, c_p, c_i64, c_p, c_i, c_p]),
    "ramp_group_by_workspace_bytes": (c_sz, [c_i]),
    "ramp_group_by": (c_i, [c_p, c_i, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "ramp_neighbors_workspace_bytes": (c_sz, [c_i]),
    "ramp_neighbors": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i64, c_i64, c_p, c_sz, c_p]),
    "ramp_segment_softmax_sum": (c_i, [c_p] * 6 + [c_i, c_i, c_i, c_i, c_p]),
    "ramp_ba_workspace_bytes": (c_sz, [c_i] * 5),
    "ramp_ba_forward": (c_i, [c_p] * 9 + [c_i] * 7 + [c_p, c_sz, c_p, c_p]),
    "ramp_ba_planned_workspace_bytes": (c_sz, [c_i] * 7),
    "ramp_ba_forward_planned": (c_i, [c_p] * 9 + [c_i] * 7 + [c_p] * 4 + [c_i] + [c_p] * 3 + [c_i, c_p, c_sz, c_p, c_p]),
    "ramp_ba_covariance_workspace_bytes": (c_sz, [c_i] * 5),
    "ramp_ba_covariance": (c_i, [c_p] * 9 + [c_i] * 6 + [c_p] * 3 + [c_p, c_sz, c_p, c_p]),
    "ramp_ba_covariance_planned_workspace_bytes": (c_sz, [c_i] * 7),
    "ramp_ba_covariance_planned": (c_i, [c_p] * 9 + [c_i] * 6 + [c_p] * 3 + [c_p] * 4 + [c_i] + [c_p] * 3
                                   + [c_i, c_p, c_sz, c_p, c_p]),
    "ramp_ba_map_covariance_workspace_bytes": (c_sz, [c_i] * 5),
    "ramp_ba_map_covariance": (c_i, [c_p] * 9 + [c_i] * 6 + [c_p] * 7 + [c_p, c_sz, c_p, c_p]),
    "ramp_ba_map_covariance_planned_workspace_bytes": (c_sz, [c_i] * 7),
    "ramp_ba_map_covariance_planned": (c_i, [c_p] * 9 + [c_i] * 6 + [c_p] * 7 + [c_p] * 4 + [c_i] + [c_p] * 3
                                       + [c_i, c_p, c_sz, c_p, c_p]),
    "ramp_map_select": (c_i, [c_p] * 4 + [c_i, c_i, c_p, c_i, c_f, c_f, c_i, c_p, c_p, c_p]),
    "ramp_group_by_small_workspace_bytes": (c_sz, [c_i, c_i]),
    "ramp_group_by_small": (c_i, [c_p, c_p, c_i64, c_i64, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_sz, c_p]),
    "ramp_neighbors_from_groups": (c_i, [c_p] * 7 + [c_i, c_i, c_p]),
    "ramp_any_nonzero": (c_i, [c_p, ctypes.c_long, c_p, ctypes.c_long, c_p, c_p]),
    "ramp_lstm_superstate_tiled": (c_i, [c_p] * 9 + [c_i, c_i, c_i, c_p]),
    "ramp_lstm_superstate_blocks": (c_i, [c_p] * 9 + [c_i, c_i, c_i, c_i, c_p]),
    "ramp_any_nonzero_blocks": (c_i, [c_p, ctypes.c_long, c_p, ctypes.c_long, c_p, c_p]),
    "ramp_any_nonzero_blocks_clear": (c_i, [c_p, ctypes.c_long, c_p, ctypes.c_long, c_p, c_p, ctypes.c_long, c_p]),
    "ramp_conv2d_nhwc": (c_i, [c_p] * 8 + [c_i] * 8 + [c_f, c_i, c_p]),
    "ramp_in_stats_finalize": (c_i, [c_p, c_i, c_i, c_f, c_f, c_p, c_p, c_p]),
    "ramp_affine_relu": (c_i, [c_p, c_p, c_p, c_p, ctypes.c_long, c_i, c_p]),
    "ramp_norm_add_relu": (c_i, [c_p] * 7 + [ctypes.c_long, c_i, c_p]),
    "ramp_affine_relu_f16": (c_i, [c_p, c_p, c_p, c_p, ctypes.c_long, c_i, c_p]),
    "ramp_norm_add_relu_f16": (c_i, [c_p] * 7 + [ctypes.c_long, c_i, c_i, c_p]),
    "ramp_norm_add_relu_f16_acc": (c_i, [c_p, c_p, c_f, c_f, c_p, c_p, c_f, c_f, c_p, ctypes.c_long, c_i, c_i, c_p]),
    "ramp_in_acc_finalize": (c_i, [c_p, c_i, c_f, c_f, c_p, c_p, c_p]),
    "ramp_conv2d_nhwc_multi": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "ramp_upd_row_fuse": (c_i, [c_p] * 6 + [ctypes.c_long, c_p, c_p, c_p, c_p, c_f, c_i, c_p, c_p, c_i, c_i, c_p]),
    "ramp_upd_gather_mask": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p]),
    "ramp_upd_gated": (c_i, [c_p] * 5 + [c_f, c_p, c_p, c_p, c_i, c_i, c_p]),
    "ramp_upd_heads": (c_i, [c_p] * 5 + [c_i, c_i, c_f, c_f, c_i, c_p]),
    "ramp_upd_segment_softmax": (c_i, [c_p] * 5 + [c_i, c_i, c_p]),
    "ramp_upd_corr_mlp": (c_i, [c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, ctypes.c_long,
                                c_p, c_p, c_f, c_p, c_i, c_p]),
    "ramp_upd_heads_linear": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_f, c_p]),
    "ramp_upd_fg": (c_i, [c_p] * 9 + [c_i, c_p]),
    "ramp_upd_gru": (c_i, [c_p, c_p, c_p, c_p, c_p, c_f, ctypes.POINTER(c_p), ctypes.POINTER(c_p), c_p, c_p, c_f, c_p,
                           c_p, c_i, c_p]),
    "ramp_upd_gru_heads": (c_i, [c_p, c_p, c_p, c_p, c_p, c_f, ctypes.POINTER(c_p), ctypes.POINTER(c_p), c_p, c_p, c_f, c_p,
                                 c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_f, c_p]),
    "ramp_upd_gru_tile_rows": (c_i, [c_i, c_i]),
    "ramp_upd_mlp_lds_bytes": (c_sz, []),
    "ramp_upd_nbr": (c_i, [c_p] * 8 + [c_i, c_p]),
    "ramp_upd_linear": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_p]),
    "ramp_upd_softagg_frag_rows": (c_sz, [c_i, c_i]),
    "ramp_upd_softagg": (c_i, [c_p] * 10 + [c_i, c_p]),
    "ramp_upd_softagg_finish": (c_i, [c_p] * 6 + [c_i, c_p]),
    # the update operator at fp32 accuracy on the f16 matrix cores (csrc/update_x3.hip)
    "ramp_x3_corr_mlp": (c_i, [c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, ctypes.c_long,
                               c_p, c_p, c_f, c_p, c_i, c_p]),
    "ramp_x3_nbr": (c_i, [c_p] * 7 + [c_i, c_p]),
    "ramp_x3_fg": (c_i, [c_p] * 9 + [c_i, c_p]),
    "ramp_x3_segment_softmax": (c_i, [c_p] * 5 + [c_i, c_p]),
    "ramp_x3_linear": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_p]),
    "ramp_x3_gru": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f, ctypes.POINTER(c_p), ctypes.POINTER(c_p), c_p, c_p, c_f,
                          c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_f, c_f, c_p]),
    # the whole operator as one call (csrc/update_op.hip)
    "ramp_update_forward": (c_i, [ctypes.POINTER(UpdateArgs), c_p]),
    # device-resident tracking step (csrc/track.hip); the ramp_track descriptor is mirrored in track_dev.py
    "ramp_track_sizeof": (c_sz, []),
    "ramp_track_plan_workspace_bytes": (c_sz, [c_i, c_i, c_i]),
    "ramp_track_ba_workspace_bytes": (c_sz, [c_i] * 6),
    "ramp_track_plan": (c_i, [c_p, c_i, c_p]),
    "ramp_track_step": (c_i, [c_p, c_i, c_i64, c_i, c_i, c_p, c_p, c_p]),
    "ramp_track_warm": (c_i, [c_p, c_p, c_p]),
    "ramp_stream_delay": (c_i, [c_i, c_p]),
    "ramp_signal_alloc": (c_i, [c_p]),
    "ramp_signal_free": (c_i, [c_p]),
    "ramp_stream_signal": (c_i, [c_p, c_p, ctypes.c_uint32]),
    "ramp_stream_wait_flag": (c_i, [c_p, c_p, ctypes.c_uint32, c_i, c_i, c_p]),
    "ramp_host_device_pointer": (c_i, [c_p, c_p]),
    # live poses (csrc/publish.hip); the record layout is mirrored in track_dev.py
    "ramp_track_publish": (c_i, [c_p, c_i64, ctypes.c_double, c_p, c_i, c_p, c_p] + [c_i] * 8 + [c_p]),
    "ramp_track_uncertainty_workspace_bytes": (c_sz, [c_p]),
    "ramp_track_uncertainty": (c_i, [c_p, c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "ramp_track_map_workspace_bytes": (c_sz, [c_p]),
    "ramp_track_map": (c_i, [c_p, c_i] + [c_p] * 7 + [c_p, c_sz, c_p]),
    "ramp_trajectory_resolve": (c_i, [c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p]),
    # poses at any time (csrc/interp.hip)
    "ramp_se3_interp_workspace_bytes": (c_sz, [c_i]),
    "ramp_se3_interp_lds_knots": (c_i, []),
    "ramp_se3_interp": (c_i, [c_p, c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_sz, c_p, c_p]),
    # motion-compensated events (csrc/warp.hip)
    "ramp_event_warp_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i]),
    "ramp_event_warp_grid_events": (ctypes.c_long, []),
    "ramp_event_warp": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_i, ctypes.c_double, c_p, c_p, c_i, c_i, c_i, c_i,
                              c_p, c_p, c_p, c_p, c_p, c_sz, c_p, c_p]),
    # inverse-depth map from the window's patches (csrc/depthmap.hip)
    "ramp_invdepth_map_workspace_bytes": (c_sz, [c_i]),
    "ramp_invdepth_map_stage_records": (c_i, []),
    "ramp_invdepth_map": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_p, c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_f, c_f,
                                c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_sz, c_p, c_p]),
    # event contrast and its gradient (csrc/contrast.hip)
    "ramp_event_contrast_workspace_bytes": (c_sz, [c_i, c_i, c_i]),
    "ramp_event_contrast": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_i, ctypes.c_double, c_p, c_p, c_p, c_i, c_i, c_i,
                                  c_p, c_p, c_p, c_p, c_p, c_sz, c_p, c_p]),
    "ramp_event_align_workspace_bytes": (c_sz, [c_i, c_i, c_i]),
    "ramp_event_align": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_i, ctypes.c_double, c_p, c_p, c_p, c_i, c_i, c_i,
                               c_i, ctypes.c_double, c_i, c_i] + [c_p] * 7 + [c_p, c_sz, c_p]),
    # event voxel grids (csrc/voxel.hip)
    "ramp_event_voxel_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i]),
    "ramp_event_voxel_grid_events": (ctypes.c_long, []),
    "ramp_event_voxel_lds_offsets": (c_i, []),
    "ramp_event_voxel": (c_i, [c_p, c_p, c_p, c_p, ctypes.c_long, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    # lens distortion (csrc/rectify.hip)
    "ramp_event_rectify_grid_events": (ctypes.c_long, []),
    "ramp_event_rectify": (c_i, [c_p, c_p, ctypes.c_long, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "ramp_image_rectify": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_f, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    # event denoising (csrc/filter.hip)
    "ramp_event_filter_workspace_bytes": (c_sz, [ctypes.c_long, c_i, c_i]),
    "ramp_event_filter_grid_events": (ctypes.c_long, []),
    "ramp_event_filter": (c_i, [c_p, c_p, c_p, ctypes.c_long, c_i, c_i, c_i, ctypes.c_double, ctypes.c_double, c_i,
                                ctypes.c_double] + [c_p] * 11 + [c_sz, c_p]),
    # IMU preintegration and alignment (csrc/imu.hip)
    "ramp_imu_workspace_bytes": (c_sz, [ctypes.c_long, c_i]),
    "ramp_imu_preintegrate": (c_i, [c_p, c_p, c_p, ctypes.c_long, c_p, c_i, c_i, c_p, c_p, ctypes.c_double, c_i, c_p, c_p, c_p]),
    "ramp_imu_align": (c_i, [c_p, c_p, c_p, ctypes.c_long, c_p, c_p, c_i, c_i, c_p, c_p, c_p, ctypes.c_double, ctypes.c_double,
                             c_i, c_i] + [c_p] * 7 + [c_sz, c_p]),
    # IMU propagation (csrc/imu_propagate.hip)
    "ramp_imu_propagate_workspace_bytes": (c_sz, [ctypes.c_long]),
    "ramp_imu_propagate": (c_i, [c_p, c_p, c_p, ctypes.c_long, c_p, c_p, c_p, ctypes.c_double, ctypes.c_double, c_i] + [c_p] * 5
                           + [c_sz, c_p]),
}

_lib = None


def build(force=False, jobs=8):
    """compile every HIP source for gfx950 into csrc/libramp_hip.so"""
    cmd = ["make", "-s", "-C", CSRC, "-j%d" % jobs]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd + ["libramp_hip.so"])
    return LIB_PATH


def register_optional(extra):
    """late registration of signatures for optional translation units"""
    SIGNATURES.update(extra)
    if _lib is not None:
        for name, (res, args) in extra.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = res, args


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "rampvo_amd: %s is missing -- the HIP extension is not built and there is no "
                "CPU fallback (run __graft_entry__.build())" % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        if l.ramp_corr_kplane() != KPLANE:      # (an older library given through RAMP_HIP_LIB: this binding would pack the planes wrong)
            raise RuntimeError("rampvo_amd: %s packs %d-channel correlation planes, this binding is written for %d "
                               "(the library is older than this binding: rebuild it from csrc/)" % (LIB_PATH, l.ramp_corr_kplane(), KPLANE))
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, _ERR.get(rc, "status %d" % rc)))


def stream():
    """the current HIP stream of the current device as a void* (raw getter: this is called ~30x per frame)"""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("rampvo_amd operators run on the GPU only (got a %s tensor); "
                               "there is no CPU fallback" % t.device)


def dtype_code(t):
    if t.dtype == torch.float32:
        return RAMP_F32
    if t.dtype == torch.float16:
        return RAMP_F16
    raise RuntimeError("unsupported dtype %s (float32 / float16 only)" % t.dtype)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_ws_cache = {}
_ws_retired = []
_ws_owner = [None]


class scratch_owner:
    """``with scratch_owner(obj):`` -- scratch taken inside belongs to ``obj`` as well as to the stream.  hipGraph
    captures all run on torch's one capture stream, so the stream alone would hand two captured graphs (two
    Patchifiers, a re-capture) the same scratch buffer although they replay on different streams."""

    def __init__(self, owner):
        self.owner = owner

    def __enter__(self):
        self.prev, _ws_owner[0] = _ws_owner[0], id(self.owner)

    def __exit__(self, *exc):
        _ws_owner[0] = self.prev


def workspace(nbytes, device, tag="ws"):
    """grow-only scratch buffer per (device, stream, owner, tag): two trackers on different streams of one GPU never
    share scratch, and neither do two captured graphs (see ``scratch_owner``).  Contents are never reused across
    calls.  A buffer that is outgrown is retired, not freed: launches already queued on its stream (or captured in
    a hipGraph) may still reference it."""
    key = (device, torch._C._cuda_getCurrentRawStream(device.index if device.index is not None
                                                      else torch.cuda.current_device()), _ws_owner[0], tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _ws_retired.append(buf)
        buf = torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf
