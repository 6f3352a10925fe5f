"""ctypes binding of libdepthcore.so (C ABI: include/depthcore.h).

The library is the product: there is NO fallback.  If the shared object is
missing or a tensor is not a contiguous fp32 device tensor the call raises.
"""
import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_size_t, c_uint8, c_uint32,
                    c_uint64, c_void_p)

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(_HERE, "libdepthcore.so")
# DEPTHCORE_LIB: a tuning / ablation build (tools/build_variant.sh -> build/variants/<name>/, outside the package) for the
# sweep scripts under tools/ ONLY.  bench.py, __graft_entry__.smoke() and the tests refuse to run on anything but the
# product library (IS_VARIANT).
LIB_PATH = os.environ.get("DEPTHCORE_LIB") or PRODUCT_LIB
IS_VARIANT = os.path.realpath(LIB_PATH) != os.path.realpath(PRODUCT_LIB)
MAX_SCALES = 4

OPT_NO_AUTOMASK = 1
OPT_AVG_REPROJ = 2
OPT_NO_SSIM = 4
OPT_ALIGN_CORNERS = 8
OPT_NO_GRAD = 16
OPT_PRED_MASK = 32
OPT_PHOTO_SPLIT, OPT_PHOTO_FULL = 64, 128
PREC_F32, PREC_BF16 = 0, 1
PASS_FWD, PASS_DGRAD, PASS_WGRAD = 0, 1, 2      # dc_pointwise_workspace

_ERR = {-1: "DC_EINVAL (bad shape / null pointer / unsupported option)",
        -2: "DC_ELAUNCH (hip launch failed)",
        -3: "DC_EWORKSPACE (workspace too small)",
        -4: "DC_EEMPTY (mask selects no pixel)"}
DC_EEMPTY = -4
EVAL_TRAINER, EVAL_EIGEN, EVAL_GT_POSITIVE = 0, 1, 2


class DepthcoreError(RuntimeError):
    pass


_F = c_void_p  # raw device pointers travel as void*


class PhotoDesc(Structure):
    """Mirror of `dc_photo_desc` (include/depthcore.h)."""
    _fields_ = [
        ("B", c_int32), ("H", c_int32), ("W", c_int32), ("num_scales", c_int32),
        ("flags", c_uint32), ("min_depth", c_float), ("max_depth", c_float), ("smoothness", c_float),
        ("target", _F), ("source", _F * 2), ("color_s", _F * MAX_SCALES), ("packed", _F * 3),
        ("K", _F), ("inv_K", _F), ("T", _F * 2),
        ("disp", _F * MAX_SCALES), ("noise", _F * MAX_SCALES), ("rng_seed", c_uint64), ("rng_seed_dev", _F),
        ("losses", _F), ("argmin", _F * MAX_SCALES),
        ("depth", _F * MAX_SCALES), ("sample", (_F * 2) * MAX_SCALES), ("color", (_F * 2) * MAX_SCALES),
        ("identity_selection", _F * MAX_SCALES),
        ("g_losses", _F), ("d_disp", _F * MAX_SCALES), ("d_T", _F * 2),
        ("pred_mask", _F * MAX_SCALES), ("d_pred_mask", _F * MAX_SCALES),
        ("workspace", _F), ("workspace_bytes", c_size_t),
        ("T_scale", (_F * 2) * MAX_SCALES), ("d_T_scale", (_F * 2) * MAX_SCALES),
    ]


class PhotoPlan(Structure):
    """Mirror of `dc_photo_plan` (include/depthcore.h: dc_photo_plan_query)."""
    _fields_ = [(n, c_int32) for n in ("strip_f", "strip_g", "strip_p", "strips_f", "strips_g", "strips_p",
                                       "rows_f", "rows_g", "rows_p", "rows_id",
                                       "rowblocks_f", "rowblocks_g", "rowblocks_p", "rowblocks_id",
                                       "sm_chunk", "nchunk", "full")] + \
               [(n, c_int32 * MAX_SCALES) for n in ("dg_tw", "dg_th", "dg_tiles_x", "dg_tiles_y")]


class AttnMap(Structure):
    """Mirror of `dc_attn_map`: where each input channel of an AttentionConv lives (include/depthcore.h)."""
    _fields_ = [("ptr", _F * 4), ("batch_stride", ctypes.c_longlong * 4), ("mode", c_int32 * 4)]


class AttnParams(Structure):
    """Mirror of `dc_attn_params`."""
    _fields_ = [(n, _F) for n in ("wq", "bq", "wk", "bk", "wv", "bv", "rel_h", "rel_w")]


ATTN_PLAIN, ATTN_PIXEL_SHUFFLE2 = 0, 1


class BnFold(Structure):
    """Mirror of `dc_bn_fold`: a BatchNorm folded into the passes of a neighbouring convolution (include/depthcore.h)."""
    _fields_ = [("groups", c_int32), ("in_scale", _F), ("in_shift", _F), ("stat_part", _F),
                ("bn_x", _F), ("bn_mean", _F), ("bn_mask", _F), ("bwd_part", _F)]



class DepthEvalDesc(Structure):
    """Mirror of `dc_depth_eval_desc` (include/depthcore.h: dc_depth_errors)."""
    _fields_ = [("B", c_int32), ("h", c_int32), ("w", c_int32), ("Hg", c_int32), ("Wg", c_int32), ("protocol", c_int32),
                ("crop", c_int32 * 4), ("median_scaling", c_int32), ("scale_factor", c_float), ("ratios", _F), ("status", _F)]


class PoseGroup(Structure):
    """Mirror of `dc_pose_group` (include/depthcore.h: dc_pose_head_fwd / _bwd)."""
    _fields_ = [("row0", c_int32), ("rows", c_int32), ("slot", c_int32), ("invert", c_int32)]


class Conv3x3Plan(Structure):
    """Mirror of `dc_conv3x3_plan` (include/depthcore.h: dc_conv3x3_plan_query); the values are the DC_C3_* enums there."""
    _fields_ = [(n, c_int32) for n in ("fwd", "fwd_v2", "fwd_mr", "gprime", "dx", "ring", "dw", "db", "bwd_v2", "dx_mr", "dw_mr", "split")]


class ConvS2Plan(Structure):
    """Mirror of `dc_convs2_plan` (include/depthcore.h: dc_convs2_plan_query); the values are the DC_S2_* enums there."""
    _fields_ = [(n, c_int32) for n in ("fwd", "fwd_mt", "fwd_nt", "fwd_slabs", "fwd_wpad", "dw", "dw_slabs", "dw_blocks",
                                       "dw_tiles_per_block", "dw_reduce", "dx", "dx_slabs")]


TILE_RGB, TILE_NORM, TILE_UNIT, TILE_MASK = 0, 1, 2, 3


class PanelTile(Structure):
    """Mirror of `dc_panel_tile` (include/depthcore.h: dc_log_panel)."""
    _fields_ = [("src", _F), ("src_elems", ctypes.c_longlong), ("kind", c_int32), ("panel", c_int32),
                ("h", c_int32), ("w", c_int32), ("up", c_int32), ("x0", c_int32), ("y0", c_int32), ("thr", c_int32)]


class SeqPlan(Structure):
    """Mirror of `dc_seq_plan` (include/depthcore.h: dc_data_seq_plan)."""
    _fields_ = [("lds_bytes", ctypes.c_longlong), ("table_len", ctypes.c_longlong), ("scratch_bytes", ctypes.c_longlong),
                ("n_img", c_int32), ("tail_start", c_int32)]


class GruInferLevel(Structure):
    """Mirror of `dc_gru_infer_level` (include/depthcore.h: dc_gru_infer_rh / _tail)."""
    _fields_ = [("gates", _F), ("cnm", _F), ("f", _F), ("h", _F), ("rh", _F), ("out", _F), ("C", c_int32), ("P", c_int32)]


_lib = None


def _sig(lib):
    i, f, p, z, ll = c_int, c_float, c_void_p, c_size_t, ctypes.c_longlong
    S = {
        "dc_version": (c_char_p, []),
        "dc_arch": (c_char_p, []),
        "dc_pose_matrix_fwd": (i, [p, p, i, p, i, p]),
        "dc_pose_matrix_bwd": (i, [p, p, i, p, p, p, i, p]),
        "dc_pose_head_fwd": (i, [p, i, i, i, f, p, i, p, p, p]),
        "dc_pose_head_bwd": (i, [p, i, i, i, f, p, i, p, p, p]),
        "dc_disp_to_depth_fwd": (i, [p, p, p, z, f, f, p]),
        "dc_disp_to_depth_bwd": (i, [p, p, p, p, z, f, f, p]),
        "dc_pix_coords": (i, [p, i, i, i, p]),
        "dc_backproject_fwd": (i, [p, p, p, i, i, i, p]),
        "dc_backproject_bwd": (i, [p, p, p, i, i, i, p]),
        "dc_project3d_fwd": (i, [p, p, p, p, i, i, i, f, p]),
        "dc_project3d_bwd_workspace": (z, [i, i, i]),
        "dc_project3d_bwd": (i, [p, p, p, p, p, p, p, i, i, i, f, p]),
        "dc_grid_sample_fwd": (i, [p, p, p, i, i, i, i, i, i, i, p]),
        "dc_grid_sample_bwd": (i, [p, p, p, p, i, i, i, i, i, i, i, p]),
        "dc_upsample_nearest2x_fwd": (i, [p, p, i, i, i, p]),
        "dc_upsample_nearest2x_bwd": (i, [p, p, i, i, i, p]),
        "dc_upsample_bilinear_fwd": (i, [p, p, i, i, i, i, i, p]),
        "dc_upsample_bilinear_bwd": (i, [p, p, i, i, i, i, i, p]),
        "dc_ssim_fwd": (i, [p, p, p, i, i, i, p]),
        "dc_ssim_bwd": (i, [p, p, p, p, p, i, i, i, p]),
        "dc_smooth_workspace": (z, [i, i, i]),
        "dc_smooth_fwd": (i, [p, p, p, p, i, i, i, i, p]),
        "dc_smooth_bwd": (i, [p, p, p, p, i, i, i, i, p]),
        "dc_photo_workspace": (z, [POINTER(PhotoDesc)]),
        "dc_photo_fwd": (i, [POINTER(PhotoDesc), p]),
        "dc_photo_bwd": (i, [POINTER(PhotoDesc), p]),
        "dc_photo_algorithmic_bytes": (c_double, [POINTER(PhotoDesc), i]),
        "dc_photo_plan_query": (i, [POINTER(PhotoDesc), POINTER(PhotoPlan)]),
        "dc_conv3x3_fwd_workspace": (z, [i, i, i, i, i, i]),
        "dc_conv3x3_fwd": (i, [p, i, i, p, i, p, p, p, p, i, i, i, i, i, i, p]),
        "dc_conv3x3_bwd_workspace": (z, [i, i, i, i, i, i]),
        "dc_conv3x3_bwd": (i, [p, i, i, p, i, p, p, p, p, p, p, p, p, i, i, i, i, i, i, p]),
        "dc_conv3x3_plan_query": (i, [i, i, i, i, i, i, i, i, i, i, POINTER(Conv3x3Plan)]),
        "dc_bn_workspace": (z, [i, i, i]),
        "dc_bn_mask_bytes": (z, [i, i, i]),
        "dc_bn_relu_fwd": (i, [p, p, p, p, p, p, p, p, p, p, p, i, i, i, f, f, i, i, p]),
        "dc_bn_relu_bwd": (i, [p, p, p, p, p, p, p, p, p, p, p, p, i, i, i, i, i, p]),
        "dc_bn_stat_parts": (i, [i, i, i, i, POINTER(c_int)]),
        "dc_bn_stats": (i, [p, p, i, i, i, i, p]),
        "dc_bn_finalize": (i, [p, i, i, c_double, p, p, p, p, p, p, p, p, i, i, f, f, p]),
        "dc_bn_apply": (i, [p, p, p, p, p, p, i, i, i, i, i, p]),
        "dc_bn_eval_coef": (i, [p, p, p, p, p, p, p, i, f, p]),
        "dc_bn_eval_bwd_workspace": (z, [i, i, i]),
        "dc_bn_eval_bwd": (i, [p, p, p, p, p, p, p, p, p, p, p, i, i, i, i, p]),
        "dc_depth_errors_workspace": (z, [POINTER(DepthEvalDesc)]),
        "dc_depth_errors": (i, [POINTER(DepthEvalDesc), p, p, p, p, p]),
        "dc_flip_concat": (i, [p, p, i, i, i, i, p]),
        "dc_disp_post_process": (i, [p, p, i, i, i, f, f, p]),
        "dc_depth_png16": (i, [p, p, i, i, i, i, i, f, p]),
        "dc_pose_ate": (i, [p, p, p, i, i, i, p]),
        "dc_disp_render_ws_bytes": (z, [i, i, i, i, i]),
        "dc_disp_render": (i, [p, p, p, p, i, i, i, i, i, c_double, p, z, p]),
        "dc_disp_range_pooled_ws_bytes": (z, [i, i, i, i, i]),
        "dc_disp_range_pooled": (i, [p, p, i, i, i, i, i, c_double, p, z, p]),
        "dc_disp_render_fixed": (i, [p, p, p, p, i, i, i, i, i, p]),
        "dc_lidar_workspace_bytes": (z, [i, i, i]),
        "dc_lidar_depth_maps": (i, [p, z, p, p, i, p, p, p, p, i, i, p, p, z, p]),
        "dc_log_panel_ws_bytes": (z, [i]),
        "dc_log_panel": (i, [p, p, i, p, p, i, i, i, i, p, z, p]),
        "dc_bn_bwd_finalize": (i, [p, i, i, c_double, p, p, p, p, p, p, i, i, p]),
        "dc_bn_bwd_apply": (i, [p, p, p, p, i, i, i, i, p]),
        "dc_conv1x1_bn_ok": (i, [i, i, i, i, i]),
        "dc_conv1x1_stat_parts": (i, [i, i, i, i, i, i, i, POINTER(c_int)]),
        "dc_conv1x1_bwd_parts": (i, [i, i, i, i, i, i, POINTER(c_int)]),
        "dc_conv1x1_fwd_bn": (i, [p, p, p, i, i, i, i, i, i, POINTER(BnFold), p]),
        "dc_conv1x1_dgrad_bn": (i, [p, p, p, p, i, i, i, i, i, i, POINTER(BnFold), p]),
        "dc_conv1x1_wgrad_bn": (i, [p, p, p, p, i, i, i, i, i, i, POINTER(BnFold), p]),
        "dc_wino3x3_bn_ok": (i, [i, i, i, i, i, i]),
        "dc_wino3x3_stat_parts": (i, [i, i, i, i, i, i, POINTER(c_int)]),
        "dc_wino3x3_bwd_parts": (i, [i, i, i, i, i, i, POINTER(c_int)]),
        "dc_wino3x3_fwd_bn": (i, [p, p, p, p, i, i, i, i, i, POINTER(BnFold), p]),
        "dc_wino3x3_dgrad_bn": (i, [p, p, p, p, p, i, i, i, i, i, POINTER(BnFold), p]),
        "dc_wino3x3_wgrad_bn": (i, [p, p, p, p, i, i, i, i, i, POINTER(BnFold), p]),
        "dc_maxpool3x3s2_fwd": (i, [p, p, p, i, i, i, p]),
        "dc_maxpool3x3s2_bwd": (i, [p, p, p, i, i, i, p]),
        "dc_maxpool3x3s2_bwd_add": (i, [p, p, p, p, i, i, i, p]),
        "dc_conv1x1_dgrad_add2": (i, [p, p, p, p, p, i, i, i, i, i, i, p]),
        "dc_conv3x3_bwd_add": (i, [p, i, i, p, i, p, p, p, p, p, p, p, p, p, p, i, i, i, i, i, i, p]),
        "dc_wino3x3_workspace": (z, [i, i, i, i, i]),
        "dc_wino3x3_fwd": (i, [p, p, p, p, i, i, i, i, i, p]),
        "dc_wino3x3_dgrad": (i, [p, p, p, p, i, i, i, i, i, p]),
        "dc_wino3x3_dgrad_add": (i, [p, p, p, p, p, i, i, i, i, i, p]),
        "dc_conv1x1_fwd": (i, [p, p, p, i, i, i, i, i, i, p]),
        "dc_conv1x1_bias_act_fwd": (i, [p, p, p, p, i, i, i, i, i, i, i, p]),
        "dc_bias_act_bwd": (i, [p, p, p, p, i, i, i, i, p]),
        "dc_conv1x1_dgrad": (i, [p, p, p, i, i, i, i, i, i, p]),
        "dc_conv1x1_dgrad_add": (i, [p, p, p, p, i, i, i, i, i, i, p]),
        "dc_conv1x1_wgrad_workspace": (z, [i, i, i, i, i, i]),
        "dc_conv1x1_wgrad": (i, [p, p, p, p, i, i, i, i, i, i, p]),
        "dc_conv_profile_enable": (i, [i, i]),
        "dc_conv_profile_collect": (i, [i, p, p, p, p, p]),
        "dc_wino3x3_wgrad_workspace": (z, [i, i, i, i, i]),
        "dc_wino3x3_wgrad": (i, [p, p, p, p, i, i, i, i, i, p]),
        "dc_stem_supported": (i, [i, i, i, i, i]),
        "dc_stem_fwd": (i, [p, i, f, f, p, p, p, i, i, i, i, p]),
        "dc_stem_wgrad": (i, [p, i, f, f, p, p, p, i, i, i, i, p]),
        "dc_adam_chunk": (i, []),
        "dc_adam_step": (i, [p, p, p, p, i, f, c_double, c_double, f, p]),
        "dc_convs2_supported": (i, [i, i, i, i, i, i]),
        "dc_convs2_fwd_workspace": (z, [i, i, i, i, i, i]),
        "dc_convs2_fwd": (i, [p, p, p, p, i, i, i, i, i, i, p]),
        "dc_convs2_dgrad_workspace": (z, [i, i, i, i, i, i]),
        "dc_convs2_dgrad": (i, [p, p, p, p, i, i, i, i, i, i, p]),
        "dc_convs2_wgrad_workspace": (z, [i, i, i, i, i, i]),
        "dc_convs2_wgrad": (i, [p, p, p, p, i, i, i, i, i, i, p]),
        "dc_convs2_plan_query": (i, [i, i, i, i, i, i, i, POINTER(ConvS2Plan)]),
        "dc_conv2d_direct_fwd": (i, [p, p, p, p, i, i, i, i, i, i, i, i, p]),
        "dc_conv2d_direct_dgrad": (i, [p, p, p, i, i, i, i, i, i, i, i, p]),
        "dc_conv2d_direct_wgrad": (i, [p, p, p, p, i, i, i, i, i, i, i, i, p]),
        "dc_gru_rh_fwd": (i, [p, p, p, i, i, i, p]),
        "dc_gru_rh_bwd": (i, [p, p, p, p, p, i, i, i, p]),
        "dc_gru_blend_fwd": (i, [p, p, p, p, i, i, i, p]),
        "dc_gru_blend_bwd": (i, [p, p, p, p, p, p, p, i, i, i, p]),
        "dc_gru_rh_bwd_acc": (i, [p, p, p, p, p, i, i, i, p]),
        "dc_gru_blend_bwd_acc": (i, [p, p, p, p, p, p, p, i, i, i, p]),
        "dc_gather_copy": (i, [p, p, p, i, p]),
        "dc_gru_residual_fwd": (i, [p, p, p, i, z, p]),
        "dc_gru_residual_bwd": (i, [p, p, i, z, p]),
        "dc_gru_state_bwd": (i, [p, p, i, z, p]),
        "dc_set_wino_plan_streams": (i, [i]),
        "dc_gru_infer_rh": (i, [POINTER(GruInferLevel), i, i, p]),
        "dc_gru_infer_tail": (i, [POINTER(GruInferLevel), i, i, p]),
        "dc_gru_infer_init": (i, [p, p, p, i, i, p]),
        "dc_lstm_block": (i, []),
        "dc_lstm_cell_fwd": (i, [p, p, p, p, i, i, i, p]),
        "dc_lstm_cell_bwd": (i, [p, p, p, p, p, p, i, i, i, p]),
        "dc_lstm_handover_fwd": (i, [p, p, p, p, p, i, i, i, i, p]),
        "dc_lstm_handover_bwd": (i, [p, p, p, p, p, p, i, i, i, i, p]),
        "dc_lstm_infer_step": (i, [p, p, p, p, p, p, p, z, i, i, i, i, p]),
        "dc_gru_handover_fwd": (i, [p, p, p, p, p, p, p, i, i, i, i, p]),
        "dc_gru_handover_bwd": (i, [p, p, p, p, p, p, p, p, p, p, p, i, i, i, i, p]),
        "dc_gru_c2f_infer_step": (i, [p, p, p, p, p, p, p, z, i, i, i, i, p]),
        "dc_set_matrix_precision": (i, [i]),
        "dc_get_matrix_precision": (i, []),
        "dc_clear_error": (i, []),
        "dc_abort_capture": (i, [p]),
        "dc_set_gemm_split": (i, [i]),
        "dc_get_gemm_split": (i, []),
        "dc_gemm1x1x3_fwd_ok": (i, [i, i, i, i, i, i]),
        "dc_gemm1x1x3_dgrad_ok": (i, [i, i, i, i, i, i]),
        "dc_gemm1x1x3_workspace": (c_size_t, [i, i]),
        "dc_gemm1x1x3_fwd": (i, [p, p, p, p, p, i, i, i, i, i, i, i, p]),
        "dc_gemm1x1x3_dgrad": (i, [p, p, p, p, p, p, i, i, i, i, i, i, p]),
        "dc_gemm1x1x3_stat_parts": (i, [i, i, i, i, i, i, i, POINTER(c_int)]),
        "dc_gemm1x1x3_bwd_parts": (i, [i, i, i, i, i, i, POINTER(c_int)]),
        "dc_gemm1x1x3_wgrad_ok": (i, [i, i, i, i, i, i]),
        "dc_gemm1x1x3_wgrad_workspace": (c_size_t, [i, i, i, i, i, i]),
        "dc_gemm1x1x3_wgrad": (i, [p, p, p, p, i, i, i, i, i, i, p]),
        "dc_pointwise_workspace": (c_size_t, [i, POINTER(BnFold), i, i, i, i, i, i]),
        "dc_pointwise_stat_parts": (i, [i, i, i, i, i, i, i, POINTER(c_int)]),
        "dc_pointwise_bwd_parts": (i, [i, i, i, i, i, i, i, POINTER(c_int)]),
        "dc_pointwise_fwd": (i, [p, p, p, p, p, i, i, i, i, i, i, i, POINTER(BnFold), p]),
        "dc_pointwise_dgrad": (i, [p, p, p, p, p, p, i, i, i, i, i, i, POINTER(BnFold), p]),
        "dc_pointwise_wgrad": (i, [p, p, p, p, i, i, i, i, i, i, POINTER(BnFold), p]),
        "dc_set_photo_full": (i, [i]),
        "dc_get_photo_full": (i, []),
        "dc_set_wino_f4": (i, [i]),
        "dc_set_wino_persist": (i, [i]),
        "dc_set_wino_phase": (i, [i]),
        "dc_set_dgrad_split": (i, [i]),
        "dc_wino_cache_new_owner": (i, []),
        "dc_wino_cache_register": (i, [i, p, i, i]),
        "dc_wino_cache_release_owner": (i, [i]),
        "dc_wino_cache_refresh": (i, [i, p]),
        "dc_wino_cache_invalidate": (i, [i]),
        "dc_wino_cache_clear": (i, []),
        "dc_wino_cache_variants": (i, []),
        "dc_resample_ksize": (i, [i, i]),
        "dc_resample_table": (i, [i, i, p, p]),
        "dc_data_resize_axis": (i, [p, p, i, i, i, i, i, p, p, i, p, p]),
        "dc_data_flip": (i, [p, p, i, i, i, p, p]),
        "dc_data_jitter": (i, [p, i, i, p, p, p, p]),
        "dc_data_to_tensor": (i, [p, p, i, i, p]),
        "dc_data_to_rgbx": (i, [p, p, i, i, p]),
        "dc_pack_rgbx": (i, [p, p, i, i, p]),
        "dc_data_jitter_to_tensor": (i, [p, p, p, i, i, p, p, p, p]),
        "dc_data_ragged_resize_axis": (i, [p, z, p, z, p, p, i, i, i, p, p, i, p, p, z, p, z, p]),
        "dc_data_cached_levels": (i, [p, z, p, p, i, i, i, i, p, p, p, p, p, p, p]),
        "dc_data_seq_plan": (i, [i, i, i, i, i, i, POINTER(SeqPlan)]),
        "dc_data_seq_levels": (i, [p, i, i, i, i, i, p, p, p, p, p, p, z, p, z, i, p]),
        "dc_data_seq_batch_plan": (i, [i, i, i, i, i, i, i, POINTER(SeqPlan)]),
        "dc_data_seq_batch_levels": (i, [p, i, i, i, i, i, p, p, p, p, p, p, p, z, p, z, i, p]),
        "dc_attnconv_fwd": (i, [POINTER(AttnMap), POINTER(AttnParams), POINTER(AttnMap), p, i, i, i, i, i, i, p]),
        "dc_attnconv_param_count": (i, [i]),
        "dc_attnconv_bwd_workspace": (z, [i, i, i, i]),
        "dc_attnconv_bwd": (i, [POINTER(AttnMap), POINTER(AttnParams), POINTER(AttnMap), p, POINTER(AttnMap), p, POINTER(AttnMap), p,
                                p, i, i, i, i, i, i, p]),
        "dc_sasa_plan": (i, [i, i, i, i, POINTER(c_int)]),
        "dc_sasa_fwd": (i, [p, p, p, ll, ll, ll, p, p, p, p, i, i, i, i, p]),
        "dc_sasa_bwd_workspace": (z, [i, i, i, i]),
        "dc_sasa_bwd": (i, [p, p, p, ll, ll, ll, p, p, p, p, p, p, p, p, p, p, p, i, i, i, i, p]),
        "dc_profile_enable": (i, [i]),
        "dc_profile_collect": (i, [POINTER(c_double), POINTER(c_int), POINTER(c_double), POINTER(c_int), POINTER(c_double),
                                   POINTER(c_double)]),
    }
    missing = []
    for name, (res, args) in S.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:           # an op whose symbol is absent fails loudly when called
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    return S, missing


EXPORTS = None
MISSING = None


def lib():
    """Load libdepthcore.so (once).  Raises if it has not been built."""
    global _lib, EXPORTS, MISSING
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DepthcoreError(
                "libdepthcore.so not found at %s -- build it with `python __graft_entry__.py` "
                "(or `make -C self-supervised-depth-estimation_amd/csrc`); there is no fallback path" % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        EXPORTS, MISSING = _sig(l)
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        raise DepthcoreError("%s failed: %s" % (what, _ERR.get(rc, rc)))


def ptr(t, dtype=torch.float32):
    """Device pointer of a contiguous CUDA(HIP) tensor, validated; None -> NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise DepthcoreError("depthcore ops need device tensors (got %s); there is no CPU path" % t.device)
    if t.dtype != dtype:
        raise DepthcoreError("expected %s, got %s" % (dtype, t.dtype))
    if not t.is_contiguous():
        raise DepthcoreError("expected a contiguous tensor")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # private accessor: optional, see stream()
_get_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def stream(t=None):
    """hipStream_t of the current PyTorch stream of the CURRENT device.

    `t` is a tensor the launch reads or writes: the kernels are launched on the calling thread's current HIP device,
    so a tensor that lives on another device is refused here (a stream of device 0 with pointers of device 1 is a
    memory fault or silent unordered peer access) -- wrap the call in `torch.cuda.device(t.device)` or call
    `torch.cuda.set_device` first (Trainer.__init__ does).
    The raw accessor is ~30x cheaper than torch.cuda.current_stream() (~9 us, needed once per launch); when a torch
    build lacks it the public API is used."""
    dev = _get_device()
    if t is not None and t.device.index != dev:
        raise DepthcoreError("tensor on %s but the current device is cuda:%d; there is no cross-device launch -- "
                             "use torch.cuda.set_device / torch.cuda.device(...)" % (t.device, dev))
    if _raw_stream is not None:
        return _raw_stream(dev)
    return torch.cuda.current_stream(dev).cuda_stream
