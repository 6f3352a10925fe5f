"""torch.autograd bindings of the C ABI in include/depthcore.h.

Every op enqueues hand-written gfx950 kernels on the current HIP stream; tensors
are allocated by PyTorch's caching allocator and passed down as raw pointers.

A facade: the bindings live in one module per subject (photo, layer_ops, convs, eval_ops, attention, recurrent, above
_autograd and convnode) and this module re-exports their names, so `ops.X` IS the subject module's X and every piece of
mutable state exists once.  The subject modules never import this one.
"""
from ._autograd import (PRECISIONS, GradFork, SkipSum, WgradLanes, _bias_grad_dst, _c, _decision_observers, _fork_addend, _grad_dst,  # noqa: F401
                        _lane_param, _parked_forks, _precision, _record_kink, _slot, _tls, _use_precision,
                        add_decision_observer, assert_no_dangling_sums, matrix_precision, remove_decision_observer, skip_of)
from ._lib import DepthcoreError, PhotoDesc, check, ptr, stream  # noqa: F401
from .attention import (PIXEL_SHUFFLE2, PLAIN, _attn_map, _attn_param_grads, _attn_params, _LocalAttention7, _plane_strided,  # noqa: F401
                        _ResidualAttentionUnit, local_attention7, residual_attention_unit)
from .convnode import _ConvF  # noqa: F401
from .convs import (ACT_ELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, PAD_REFLECT, PAD_ZERO, WinoWeightCache, _BNEval, _BNReLU,  # noqa: F401
                    _Conv1x1, _Conv3x3, _ConvDirect, _MaxPool, _StemConv, _wino_release, bn_eval, bn_relu, conv1x1, conv2d_direct,
                    conv3x3_block, conv_profile_collect, conv_profile_enable, conv_s2, conv_s2_supported, maxpool3x3s2, stem_conv,
                    stem_supported, wino_conv3x3)
from .data import seq_item_rows, seq_rows  # noqa: F401
from .eval_ops import (BENCHMARK_SIZE, STEREO_SCALE_FACTOR, TILE_KINDS, TRAINER_CROP, _MAGMA, _PROTOCOLS, _depth_errors,  # noqa: F401
                       _render_disparity, depth_errors, depth_png16, disparity_range_pooled, eigen_crop, flip_concat,
                       lidar_depth_maps, lidar_depth_maps_staged, log_panels, magma_lut, pose_ate, post_process_disparity,
                       render_disparity, render_disparity_fixed)
from .layer_ops import (_aligned8, _Backproject, _DispToDepth, _GridSample, _PoseHead, _PoseMatrix, _Project3D, _Smooth, _SSIM,  # noqa: F401
                        _UpsampleBilinear, _UpsampleNearest2x, backproject, disp_to_depth, grid_sample_border, pix_coords,
                        pose_head, pose_matrix, project3d, smooth_loss, ssim, upsample_bilinear, upsample_nearest2x)
from .photo import (PhotoConfig, _fill_desc, _PhotoLoss, pack_rgbx, photo_algorithmic_bytes, photometric_loss, profile_collect,  # noqa: F401
                    profile_enable)
from .recurrent import (_GruBlend, _GruHandover, _GruLevel, _GruResidual, _GruRH, _infer_levels, _infer_rows, _LstmCell,  # noqa: F401
                        _LstmHandover, _plan_streams, _rows, copy_segments, gru_blend, gru_infer_init, gru_infer_rh, gru_infer_tail,
                        gru_level_sequence, gru_reset_times_state, gru_sequence_residual, lstm_cell, lstm_handover, lstm_infer_step,
                        gru_handover, gru_c2f_infer_step, stack_frames)
