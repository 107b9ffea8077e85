"""ctypes binding of ``libzsv_hip.so`` (C ABI declared in ``include/zsv_hip.h``).

The shared object is built in-tree by ``csrc/Makefile`` (``__graft_entry__.build()``) with
plain ``hipcc --offload-arch=gfx950``; nothing in its signatures is a torch type -- Python
passes ``tensor.data_ptr()`` and the current HIP stream handle.  There is NO fallback: if
the library is missing, or an op is called on a non-HIP tensor, a ``RuntimeError`` is raised.
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZSV_LIB_PATH") or os.path.join(_HERE, "libzsv_hip.so")   # (override: A/B of two builds)


class ConvDesc(Structure):
    """Mirror of ``zsv_conv_desc`` (include/zsv_hip.h)."""
    _fields_ = [(n, c_int32) for n in (
        "N", "Cin", "Ti", "Hi", "Wi", "Cout", "To", "Ho", "Wo",
        "kT", "kH", "kW", "sT", "sH", "sW", "pT", "pH", "pW")]


_P = c_void_p
# name -> (restype, argtypes); must list every symbol include/zsv_hip.h declares
SIGNATURES = {
    "zsv_status_string": (c_char_p, [c_int]),
    "zsv_version": (c_char_p, []),
    "zsv_reload_knobs": (c_int32, []),
    "zsv_conv3d_fwd_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "zsv_conv3d_fwd": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "zsv_conv3d_fwd_stat_tiles": (c_int32, [POINTER(ConvDesc), _P]),
    "zsv_conv3d_fwd_stats": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, c_int, _P, c_int32, _P, c_size_t, _P]),
    "zsv_conv3d_fwd_add_supported": (c_int32, [POINTER(ConvDesc)]),
    "zsv_conv3d_fwd_add": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "zsv_conv3d_fwd_full": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, c_int, _P, c_int32, _P, c_size_t, _P]),
    "zsv_conv3d_dgrad_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "zsv_conv3d_dgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, c_size_t, _P]),
    "zsv_conv3d_dgrad_add_supported": (c_int32, [POINTER(ConvDesc)]),
    "zsv_conv3d_dgrad_add": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, c_size_t, _P]),
    "zsv_conv3d_dgrad_add_strided_supported": (c_int32, [POINTER(ConvDesc), c_int32, c_int32, c_int32]),
    "zsv_conv3d_dgrad_add_strided": (c_int, [POINTER(ConvDesc), _P, _P, _P, c_int32, c_int32, c_int32, _P, _P, c_size_t, _P]),
    "zsv_conv3d_wgrad_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "zsv_conv3d_wgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, c_size_t, _P]),
    "zsv_conv3d_wgrad_mask_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "zsv_conv3d_wgrad_mask": (c_int, [POINTER(ConvDesc), _P, _P]),
    "zsv_conv3d_wgrad_masked": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, c_size_t, _P, _P]),
    # depthwise (groups == channels): the same descriptor with Cin == Cout
    "zsv_dwconv3d_supported": (c_int32, [POINTER(ConvDesc)]),
    "zsv_dwconv3d_fwd": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, c_int, _P]),
    "zsv_dwconv3d_dgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P]),
    "zsv_dwconv3d_wgrad_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "zsv_dwconv3d_wgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, c_size_t, _P]),
    "zsv_bn_fwd_train_coeffs": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, c_float, c_float, _P, c_int32, _P,
                                        c_int32, _P, c_size_t, _P]),
    "zsv_conv3d_pre_supported": (c_int32, [POINTER(ConvDesc)]),
    "zsv_conv3d_fwd_pre": (c_int, [POINTER(ConvDesc), _P, _P, c_int32, _P, _P, _P, c_int32, _P, c_size_t, _P]),
    "zsv_conv3d_wgrad_pre": (c_int, [POINTER(ConvDesc), _P, _P, c_int32, _P, _P, _P, c_size_t, _P]),
    "zsv_channel_sum_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "zsv_channel_sum": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P, c_size_t, _P]),
    "zsv_bn_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "zsv_bn_fwd_train": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P, _P, c_int, _P, _P, _P, _P, _P,
                                 c_float, c_float, _P, c_size_t, _P]),
    "zsv_bn_fwd_train_stats": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P, _P, c_int, _P, _P, _P, _P, _P,
                                       c_float, c_float, _P, c_int32, _P, c_size_t, _P]),
    "zsv_bn_fwd_eval": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, c_int, c_float, _P, _P,
                                c_size_t, _P]),
    "zsv_bn_bwd": (c_int, [_P, _P, _P, c_int32, c_int32, c_int32, _P, _P, _P, _P, c_int, _P, _P, _P, _P, _P,
                           c_size_t, _P]),
    "zsv_bn_bwd_eval": (c_int, [_P, _P, _P, c_int32, c_int32, c_int32, _P, _P, _P, _P, c_float, c_int, _P, _P, _P, _P, _P,
                                c_size_t, _P]),
    "zsv_bn_eval_coeffs": (c_int, [c_int32, _P, _P, _P, _P, c_float, _P, c_int32, _P]),
    # BatchNorm statistics over all ranks (a collective runs between moments and finalize, and between bwd_reduce and bwd_apply):
    # x, N, C, S, moments, workspace, bytes, stream / gathered, world, C, gamma, beta, running_mean, running_var, momentum, eps,
    # save_mean, save_invstd, total_count_out, stream / x, N, C, S, save_mean, save_invstd, gamma, beta, residual, fuse_relu, y,
    # stream / dy, x, y, N, C, S, save_mean, save_invstd, gamma, beta, fuse_relu, sums, workspace, bytes, stream / dy, x, y, N, C,
    # S, save_mean, save_invstd, gamma, beta, fuse_relu, sums_local, sums_global, total_count, dx, d_residual, dgamma, dbeta, stream
    "zsv_bn_sync_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "zsv_bn_sync_moments": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P, c_size_t, _P]),
    "zsv_bn_sync_finalize": (c_int, [_P, c_int32, c_int32, _P, _P, _P, _P, c_float, c_float, _P, _P, _P, _P]),
    "zsv_bn_sync_apply": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, c_int, _P, _P]),
    "zsv_bn_sync_bwd_reduce": (c_int, [_P, _P, _P, c_int32, c_int32, c_int32, _P, _P, _P, _P, c_int, _P, _P, c_size_t, _P]),
    "zsv_bn_sync_bwd_apply": (c_int, [_P, _P, _P, c_int32, c_int32, c_int32, _P, _P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "zsv_relu_fwd": (c_int, [_P, _P, c_int64, _P]),
    "zsv_relu_bwd": (c_int, [_P, _P, _P, c_int64, _P]),
    "zsv_relu_bwd_bias": (c_int, [_P, _P, _P, c_int32, c_int32, c_int32, _P, _P, c_size_t, _P]),
    "zsv_add_relu_fwd": (c_int, [_P, _P, _P, c_int64, _P]),
    "zsv_meanpool_fwd": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P]),
    "zsv_meanpool_bwd": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P]),
    "zsv_maxpool3d_fwd": (c_int, [_P] + [c_int32] * 14 + [_P, _P, _P]),
    "zsv_maxpool3d_bwd": (c_int, [_P, _P] + [c_int32] * 14 + [_P, _P]),
    "zsv_linear_fwd_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "zsv_linear_fwd": (c_int, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int, _P, c_size_t, _P]),
    "zsv_linear_dgrad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "zsv_linear_dgrad": (c_int, [_P, _P, _P, c_int32, c_int32, c_int32, _P, c_size_t, _P]),
    "zsv_linear_wgrad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "zsv_linear_wgrad": (c_int, [_P, _P, _P, c_int32, c_int32, c_int32, _P, c_size_t, _P]),
    "zsv_bf16_channel_pitch": (c_int32, [c_int32]),
    "zsv_conv3d_bf16_blob_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "zsv_conv3d_bf16_pack": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "zsv_conv3d_bf16_pack_dgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P]),
    "zsv_conv3d_bf16_dgrad_blob_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "zsv_conv3d_bf16_dgrad_pack": (c_int, [POINTER(ConvDesc), _P, _P, _P]),
    "zsv_conv3d_bf16_dgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "zsv_conv3d_bf16_fwd": (c_int, [POINTER(ConvDesc), _P, _P, _P, c_int, _P, _P]),
    "zsv_clip_to_bf16": (c_int, [_P] + [c_int32] * 9 + [_P, _P]),
    "zsv_maxpool3d_bf16": (c_int, [_P] + [c_int32] * 14 + [_P, _P]),
    "zsv_meanpool_bf16": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P]),
    "zsv_fp8_channel_pitch": (c_int32, [c_int32]),
    "zsv_conv3d_fp8_blob_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "zsv_conv3d_fp8_pack": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "zsv_conv3d_fp8_fwd": (c_int, [POINTER(ConvDesc), _P, _P, _P, c_int, _P, _P]),
    "zsv_meanpool_fp8": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P]),
    "zsv_maxpool3d_fp8": (c_int, [_P] + [c_int32] * 14 + [_P, _P]),
    "zsv_absmax_bf16": (c_int, [_P, c_int64, _P, _P]),
    "zsv_bn_cl_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "zsv_bn_cl_fwd_train": (c_int, [_P, _P, c_int64, c_int32, _P, _P, _P, _P, c_float, c_float, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    "zsv_bn_cl_fwd_train_stats": (c_int, [_P, _P, c_int64, c_int32, _P, _P, _P, _P, c_float, c_float, c_int, _P, _P, _P, _P, _P, c_int32, _P,
                                          c_size_t, _P]),
    "zsv_conv3d_bf16_stat_rows": (c_int32, [POINTER(ConvDesc)]),
    "zsv_conv3d_bf16_fwd_stats": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, c_int32, _P, _P]),
    "zsv_bn_cl_bwd": (c_int, [_P, _P, _P, c_int64, c_int32, _P, _P, _P, _P, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    "zsv_bn_cl_fwd_eval": (c_int, [_P, _P, c_int64, c_int32, _P, _P, _P, _P, c_float, c_int, _P, _P, _P]),
    "zsv_bn_cl_bwd_eval": (c_int, [_P, _P, _P, c_int64, c_int32, _P, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    "zsv_conv3d_bf16_wgrad_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "zsv_conv3d_bf16_wgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, c_size_t, _P]),
    "zsv_maxpool3d_bf16_bwd": (c_int, [_P, _P] + [c_int32] * 14 + [_P, _P]),
    "zsv_relu_bias_bwd_cl": (c_int, [_P, _P, c_int64, c_int32, _P, _P, _P, c_size_t, _P]),
    "zsv_cl_bf16_to_ncs_f32": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P]),
    "zsv_ncs_f32_to_cl_bf16": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P]),
    "zsv_meanpool_bf16_bwd": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P]),
    "zsv_clip_transform": (c_int, [_P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, _P, _P, _P]),
    "zsv_clip_transform_batch": (c_int, [_P, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "zsv_still_image_clips": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "zsv_resample_coeffs": (c_int, [c_int32, c_int32, _P, _P, _P]),
    "zsv_cosine_topk_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "zsv_cosine_topk": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, c_size_t, _P]),
    # pred, true, labels, class table, rows, dim, classes, position tables, tables, counts, class_counts, workspace, bytes, stream
    "zsv_split_accuracy_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "zsv_split_accuracy": (c_int, [_P, _P, _P, _P, c_int32, c_int32, c_int32, _P, c_int32, _P, _P, _P, c_size_t, _P]),
    # softmax cross-entropy (csrc/softmax_xent.hip): logits, labels, N, C, label_smoothing, ignore_index, row_loss, row_rank, dlogits,
    # stream / row_loss, row_rank, N, mean, loss, counts, stream / dlogits, grad_loss, counts, mean, N, C, dx, stream
    "zsv_softmax_xent_fwd": (c_int, [_P, _P, c_int32, c_int32, c_double, c_int64, _P, _P, _P, _P]),
    "zsv_softmax_xent_reduce": (c_int, [_P, _P, c_int32, c_int32, _P, _P, _P]),
    "zsv_softmax_xent_bwd": (c_int, [_P, _P, _P, c_int32, c_int32, c_int32, _P, _P]),
    "zsv_adam_multi": (c_int, [_P, c_int32, c_int64, c_float, c_float, c_float, c_float, c_int32, _P]),
    "zsv_grad_check_multi": (c_int, [_P, c_int32, c_int64, _P, _P]),
    "zsv_adam_multi_scaled": (c_int, [_P, c_int32, c_int64, c_float, c_float, c_float, c_float, _P, _P]),
    "zsv_scaler_update": (c_int, [_P, c_float, c_float, c_int32, _P]),
    "zsv_grad_norm_workspace_bytes": (c_size_t, [c_int64]),
    "zsv_grad_norm_multi": (c_int, [_P, c_int32, c_int64, c_int64, _P, c_size_t, _P, _P]),
    "zsv_grad_norm_finalize": (c_int, [_P, c_int64, c_float, _P, _P, _P]),
    "zsv_grad_unscale_multi": (c_int, [_P, c_int32, c_int64, _P, _P]),
    "zsv_adamw_multi": (c_int, [_P, c_int32, c_int64, c_double, c_float, c_float, c_float, c_double, c_int32, _P, c_int32, _P]),
    "zsv_adamw_multi_scaled": (c_int, [_P, c_int32, c_int64, c_double, c_float, c_float, c_float, c_double, c_int32, _P, _P,
                                       c_int32, _P]),
    "zsv_grad_accum_multi": (c_int, [_P, c_int32, c_int64, c_float, c_int32, _P]),
    # table, count, chunks, lr, momentum, dampening, nesterov, weight_decay, maximize, clip, scaler state, grads_unscaled, first_step,
    # shadows, avg state, ema_weight, stream
    "zsv_sgd_multi": (c_int, [_P, c_int32, c_int64, c_double, c_float, c_float, c_int32, c_double, c_int32, _P, _P, c_int32, c_int32,
                              _P, _P, c_float, _P]),
    # LARS / LAMB (csrc/layerwise.hip).  The three workspace launches: table, count, chunks, chunk_offset, tensor_offset, all_count,
    # workspace, bytes, then their own arguments; the two apply launches: table, count, chunks, records, then zsv_sgd_multi's
    # arguments from lr on / lr, betas, eps, weight_decay, scaler state, step, shadows, avg state, ema_weight
    "zsv_layerwise_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "zsv_lars_norms": (c_int, [_P, c_int32, c_int64, c_int64, c_int32, c_int32, _P, c_size_t, _P, _P]),
    "zsv_lamb_moments": (c_int, [_P, c_int32, c_int64, c_int64, c_int32, c_int32, _P, c_size_t, c_float, c_float, c_float, c_double,
                                 _P, _P, c_int32, c_int32, _P]),
    "zsv_layerwise_finalize": (c_int, [_P, c_int32, c_int64, c_int64, c_int32, c_int32, _P, c_size_t, c_int32, c_int32, c_double,
                                       c_double, c_double, c_double, _P, _P, c_int32, _P]),
    "zsv_lars_multi": (c_int, [_P, c_int32, c_int64, _P, c_double, c_float, c_float, c_int32, c_double, c_int32, _P, _P, c_int32,
                               c_int32, _P, _P, c_float, _P]),
    "zsv_lamb_multi": (c_int, [_P, c_int32, c_int64, _P, c_double, c_float, c_float, c_float, c_double, _P, c_int32, _P, _P, c_float,
                               _P]),
    # the four Adam launches with weight averaging: their own arguments up to the stream, then shadows, avg state, ema_weight
    "zsv_adam_multi_avg": (c_int, [_P, c_int32, c_int64, c_float, c_float, c_float, c_float, c_int32, _P, _P, c_float, _P]),
    "zsv_adam_multi_scaled_avg": (c_int, [_P, c_int32, c_int64, c_float, c_float, c_float, c_float, _P, _P, _P, c_float, _P]),
    "zsv_adamw_multi_avg": (c_int, [_P, c_int32, c_int64, c_double, c_float, c_float, c_float, c_double, c_int32, _P, c_int32,
                                    _P, _P, c_float, _P]),
    "zsv_adamw_multi_scaled_avg": (c_int, [_P, c_int32, c_int64, c_double, c_float, c_float, c_float, c_double, c_int32, _P, _P,
                                           c_int32, _P, _P, c_float, _P]),
    "zsv_avg_multi": (c_int, [_P, c_int32, c_int64, _P, c_float, _P, _P]),
    "zsv_avg_advance": (c_int, [_P, _P, _P]),
    "zsv_swap_multi": (c_int, [_P, c_int32, c_int64, _P]),
    "zsv_adam_step": (c_int, [_P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_int32, _P]),
    "zsv_conv3d_panel_query": (c_int, [POINTER(ConvDesc), c_int32, c_int32, POINTER(c_size_t)]),
    "zsv_conv3d_panel_job": (c_int, [POINTER(ConvDesc), c_int32, c_int32, _P, _P, c_size_t, _P]),
    "zsv_pack_multi": (c_int, [_P, c_int32, c_int64, _P]),
    "zsv_conv3d_fwd_full_panel": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, c_int, _P, c_int32, _P, c_size_t, _P, _P, c_size_t]),
    "zsv_conv3d_fwd_pre_panel": (c_int, [POINTER(ConvDesc), _P, _P, c_int32, _P, _P, _P, c_int32, _P, c_size_t, _P, _P, c_size_t]),
    "zsv_conv3d_dgrad_add_panel": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, c_size_t, _P, _P, c_size_t]),
    "zsv_conv3d_dgrad_add_strided_panel": (c_int, [POINTER(ConvDesc), _P, _P, _P, c_int32, c_int32, c_int32, _P, _P, c_size_t, _P, _P,
                                                   c_size_t]),
}


class PackJob(Structure):
    """Mirror of ``zsv_pack_job`` (include/zsv_hip.h): one weight-panel pack launch written down for ``zsv_pack_multi``."""
    _fields_ = [("kind", c_int32), ("reserved", c_int32), ("total", c_int64), ("first_block", c_int64), ("w", c_void_p),
                ("out", c_void_p), ("l", c_int64 * 2), ("i", c_int32 * 20)]

_lock = threading.Lock()
_lib = None


# The library snapshots its ZSV_* switches at load (csrc/knobs.h): the launch path reads an array, never getenv().  A process that
# flips a switch afterwards (tests, A/B tools) calls ``reload_knobs()``.  (Round 3 watched os.environ with a process-wide audit
# hook instead -- a Python callback on every audited event of the interpreter, on the launch path of every op, that can never be
# removed; ADVICE r3.  It is now installed only on request, ZSV_WATCH_ENV=1, for interactive sessions.)
_knobs_dirty = False
_knob_generation = 0          # bumped whenever the library re-read changed switches (cached weight panels depend on them)
_knob_snapshot = None


def knob_generation() -> int:
    return _knob_generation


def _zsv_environment():
    return tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("ZSV_")))


def reload_knobs() -> bool:
    """Make the library re-read its ZSV_* switches if any of them changed since the last snapshot.  Call it after writing a
    ``ZSV_*`` variable in a live process and before the next launch; not meant to race with launches on other threads.
    Returns True when something had changed."""
    global _knob_generation, _knob_snapshot, _knobs_dirty
    # (the flag goes down before load(): load() calls back here while it is up, and would never return.  A write that lands
    # after this line raises it again and is picked up by the next load(); the snapshot below is taken after it either way.)
    _knobs_dirty = False
    lib = load()
    with _lock:
        now = _zsv_environment()
        if now == _knob_snapshot:
            return False
        _knob_snapshot = now
        _knob_generation += 1
        lib.zsv_reload_knobs()
        return True


def _watch_environment(event, args):
    global _knobs_dirty
    if event in ("os.putenv", "os.unsetenv") and args and bytes(args[0]).startswith(b"ZSV_"):
        _knobs_dirty = True


def load() -> ctypes.CDLL:
    """Load (once) and type the library; raises ``RuntimeError`` when it has not been built."""
    global _lib, _knob_snapshot
    if _lib is not None:
        if _knobs_dirty:                      # (only ever set under ZSV_WATCH_ENV=1)
            reload_knobs()
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.isfile(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_PATH} is missing: build the HIP extension first "
                    "(python -c 'import __graft_entry__ as g; g.build()' or make -C "
                    "zeroshotvideoclassification_amd/csrc). There is no CPU fallback.")
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)      # AttributeError if the symbol is not exported
                fn.restype = res
                fn.argtypes = args
            if os.environ.get("ZSV_WATCH_ENV"):
                import sys
                sys.addaudithook(_watch_environment)
            _knob_snapshot = _zsv_environment()
            _lib = lib
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().zsv_status_string(int(status)).decode()
        raise RuntimeError(f"{what} failed: {msg} (zsv status {status})")


# ---- writes the autograd version counters cannot see ---------------------------------------------
# Kernels write through raw ``data_ptr()``s (BatchNorm running statistics, FusedAdam's parameter update),
# and ``.data`` writes (``dist.broadcast(t.data)``, ``p.data = ...``) skip ``tensor._version`` as well.
# Anything that caches values derived from parameters / buffers (``inference.engine_for``) keys on this
# counter too; every such writer calls ``note_raw_write()``.
_raw_write_generation = 0
_raw_param_generation = 0       # ... of which: writes that touched PARAMETERS (cached weight panels key on this one only)


def note_raw_write(parameters: bool = True) -> None:
    """``parameters=False``: only buffers were written (BatchNorm running statistics, every training forward)."""
    global _raw_write_generation, _raw_param_generation
    _raw_write_generation += 1
    if parameters:
        _raw_param_generation += 1


def raw_write_generation() -> int:
    return _raw_write_generation


def raw_param_generation() -> int:
    return _raw_param_generation
