"""Loader for libmumpy_hip.so.  Fails loudly: there is no fallback implementation."""
import ctypes
import os
import subprocess
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
_LIB = None

c_f = ctypes.c_void_p      # device pointers travel as void*
c_i = ctypes.c_int
c_l = ctypes.c_int64
c_fl = ctypes.c_float
c_d = ctypes.c_double


class Surface(NamedTuple):
    """One public header of include/ and its binding.  `version_fn` is the export that answers the header's version define."""
    header: str
    version_fn: str
    version: int
    signatures: dict        # name -> argtypes; the return type is int64_t for a *_bytes query and int for everything else


# One record per header, oldest first: a surface is frozen once the next one exists.  Each table mirrors its header one to one
# (tests/test_abi.py holds every record to its header and to both libraries' exports).
SURFACES = [
    Surface("mumpy_hip.h", "mumpy_abi_version", 2, {
        "mumpy_layernorm_fwd": [c_f, c_f, c_f, c_f, c_l, c_i, c_fl, c_f],
        "mumpy_layernorm_bf16_fwd": [c_f, c_f, c_f, c_f, c_l, c_i, c_fl, c_f],
        "mumpy_linear_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f],
        "mumpy_linear_bf16s_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_f],
        "mumpy_window_attention_bf16_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_window_attention_bf16mm_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_linear_ws_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f, c_l, c_f],
        "mumpy_linear_wsz_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f, c_l, c_f],
        "mumpy_linear_rd_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f],
        "mumpy_window_attention_bg_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_linear_workspace_bytes": [c_l, c_i, c_i],
        "mumpy_tuning_build": [],
        "mumpy_workspace_status": [c_f, ctypes.POINTER(ctypes.c_int)],
        "mumpy_linear_ln_tiles": [c_l, c_i, c_i],
        "mumpy_linear_lnx_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f, c_l, c_f, c_f, c_i, c_f, c_fl, c_f],
        "mumpy_linear_rows_fwd": [c_f, c_l, c_l, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f, c_l, c_f],
        "mumpy_linear_rows_kseg_fwd": [c_f, c_l, c_l, c_i, c_i, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f, c_l, c_f],
        "mumpy_gn_stats_nhwc_fwd": [c_f, c_f, c_i, c_l, c_i, c_i, c_i, c_f],
        "mumpy_gn_apply_resample_nhwc_fwd": [c_f, c_f, c_i, c_f, c_f, c_i, c_fl, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_i, c_i,
                                             c_i, c_i, c_i, c_i, c_f],
        "mumpy_conv2d_nhwc_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_l, c_f],
        "mumpy_conv2d_workspace_bytes": [c_i, c_i, c_i, c_i, c_i, c_i, c_i],
        "mumpy_avgpool2_pad_nhwc_fwd": [c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_copy_rows_fwd": [c_f, c_l, c_f, c_l, c_l, c_i, c_f],
        "mumpy_merge_views_fwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_trunk_head_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f],
        "mumpy_final_conv_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_window_attention_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_deform_offsets_fwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f],
        "mumpy_deform_sample_fwd": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_deform_attention_fwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_deform_sample_kv_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_deform_out_combine_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f],
        "mumpy_deform_attention_mm16_fwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_window_attention_plan": [c_i, c_i, c_i, c_i],
        "mumpy_window_attention_bf16_plan": [c_i, c_i, c_i, c_i],
        "mumpy_deform_attention_plan": [c_i, c_i, c_i, c_i, c_i],
        "mumpy_deform_sample_kv_mm16_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_deform_out_combine_mm16_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f],
        "mumpy_deform_combine_fwd": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f],
        "mumpy_faf_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_patch_embed_fwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_patch_merge_ln_fwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_temporal_attention_fwd": [c_f, c_f, c_l, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_attention_probs_fwd": [c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_l, c_l, c_l, c_l, c_l, c_fl, c_f],
        "mumpy_temporal_attention_q_fwd": [c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_sigmoid_threshold_fwd": [c_f, c_f, c_l, c_fl, c_f],
        "mumpy_add_fwd": [c_f, c_f, c_f, c_l, c_f],
        "mumpy_normalize_u8_fwd": [c_f, c_f, c_l, c_i, c_i, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), c_f],
        "mumpy_resize_nearest_table": [c_i, c_i, ctypes.POINTER(ctypes.c_int32)],
        "mumpy_resize_normalize_u8_fwd": [c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_i, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), c_f],
        "mumpy_mask_loss_workspace_bytes": [c_i, c_l],
        "mumpy_mask_loss_fwd_bwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_l, c_fl, c_fl, c_f],
        "mumpy_layernorm_bwd_workspace_bytes": [c_l, c_i],
        "mumpy_layernorm_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_l, c_i, c_fl, c_i, c_f],
        "mumpy_gelu_fwd": [c_f, c_f, c_l, c_f],
        "mumpy_gelu_bwd": [c_f, c_f, c_f, c_l, c_f],
        "mumpy_transpose_fwd": [c_f, c_f, c_l, c_l, c_f],
        "mumpy_col_sum_workspace_bytes": [c_l, c_i],
        "mumpy_col_sum_fwd": [c_f, c_f, c_f, c_l, c_l, c_i, c_f],
        "mumpy_final_conv_bwd_workspace_bytes": [c_i, c_i, c_i],
        "mumpy_final_conv_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_f],
        "mumpy_patch_gather_fwd": [c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_f],
        "mumpy_conv_weight_dgrad_fwd": [c_f, c_f, c_i, c_i, c_i, c_i, c_f],
        "mumpy_conv2d_wgrad_workspace_bytes": [c_i, c_i, c_i, c_i, c_i, c_i, c_i],
        "mumpy_conv2d_wgrad_nhwc": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_l, c_f],
        "mumpy_linear_bwd_workspace_bytes": [c_l, c_i, c_i],
        "mumpy_linear_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f, c_l, c_f],
        "mumpy_window_attention_bwd_workspace_bytes": [c_i, c_i, c_i, c_i],
        "mumpy_window_attention_bwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_i, c_fl, c_i, c_f],
        "mumpy_window_attention_bwd_csr": [c_f, c_f, c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_i, c_fl, c_i, c_f],
        "mumpy_window_attention_mm16_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_window_attention_mm16_bwd_workspace_bytes": [c_i, c_i, c_i, c_i],
        "mumpy_window_attention_mm16_bwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_i, c_fl, c_i, c_f],
        "mumpy_relpos_bias_expand_fwd": [c_f, c_f, c_f, c_i, c_f],
        "mumpy_gn_bwd_workspace_bytes": [c_i, c_l, c_i],
        "mumpy_gn_bwd_nhwc": [c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_l, c_i, c_i, c_fl, c_i, c_f],
        "mumpy_upsample_bwd_nhwc": [c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_temporal_attention_bwd": [c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_fl, c_f],
        "mumpy_scale_samples_fwd": [c_f, c_f, c_f, c_i, c_l, c_f],
        "mumpy_dwconv5_window_fwd": [c_f, c_f, c_f, c_f, c_l, c_i, c_f],
        "mumpy_dwconv5_window_bwd_workspace_bytes": [c_l, c_i],
        "mumpy_dwconv5_window_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_l, c_i, c_f],
        "mumpy_deform_attention_bwd_workspace_bytes": [c_l, c_i],
        "mumpy_deform_attention_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_l, c_i, c_i, c_fl, c_f],
        "mumpy_deform_sample_bwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_f],
        "mumpy_adamw_hyper": [ctypes.POINTER(ctypes.c_float), c_d, c_d, c_d, c_d, c_d, c_i, c_d],
        "mumpy_adamw_step_dev": [c_f, c_f, c_f, c_f, c_l, c_f, c_f],
        "mumpy_adamw_step": [c_f, c_f, c_f, c_f, c_l, c_d, c_d, c_d, c_d, c_d, c_i, c_d, c_f],
        "mumpy_sgd_step": [c_f, c_f, c_f, c_l, c_d, c_d, c_d, c_d, c_i, c_d, c_f],
        "mumpy_sgd_hyper": [ctypes.POINTER(ctypes.c_float), c_d, c_d, c_d, c_d, c_i, c_d],
        "mumpy_sgd_step_dev": [c_f, c_f, c_f, c_l, c_f, c_i, c_f],
        "mumpy_rmsprop_step": [c_f, c_f, c_f, c_f, c_l, c_d, c_d, c_d, c_d, c_d, c_d, c_f],
        "mumpy_rmsprop_hyper": [ctypes.POINTER(ctypes.c_float), c_d, c_d, c_d, c_d, c_d, c_d],
        "mumpy_rmsprop_step_dev": [c_f, c_f, c_f, c_f, c_l, c_f, c_f],
        "mumpy_grad_norm_partials": [c_l],
        "mumpy_grad_norm_partial": [c_f, c_l, c_f, c_f],
        "mumpy_grad_norm_finish": [c_f, c_f, c_f, c_f, c_i, c_i, c_d, c_f, c_f],      # (the first four: HOST tables, one entry per group)
    }),
    Surface("mumpy_hip_ext.h", "mumpy_ext_version", 1, {
        "mumpy_adamw_gate_hyper": [ctypes.POINTER(ctypes.c_double), c_d, c_d, c_d, c_i],
        "mumpy_update_gate": [c_f, c_i, c_f, c_f, c_f, c_i, c_f, c_f, c_f],       # (stats, hyper_dev, optimizer_kind: HOST tables)
        "mumpy_adamw_step_gated_dev": [c_f, c_f, c_f, c_f, c_l, c_f, c_f, c_f],
        "mumpy_sgd_step_gated_dev": [c_f, c_f, c_f, c_l, c_f, c_i, c_f, c_f],
        "mumpy_rmsprop_step_gated_dev": [c_f, c_f, c_f, c_f, c_l, c_f, c_f, c_f],
    }),
    Surface("mumpy_hip_ext2.h", "mumpy_ext2_version", 2, {
        "mumpy_deform_attention_mm16_bwd_workspace_bytes": [c_l, c_i, c_i],
        "mumpy_deform_attention_mm16_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_l, c_i, c_i, c_fl, c_f],
        "mumpy_linear_gelu_dual_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f, c_l, c_f],
        "mumpy_linear_gelu_bwd_workspace_bytes": [c_l, c_i, c_i],
        "mumpy_linear_gelu_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f, c_l, c_f],
    }),
    # mean3 / std3: HOST arrays
    Surface("mumpy_hip_ext3.h", "mumpy_ext3_version", 1, {
        "mumpy_augment_stage_u8_fwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_l, c_i, c_i, c_i, ctypes.POINTER(ctypes.c_float),
                                       ctypes.POINTER(ctypes.c_float), c_f],
    }),
    # mean3 / std3: HOST arrays
    Surface("mumpy_hip_ext4.h", "mumpy_ext4_version", 1, {
        "mumpy_augment_warp_u8_fwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_l, c_i, c_i, c_i,
                                      ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), c_f],
    }),
    # mean3 / std3: HOST arrays
    Surface("mumpy_hip_ext5.h", "mumpy_ext5_version", 1, {
        "mumpy_clip_window_u8_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_l, c_i, c_i, c_i, c_i, ctypes.POINTER(ctypes.c_float),
                                     ctypes.POINTER(ctypes.c_float), c_f],
        "mumpy_mask_score_u8_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_l, c_l, c_f],
        "mumpy_frame_metrics_fwd": [c_f, c_l, c_l, c_f, c_i, c_f],
    }),
    Surface("mumpy_hip_ext6.h", "mumpy_ext6_version", 1, {
        "mumpy_resize_bilinear_u8_fwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
    }),
    Surface("mumpy_hip_ext7.h", "mumpy_ext7_version", 1, {
        "mumpy_score_exceed_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_l, c_l, c_i, c_f],
        "mumpy_sweep_metrics_fwd": [c_f, c_l, c_l, c_i, c_f, c_f, c_i, c_f],
    }),
    # the frozen siblings' arguments plus `int groups` before the stream
    Surface("mumpy_hip_ext8.h", "mumpy_ext8_version", 1, {
        "mumpy_deform_sample_grouped_fwd": [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_deform_sample_kv_grouped_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_deform_sample_kv_mm16_grouped_fwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_deform_attention_grouped_fwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_fl, c_i, c_f],
        "mumpy_deform_attention_mm16_grouped_fwd": [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_fl, c_i, c_f],
    }),
    # the frozen backward siblings' arguments plus `int groups` before the stream
    Surface("mumpy_hip_ext9.h", "mumpy_ext9_version", 1, {
        "mumpy_deform_sample_grouped_bwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f],
        "mumpy_deform_attention_grouped_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_l, c_i, c_i, c_fl, c_i, c_f],
        "mumpy_deform_attention_mm16_grouped_bwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_l, c_i, c_i, c_fl, c_i, c_f],
    }),
    # eps3 / lo3 / hi3: HOST arrays
    Surface("mumpy_hip_ext10.h", "mumpy_ext10_version", 1, {
        "mumpy_faf_bwd": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f],
        "mumpy_tokenize_dx": [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f],
        "mumpy_pgd_step": [c_f, c_f, c_f, c_l, c_l, c_fl, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                           ctypes.POINTER(ctypes.c_float), c_f],
    }),
]
ABI_VERSION = SURFACES[0].version
SIGNATURES = {name: args for s in SURFACES for name, args in s.signatures.items()}      # every bound entry, whichever header declares it

# include/mumpy_perturb.h: the ordinary perturbations of uint8 frames.  A surface outside the mumpy_hip.h / mumpy_hip_ext*.h family that
# SURFACES lists (tests/test_abi.py pins that family's headers, versions and names with literals, and tests/test_input_grad_host.py
# the names of the newest of them), bound and version-checked by load_library in the same way; tests/test_perturb_host.py holds it to
# its header and to both libraries' exports.
PERTURB = Surface("mumpy_perturb.h", "mumpy_perturb_version", 1, {
    "mumpy_jpeg_roundtrip_workspace_bytes": [c_l, c_i, c_i],
    "mumpy_jpeg_roundtrip_u8_fwd": [c_f, c_f, c_f, c_f, c_f, c_l, c_l, c_i, c_i, c_i, c_f],
    "mumpy_gaussian_blur_workspace_bytes": [c_l, c_i, c_i],
    "mumpy_gaussian_blur_u8_fwd": [c_f, c_f, c_f, c_f, c_l, c_l, c_i, c_i, c_f],
    "mumpy_resize_nearest_u8_fwd": [c_f, c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_i, c_f],
})

# include/mumpy_photometric.h: the photometric operations of uint8 frames, a surface of its own for the same reason
# (tests/test_perturb_host.py pins the names of mumpy_perturb.h); tests/test_photometric_host.py holds it to its header and exports.
PHOTOMETRIC = Surface("mumpy_photometric.h", "mumpy_photometric_version", 1, {
    "mumpy_photometric_workspace_bytes": [c_l, c_i, c_i],
    "mumpy_photometric_u8_fwd": [c_f, c_f, c_f, c_f, c_l, c_l, c_i, c_i, c_f],
})

# include/mumpy_geometric.h: the affine operations and Cutout on uint8 frames and masks, a surface of its own for the same reason;
# tests/test_geometric_host.py holds it to its header and exports.
GEOMETRIC = Surface("mumpy_geometric.h", "mumpy_geometric_version", 1, {
    "mumpy_geometric_u8_fwd": [c_f, c_f, c_f, c_l, c_i, c_i, c_i, c_f],
})

# include/mumpy_postprocess.h: cleaning predicted masks (small components out, small holes filled), a surface of its own for the same
# reason; tests/test_postprocess_host.py holds it to its header and exports.
POSTPROCESS = Surface("mumpy_postprocess.h", "mumpy_postprocess_version", 1, {
    "mumpy_mask_clean_workspace_bytes": [c_l, c_i, c_i],
    "mumpy_mask_clean_u8_fwd": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_l, c_i, c_i, c_f],
})


def library_path() -> str:
    """MUMPY_HIP_LIB=<file> overrides; MUMPY_TUNING=1 selects the diagnostics build (tools/gemm_shapes.py & co: the only build
    whose kernels' A/B hooks read MUMPY_GEMM_* / MUMPY_WA_* variables).  This choice is the binding's, not the library's."""
    if "MUMPY_HIP_LIB" in os.environ:
        return os.environ["MUMPY_HIP_LIB"]
    name = "libmumpy_hip_tuning.so" if os.environ.get("MUMPY_TUNING", "0") == "1" else "libmumpy_hip.so"
    return os.path.join(_PKG, "lib", name)


def tuning_library_path() -> str:
    """The diagnostics build (same sources, -DMUMPY_TUNING): its planner / kernel A/B hooks read MUMPY_* environment variables.
    Select it for a process with MUMPY_HIP_LIB=<this path>; the shipped library reads no environment variable."""
    return os.path.join(_PKG, "lib", "libmumpy_hip_tuning.so")


def build_library(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", os.path.join(_PKG, "csrc"), "-j8", "all", "tuning"], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode:
        raise RuntimeError("building libmumpy_hip.so failed (see output above)")
    return library_path()


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"libmumpy_hip.so not found at {path}: the HIP kernels are the only implementation of this package "
            "(no CPU/torch fallback). Build it with `python __graft_entry__.py` or `make -C <pkg>/csrc`.")
    lib = ctypes.CDLL(path)
    lib.mumpy_last_error.restype = ctypes.c_char_p
    lib.mumpy_last_route.restype = ctypes.c_char_p      # (AttributeError here or below = the library is stale: fail loudly)
    lib.mumpy_last_route.argtypes = []
    for s in SURFACES + [PERTURB, PHOTOMETRIC, GEOMETRIC, POSTPROCESS]:
        version = getattr(lib, s.version_fn)
        version.restype, version.argtypes = c_i, []
        if version() != s.version:
            raise RuntimeError(f"{path}: {s.version_fn}() is {version()}, the binding of include/{s.header} expects {s.version}; rebuild")
        for name, args in s.signatures.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = c_l if name.endswith("_bytes") else c_i
    _LIB = lib
    return lib
