"""ctypes binding of libmvp_hip.so (C ABI declared in include/mvp_hip.h).

The product path has NO fallback: if the HIP library is missing or an op returns an error
code, a Python exception is raised.  PyTorch is used only for device memory and streams;
every entry point receives raw device pointers + the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MVP_LIB: diagnostic override (A/B builds of the same ABI, e.g. tools/tn_bench.py); the product default is the in-tree library
LIB_PATH = os.environ.get("MVP_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "libmvp_hip.so")

PREC_BF16 = 1
PREC_BF16X3 = 3
PREC_F16X2 = 2  # two fp16 products per GEMM contraction over compensated fp16 pairs (ops.split_f16_comp / ops.f16x2_weight): mvp_hip.h
ACT_NONE, ACT_GELU, ACT_RELU, ACT_QUICK_GELU, ACT_GELU_TANH = 0, 1, 2, 3, 4  # MVP_ACT_*
RESIZE_NEAREST, RESIZE_BILINEAR, RESIZE_BICUBIC = 0, 1, 2
PAIR_SEPARATE, PAIR_A_ILV32, PAIR_W_ILV32 = 0, 1, 2  # mvp_gemm_args.pair_layout (bit flags)
BN_ACT_NONE, BN_ACT_SIGMOID, BN_ACT_TANH = 0, 1, 2  # MVP_BN_ACT_*
BN_ACT_WORKSPACE_BYTES, BCE_WORKSPACE_BYTES = 98304, 8192  # MVP_BN_ACT_WORKSPACE_BYTES, MVP_BCE_WORKSPACE_BYTES
BN_RUNNING_MAX = 8  # MVP_BN_RUNNING_MAX: modules per mvp_bn_running_update_n launch
TILES_SHARED, TILES_NO_PP, TILES_NO_UNI = 1, 2, 4
ROUTE_PP, ROUTE_TILE, ROUTE_SPLITK, ROUTE_CONV = 1, 2, 3, 4  # MVP_GEMM_ROUTE_*: mvp_gemm_route_t.family
ATT_V_BF16_PAIR, ATT_V_F16, ATT_V_F16_QK_F16 = 0, 1, 2  # MVP_ATT_V_*: mvp_attention_args.v_format

_vp = C.c_void_p
_i = C.c_int
_f = C.c_float
_i64 = C.c_int64


class MvpError(RuntimeError):
    pass


STRUCTS = {}  # C struct name in include/mvp_hip.h -> its ctypes mirror below; tests/test_abi.py holds each to the header field by field


class Struct(C.Structure):
    def __init_subclass__(cls, c_name: str, **kw):
        super().__init_subclass__(**kw)
        STRUCTS[c_name] = cls


class Info(Struct, c_name="mvp_info_t"):
    _fields_ = [("abi_version", _i), ("device_count", _i), ("gfx950", _i), ("cu_count", _i), ("arch", C.c_char * 64)]


class SplitArgs(Struct, c_name="mvp_split_bf16_args"):
    _fields_ = [("src", _vp), ("hi", _vp), ("lo", _vp), ("n", _i64)]


class PatchGatherArgs(Struct, c_name="mvp_patch_gather_args"):
    _fields_ = [("images", _vp), ("out_hi", _vp), ("out_lo", _vp), ("B", _i), ("C", _i), ("H", _i), ("W", _i),
                ("P", _i), ("gh", _i), ("gw", _i), ("pad_top", _i), ("pad_left", _i)]


class GemmArgs(Struct, c_name="mvp_gemm_args"):
    _fields_ = [("a_hi", _vp), ("a_lo", _vp), ("w_hi", _vp), ("w_lo", _vp), ("bias", _vp), ("residual", _vp),
                ("out_f32", _vp), ("out_hi", _vp), ("out_lo", _vp), ("M", _i), ("N", _i), ("K", _i),
                ("lda", _i), ("ldw", _i), ("ldr", _i), ("ldo", _i), ("ldob", _i), ("act", _i), ("precision", _i),
                ("row_group", _i), ("row_group_stride", _i), ("row_group_off", _i), ("res_row_mod", _i),
                ("conv", _i), ("cH", _i), ("cW", _i), ("cC", _i), ("cHo", _i), ("cWo", _i), ("ckh", _i), ("ckw", _i),
                ("cstride", _i), ("cpad", _i), ("cup", _i), ("zero_page", _vp), ("relu_mask", _vp), ("out_mask", _vp), ("ldm", _i), ("mask_mode", _i),
                ("residual2", _vp), ("act_after_res", _i), ("splitk", _i), ("splitk_ws", _vp), ("splitk_ws_bytes", _i64),
                ("residual_hi", _vp), ("residual_lo", _vp), ("tile_policy", _i), ("pair_layout", _i), ("out_pair_layout", _i),
                ("out_f16_col0", _i)]


class LayerNormArgs(Struct, c_name="mvp_layernorm_args"):
    _fields_ = [("x", _vp), ("gamma", _vp), ("beta", _vp), ("out_hi", _vp), ("out_lo", _vp), ("out_f32", _vp),
                ("M", _i), ("C", _i), ("eps", _f), ("out_layout", _i), ("out_f16", _i)]


class AttentionArgs(Struct, c_name="mvp_attention_args"):
    _fields_ = [("qkv_hi", _vp), ("qkv_lo", _vp), ("out_hi", _vp), ("out_lo", _vp), ("B", _i), ("N", _i), ("H", _i),
                ("ld_qkv", _i), ("ld_out", _i), ("scale", _f), ("precision", _i), ("out_layout", _i), ("v_format", _i), ("out_f16", _i)]


class AttentionBiasArgs(Struct, c_name="mvp_attention_bias_args"):  # attention with a dense per-head logit bias (added within ABI 8)
    _fields_ = [("att", AttentionArgs), ("bias", _vp), ("bias_head_stride", _i64), ("ld_bias", _i)]


class GatherRowsArgs(Struct, c_name="mvp_gather_rows_args"):  # row gather of 16-bit pair buffers by an index table (added within ABI 8)
    _fields_ = [("in_hi", _vp), ("in_lo", _vp), ("out_hi", _vp), ("out_lo", _vp), ("idx", _vp), ("rows", _i), ("rows_in", _i), ("cols", _i),
                ("ld_in", _i), ("ld_out", _i)]


class RelposTermsArgs(Struct, c_name="mvp_relpos_terms_args"):  # SAM's decomposed relative-position terms (added within ABI 8)
    _fields_ = [("qkv", _vp), ("out_hi", _vp), ("out_lo", _vp), ("rel", _vp), ("rh", _vp), ("rw", _vp), ("rel_bh_stride", _i64),
                ("M", _i), ("N", _i), ("H", _i), ("Qh", _i), ("Qw", _i), ("Kh", _i), ("Kw", _i), ("ld_in", _i), ("ld_out", _i), ("ld_rel", _i),
                ("precision", _i), ("v_format", _i)]


class AttentionRelposArgs(Struct, c_name="mvp_attention_relpos_args"):  # attention with the decomposed bias (added within ABI 8)
    _fields_ = [("att", AttentionArgs), ("rel", _vp), ("rel_bh_stride", _i64), ("ld_rel", _i), ("Kh", _i), ("Kw", _i)]


class ClsRowsArgs(Struct, c_name="mvp_cls_rows_args"):
    _fields_ = [("cls", _vp), ("pos0", _vp), ("x", _vp), ("B", _i), ("N", _i), ("C", _i)]


class GemmScaledArgs(Struct, c_name="mvp_gemm_scaled_args"):  # LayerScale in the GEMM epilogue (ABI 7 addition)
    _fields_ = [("gemm", GemmArgs), ("col_scale", _vp)]


class GemmRoute(Struct, c_name="mvp_gemm_route_t"):  # the kernel mvp_gemm_bias_act_res runs (ABI 8)
    _fields_ = [("family", _i), ("bm", _i), ("bn", _i), ("bk", _i), ("split", _i), ("nstage", _i), ("nw", _i), ("wnw", _i)]


class PatchGatherLdArgs(Struct, c_name="mvp_patch_gather_ld_args"):  # padded patch rows (ABI 7 addition)
    _fields_ = [("g", PatchGatherArgs), ("ldk", _i)]


class PrefixRowsArgs(Struct, c_name="mvp_prefix_rows_args"):  # CLS + register rows (ABI 7 addition)
    _fields_ = [("cls", _vp), ("pos0", _vp), ("reg", _vp), ("x", _vp), ("B", _i), ("N", _i), ("C", _i), ("R", _i)]


class Rope2dQkvArgs(Struct, c_name="mvp_rope2d_qkv_args"):  # 2-D RoPE between the qkv GEMM and attention (added within ABI 8)
    _fields_ = [("qkv", _vp), ("out_hi", _vp), ("out_lo", _vp), ("cos_tab", _vp), ("sin_tab", _vp), ("M", _i), ("N", _i), ("H", _i),
                ("n_prefix", _i), ("gh", _i), ("gw", _i), ("tab_rows", _i), ("ld_in", _i), ("ld_out", _i), ("precision", _i), ("v_format", _i)]


class BnTokensArgs(Struct, c_name="mvp_bn_tokens_args"):
    _fields_ = [("x", _vp), ("gamma", _vp), ("beta", _vp), ("running_mean", _vp), ("running_var", _vp), ("stats", _vp),
                ("nchw", _vp), ("tok_hi", _vp), ("tok_lo", _vp), ("ld_tok", _i), ("col_off", _i),
                ("tokT_hi", _vp), ("tokT_lo", _vp), ("ldT", _i),
                ("workspace", _vp), ("workspace_bytes", _i64),
                ("B", _i), ("N", _i), ("C", _i), ("hw", _i), ("eps", _f), ("momentum", _f), ("mode", _i), ("cls_out", _vp), ("num_batches_tracked", _vp),
                ("defer_running", _i), ("groups", _i), ("stats_gstride", _i64), ("nchw_gstride", _i64), ("tok_gstride", _i64), ("cls_gstride", _i64)]


class BnRunningUpdateArgs(Struct, c_name="mvp_bn_running_update_args"):
    _fields_ = [("stats", _vp), ("running_mean", _vp), ("running_var", _vp), ("num_batches_tracked", _vp), ("C", _i), ("momentum", _f)]


class PackNchwArgs(Struct, c_name="mvp_pack_nchw_args"):
    _fields_ = [("nchw", _vp), ("tok_hi", _vp), ("tok_lo", _vp), ("ld_tok", _i), ("col_off", _i),
                ("tokT_hi", _vp), ("tokT_lo", _vp), ("ldT", _i), ("B", _i), ("C", _i), ("hw", _i)]


class ResizeArgs(Struct, c_name="mvp_resize_args"):
    _fields_ = [("src", _vp), ("dst", _vp), ("planes", _i), ("Hi", _i), ("Wi", _i), ("Ho", _i), ("Wo", _i),
                ("mode", _i), ("align_corners", _i), ("channels_last", _i), ("C", _i), ("scale_h", _f), ("scale_w", _f)]


class DepthPredictArgs(Struct, c_name="mvp_depth_predict_args"):
    _fields_ = [("logits", _vp), ("depth", _vp), ("inv_sum", _vp), ("grad_depth", _vp), ("grad_logits", _vp),
                ("P", _i64), ("K", _i), ("min_depth", _f), ("max_depth", _f), ("kind", _i)]


class DepthLossArgs(Struct, c_name="mvp_depth_loss_args"):
    _fields_ = [("pred", _vp), ("target", _vp), ("loss", _vp), ("grad_pred", _vp), ("workspace", _vp),
                ("workspace_bytes", _i64), ("B", _i), ("HW", _i64), ("w_sig", _f), ("w_grad", _f), ("max_depth", _f),
                ("eps", _f), ("sigma", _f)]


class AngularLossArgs(Struct, c_name="mvp_angular_loss_args"):
    _fields_ = [("pred", _vp), ("gt", _vp), ("mask", _vp), ("loss", _vp), ("grad_pred", _vp), ("workspace", _vp),
                ("workspace_bytes", _i64), ("B", _i), ("Cp", _i), ("HW", _i64), ("eps", _f)]


class ColsumArgs(Struct, c_name="mvp_colsum_args"):
    _fields_ = [("x", _vp), ("out", _vp), ("M", _i), ("N", _i), ("ld", _i), ("accumulate", _i), ("workspace", _vp), ("workspace_bytes", _i64)]


class AdamWArgs(Struct, c_name="mvp_adamw_args"):
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("hyper", _vp), ("n", _i64),
                ("beta1", _f), ("beta2", _f), ("eps", _f), ("weight_decay", _f), ("grad_scale", _f),
                ("lr", _f), ("bias_c1", _f), ("bias_c2", _f)]


class CorrArgmaxArgs(Struct, c_name="mvp_corr_argmax_args"):
    _fields_ = [("src_feat", _vp), ("tgt_feat", _vp), ("kp_xy", _vp), ("out_xy", _vp), ("out_val", _vp),
                ("workspace", _vp), ("workspace_bytes", _i64), ("C", _i), ("h", _i), ("w", _i), ("K", _i), ("heat_out", _vp)]


class Argmax2dArgs(Struct, c_name="mvp_argmax_2d_args"):
    _fields_ = [("x", _vp), ("out_xy", _vp), ("K", _i), ("h", _i), ("w", _i), ("max_value", _i)]


class KnnRatioArgs(Struct, c_name="mvp_knn_ratio_args"):  # top-2 cosine nearest neighbours + ratio test (added within ABI 8)
    _fields_ = [("src_feat", _vp), ("tgt_feat", _vp), ("src_valid", _vp), ("tgt_valid", _vp), ("nn_idx", _vp), ("dist", _vp), ("weight", _vp),
                ("n_valid", _vp), ("workspace", _vp), ("workspace_bytes", _i64), ("C", _i), ("N0", _i), ("N1", _i)]


class PointcloudSampleArgs(Struct, c_name="mvp_pointcloud_sample_args"):  # zero-padded bilinear sampling at projected points (added within ABI 8)
    _fields_ = [("feat", _vp), ("pc", _vp), ("K", _vp), ("out", _vp), ("valid", _vp), ("C", _i), ("fh", _i), ("fw", _i), ("N", _i),
                ("H", _i), ("W", _i), ("ld_out", _i)]


class TwoafcArgs(Struct, c_name="mvp_twoafc_args"):  # pooled cosine scoring of 2AFC triplets + running confusion counts (added within ABI 8)
    _fields_ = [("ref", _vp), ("left", _vp), ("right", _vp), ("label", _vp), ("sim", _vp), ("pred", _vp), ("counts", _vp),
                ("workspace", _vp), ("workspace_bytes", _i64), ("ld", _i64), ("B", _i), ("C", _i), ("HW", _i), ("accumulate", _i)]


class PixelScoreArgs(Struct, c_name="mvp_pixel_score_args"):  # PSNR / SSIM scoring of 2AFC triplets + running confusion counts (added within ABI 8)
    _fields_ = [("ref", _vp), ("left", _vp), ("right", _vp), ("label", _vp), ("sim", _vp), ("pred", _vp), ("counts", _vp),
                ("workspace", _vp), ("workspace_bytes", _i64), ("ld", _i64), ("B", _i), ("C", _i), ("H", _i), ("W", _i), ("metric", _i),
                ("accumulate", _i)]


class NcutAffinityArgs(Struct, c_name="mvp_ncut_affinity_args"):  # MaskCut: normalised, painted-out patch affinity (added within ABI 8)
    _fields_ = [("feats", _vp), ("painted", _vp), ("active", _vp), ("A", _vp), ("sums", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
                ("ldf", _i64), ("Bimg", _i), ("C", _i), ("N", _i)]


class NcutThresholdArgs(Struct, c_name="mvp_ncut_threshold_args"):  # MaskCut: 2-means threshold, bit matrix, degrees (added within ABI 8)
    _fields_ = [("A", _vp), ("sums", _vp), ("active", _vp), ("tau", _vp), ("bits", _vp), ("deg", _vp), ("rounds", _vp),
                ("Bimg", _i), ("N", _i), ("max_rounds", _i)]


class NcutFiedlerArgs(Struct, c_name="mvp_ncut_fiedler_args"):  # MaskCut: LDS-resident normalised-cut eigen-solver (added within ABI 8)
    _fields_ = [("bits", _vp), ("deg", _vp), ("active", _vp), ("v", _vp), ("lambda", _vp), ("residual", _vp), ("iters", _vp),
                ("converged", _vp), ("Bimg", _i), ("N", _i), ("max_iters", _i), ("r_tol", _f), ("mix_tol", _f)]


class NcutPartitionArgs(Struct, c_name="mvp_ncut_partition_args"):  # MaskCut: bipartition, seed component, painting (added within ABI 8)
    _fields_ = [("v", _vp), ("prev_mask", _vp), ("active", _vp), ("pass_mask", _vp), ("painted", _vp), ("union_mask", _vp), ("seed", _vp),
                ("Bimg", _i), ("h", _i), ("w", _i), ("use_prev", _i)]


class Dwconv7LnArgs(Struct, c_name="mvp_dwconv7_ln_args"):  # ConvNeXt: depthwise 7x7 + LayerNorm -> fc1's A operand (added within ABI 8)
    _fields_ = [("x", _vp), ("weight", _vp), ("bias", _vp), ("gamma", _vp), ("beta", _vp), ("out_hi", _vp), ("out_lo", _vp), ("out_f32", _vp),
                ("B", _i), ("H", _i), ("W", _i), ("C", _i), ("ldx", _i), ("eps", _f), ("out_layout", _i), ("out_f16", _i)]


class GrnArgs(Struct, c_name="mvp_grn_args"):  # ConvNeXt V2: global response normalisation, statistics and apply (added within ABI 8)
    _fields_ = [("h", _vp), ("gamma", _vp), ("beta", _vp), ("G", _vp), ("N", _vp), ("out_hi", _vp), ("out_lo", _vp), ("out_f32", _vp),
                ("workspace", _vp), ("workspace_bytes", _i64), ("B", _i), ("HW", _i), ("C4", _i), ("out_layout", _i)]


class CrfFilterArgs(Struct, c_name="mvp_crf_filter_args"):  # dense CRF: exact all-pairs Gaussian filtering of F fields (added within ABI 8)
    _fields_ = [("rgb", _vp), ("in", _vp), ("active", _vp), ("out", _vp), ("in_stride", _i64), ("out_stride", _i64),
                ("B", _i), ("F", _i), ("H", _i), ("W", _i), ("inv_var_xy", _f), ("inv_var_rgb", _f)]


class CrfUpdateArgs(Struct, c_name="mvp_crf_update_args"):  # dense CRF: normalisers, Q^0, one mean-field step, MAP (added within ABI 8)
    _fields_ = [("mask", _vp), ("active", _vp), ("norm_g", _vp), ("norm_b", _vp), ("ones_g", _vp), ("ones_b", _vp), ("filt_g", _vp),
                ("filt_b", _vp), ("q", _vp), ("x_g", _vp), ("x_b", _vp), ("map", _vp), ("stride", _i64), ("N", _i64),
                ("B", _i), ("F", _i), ("mode", _i), ("w_g", _f), ("w_b", _f)]


class MaskFinishArgs(Struct, c_name="mvp_mask_finish_args"):  # hole filling, IoU rule and union of the refined masks (added within ABI 8)
    _fields_ = [("map", _vp), ("ref", _vp), ("active", _vp), ("refined", _vp), ("kept", _vp), ("union_mask", _vp), ("stride", _i64),
                ("B", _i), ("F", _i), ("H", _i), ("W", _i)]


class AugmentStatsArgs(Struct, c_name="mvp_augment_stats_args"):  # training augmentation: the contrast mean's partial sums (added within ABI 8)
    _fields_ = [("image", _vp), ("params", _vp), ("partials", _vp), ("partials_bytes", _i64), ("B", _i), ("H", _i), ("W", _i), ("image_u8", _i)]


class AugmentApplyArgs(Struct, c_name="mvp_augment_apply_args"):  # training augmentation: jitter + shared gather + normalise (added within ABI 8)
    _fields_ = [("image", _vp), ("depth", _vp), ("snorm", _vp), ("params", _vp), ("partials", _vp), ("out_image", _vp), ("out_depth", _vp),
                ("out_snorm", _vp), ("partials_bytes", _i64), ("B", _i), ("H", _i), ("W", _i), ("Ho", _i), ("Wo", _i), ("image_u8", _i),
                ("mean_r", _f), ("mean_g", _f), ("mean_b", _f), ("std_r", _f), ("std_g", _f), ("std_b", _f)]


class SwigluArgs(Struct, c_name="mvp_swiglu_args"):  # DINOv2 ViT-g/14: silu(gate) * value -> the padded A operand of w3 (added within ABI 8)
    _fields_ = [("h12", _vp), ("out_hi", _vp), ("out_lo", _vp), ("out_f32", _vp), ("M", _i), ("H", _i), ("ld_in", _i), ("ld_out", _i),
                ("out_layout", _i), ("out_f16", _i)]


class TaskPrepareArgs(Struct, c_name="mvp_task_prepare_args"):  # Taskonomy: raw target + raw mask -> training tensors (added within ABI 8)
    _fields_ = [("target_raw", _vp), ("mask_raw", _vp), ("target", _vp), ("valid", _vp), ("B", _i), ("H", _i), ("W", _i), ("Cs", _i), ("Ct", _i),
                ("bits", _i), ("clamp_max", _f)]


class MaskedL1Args(Struct, c_name="mvp_masked_l1_args"):  # MaskedL1Loss and its gradient (added within ABI 8)
    _fields_ = [("pred", _vp), ("target", _vp), ("valid", _vp), ("loss", _vp), ("grad_pred", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
                ("B", _i), ("C", _i), ("Cm", _i), ("HW", _i64)]


class TaskMetricsArgs(Struct, c_name="mvp_task_metrics_args"):  # per-image AbsRel / threshold sums of the Taskonomy metrics (added within ABI 8)
    _fields_ = [("pred", _vp), ("target", _vp), ("valid", _vp), ("out", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
                ("B", _i), ("C", _i), ("Cm", _i), ("HW", _i64), ("form", _i), ("t1", _f), ("t2", _f), ("t3", _f)]


class F16ScanArgs(Struct, c_name="mvp_f16_scan_args"):  # range scan of an fp16-form pair operand into a 16-byte record (added within ABI 8)
    _fields_ = [("hi", _vp), ("record", _vp), ("rows", _i), ("col0", _i), ("cols", _i), ("ld", _i), ("layout", _i)]


class BnActArgs(Struct, c_name="mvp_bn_act_args"):  # BatchNorm2d + activation on a few-channel map, forward and backward (added within ABI 8)
    _fields_ = [("x", _vp), ("y", _vp), ("gamma", _vp), ("beta", _vp), ("running_mean", _vp), ("running_var", _vp), ("num_batches_tracked", _vp),
                ("stats", _vp), ("grad_y", _vp), ("grad_x", _vp), ("grad_gamma", _vp), ("grad_beta", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
                ("B", _i), ("HW", _i64), ("C", _i), ("ld", _i), ("n", _i64), ("eps", _f), ("momentum", _f), ("act", _i), ("training", _i), ("accumulate", _i)]


class BceLossArgs(Struct, c_name="mvp_bce_loss_args"):  # nn.BCELoss (mean) and its gradient (added within ABI 8)
    _fields_ = [("pred", _vp), ("target", _vp), ("loss", _vp), ("grad_pred", _vp), ("workspace", _vp), ("workspace_bytes", _i64), ("N", _i64)]


class BinaryCountsArgs(Struct, c_name="mvp_binary_counts_args"):  # TP / FP / FN / TN of a thresholded prediction (added within ABI 8)
    _fields_ = [("pred", _vp), ("gt", _vp), ("counts", _vp), ("G", _i), ("n", _i64), ("threshold", _f)]


class ScaleShiftArgs(Struct, c_name="mvp_scale_shift_args"):
    _fields_ = [("x", _vp), ("scale_shift", _vp), ("grad_out", _vp), ("out", _vp), ("B", _i), ("HW", _i64), ("lo", _f), ("hi", _f),
                ("clamp", _i), ("backward", _i)]


class MetricsBreakdownArgs(Struct, c_name="mvp_metrics_breakdown_args"):
    _fields_ = [("pred", _vp), ("gt", _vp), ("seg", _vp), ("scale_shift", _vp), ("level_sums", _vp), ("seg_sums", _vp),
                ("workspace", _vp), ("workspace_bytes", _i64), ("B", _i), ("H", _i), ("W", _i), ("Cp", _i), ("num_levels", _i), ("num_ids", _i),
                ("t1", _f), ("t2", _f), ("t3", _f)]


class ConvWeightPackArgs(Struct, c_name="mvp_conv_weight_pack_args"):
    _fields_ = [("w", _vp), ("out_hi", _vp), ("out_lo", _vp), ("Cout", _i), ("Cin", _i), ("kh", _i), ("kw", _i), ("mode", _i)]


class UpsampleClArgs(Struct, c_name="mvp_upsample_cl_args"):
    _fields_ = [("src", _vp), ("dst_f32", _vp), ("dst_hi", _vp), ("dst_lo", _vp), ("B", _i), ("H", _i), ("W", _i), ("C", _i),
                ("f", _i), ("backward", _i)]


class UpconvBoxsumArgs(Struct, c_name="mvp_upconv_boxsum_args"):
    _fields_ = [("g", _vp), ("out_hi", _vp), ("out_lo", _vp), ("B", _i), ("H", _i), ("W", _i), ("C", _i), ("f", _i)]


class UpconvGatherArgs(Struct, c_name="mvp_upconv_gather_args"):
    _fields_ = [("t", _vp), ("bias", _vp), ("out_f32", _vp), ("out_hi", _vp), ("out_lo", _vp), ("out_mask", _vp),
                ("B", _i), ("H", _i), ("W", _i), ("C", _i), ("f", _i), ("act", _i)]


class DepthMetricsArgs(Struct, c_name="mvp_depth_metrics_args"):
    _fields_ = [("pred", _vp), ("gt", _vp), ("out", _vp), ("scale_shift", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
                ("B", _i), ("HW", _i64), ("scale_invariant", _i)]


class SnormMetricsArgs(Struct, c_name="mvp_snorm_metrics_args"):
    _fields_ = [("pred", _vp), ("gt", _vp), ("out", _vp), ("workspace", _vp), ("workspace_bytes", _i64), ("B", _i), ("Cp", _i),
                ("HW", _i64), ("t1", _f), ("t2", _f), ("t3", _f)]


class LinearBinsArgs(Struct, c_name="mvp_linear_bins_args"):
    _fields_ = [("l0", _vp), ("depth", _vp), ("inv_sum", _vp), ("gate", _vp), ("grad_depth", _vp), ("grad_l0", _vp),
                ("B", _i), ("h", _i), ("w", _i), ("K", _i), ("f", _i), ("min_depth", _f), ("max_depth", _f)]


class Im2colArgs(Struct, c_name="mvp_im2col_args"):
    _fields_ = [("src", _vp), ("out_hi", _vp), ("out_lo", _vp), ("B", _i), ("C", _i), ("H", _i), ("W", _i), ("Ho", _i), ("Wo", _i),
                ("kh", _i), ("kw", _i), ("stride", _i), ("pad", _i), ("ldk", _i)]


class MaxpoolClArgs(Struct, c_name="mvp_maxpool_cl_args"):
    _fields_ = [("src", _vp), ("dst_f32", _vp), ("dst_hi", _vp), ("dst_lo", _vp), ("B", _i), ("H", _i), ("W", _i), ("C", _i),
                ("Ho", _i), ("Wo", _i), ("k", _i), ("stride", _i), ("pad", _i)]


class StemArgs(Struct, c_name="mvp_stem_args"):
    _fields_ = [("images", _vp), ("w_hi", _vp), ("w_lo", _vp), ("bias", _vp), ("out_f32", _vp), ("out_hi", _vp), ("out_lo", _vp),
                ("B", _i), ("H", _i), ("W", _i), ("precision", _i)]


class MaskSplitArgs(Struct, c_name="mvp_mask_split_args"):
    _fields_ = [("src", _vp), ("mask", _vp), ("dst_f32", _vp), ("dst_hi", _vp), ("dst_lo", _vp), ("M", _i64), ("N", _i),
                ("lds", _i), ("ldm", _i), ("ldo", _i), ("relu_mask_out", _vp)]


class GemmTnArgs(Struct, c_name="mvp_gemm_tn_args"):
    _fields_ = [("g_hi", _vp), ("g_lo", _vp), ("x_hi", _vp), ("x_lo", _vp), ("partial", _vp), ("dw", _vp), ("zero_page", _vp),
                ("M", _i64), ("Cout", _i), ("Cin", _i), ("ldg", _i), ("ldx", _i), ("H", _i), ("W", _i), ("Ho", _i), ("Wo", _i),
                ("kh", _i), ("kw", _i), ("stride", _i), ("pad", _i), ("up", _i), ("splits", _i), ("accumulate", _i), ("precision", _i)]


# every exported symbol of include/mvp_hip.h: name -> args struct (None = special signature)
SYMBOLS = {
    "mvp_get_info": None,
    "mvp_strerror": None,
    "mvp_sizeof": None,
    "mvp_split_bf16": SplitArgs,
    "mvp_patch_gather": PatchGatherArgs,
    "mvp_gemm_bias_act_res": GemmArgs,
    "mvp_gemm_splitk_workspace_bytes": None,
    "mvp_gemm_route": None,
    "mvp_layernorm_fwd": LayerNormArgs,
    "mvp_attention_fwd": AttentionArgs,
    "mvp_cls_rows": ClsRowsArgs,
    "mvp_bn_tokens_workspace_bytes": None,
    "mvp_bn_tokens_to_nchw_fwd": BnTokensArgs,
    "mvp_bn_running_update": BnRunningUpdateArgs,
    "mvp_bn_running_update_n": None,
    "mvp_pack_nchw_tokens": PackNchwArgs,
    "mvp_resize_fwd": ResizeArgs,
    "mvp_resize_bwd": ResizeArgs,
    "mvp_resize_aa_fwd": ResizeArgs,
    "mvp_depth_predict_fwd": DepthPredictArgs,
    "mvp_depth_predict_bwd": DepthPredictArgs,
    "mvp_depth_loss_workspace_bytes": None,
    "mvp_depth_loss_fwd_bwd": DepthLossArgs,
    "mvp_angular_loss_fwd_bwd": AngularLossArgs,
    "mvp_colsum_workspace_bytes": None,
    "mvp_colsum": ColsumArgs,
    "mvp_adamw_step": AdamWArgs,
    "mvp_corr_argmax": CorrArgmaxArgs,
    "mvp_corr_workspace_bytes": None,
    "mvp_argmax_2d": Argmax2dArgs,
    "mvp_scale_shift": ScaleShiftArgs,
    "mvp_metrics_breakdown_workspace_bytes": None,
    "mvp_metrics_breakdown": MetricsBreakdownArgs,
    "mvp_conv_weight_pack": ConvWeightPackArgs,
    "mvp_upsample_nearest_cl": UpsampleClArgs,
    "mvp_upconv3_grad_boxsum": UpconvBoxsumArgs,
    "mvp_upconv3_fwd_gather": UpconvGatherArgs,
    "mvp_mask_split": MaskSplitArgs,
    "mvp_metrics_workspace_bytes": None,
    "mvp_depth_metrics": DepthMetricsArgs,
    "mvp_snorm_metrics": SnormMetricsArgs,
    "mvp_linear_bins_fwd": LinearBinsArgs,
    "mvp_linear_bins_bwd": LinearBinsArgs,
    "mvp_im2col_nchw": Im2colArgs,
    "mvp_maxpool_cl": MaxpoolClArgs,
    "mvp_stem7x7_pool": StemArgs,
    "mvp_gemm_pp": GemmArgs,
    "mvp_gemm_tn_workspace_bytes": None,
    "mvp_gemm_tn_conv": GemmTnArgs,
    "mvp_gemm_scaled": GemmScaledArgs,
    "mvp_patch_gather_ld": PatchGatherLdArgs,
    "mvp_prefix_rows": PrefixRowsArgs,
    "mvp_rope2d_qkv": Rope2dQkvArgs,
    "mvp_attention_bias_fwd": AttentionBiasArgs,
    "mvp_gather_rows": GatherRowsArgs,
    "mvp_relpos_terms": RelposTermsArgs,
    "mvp_attention_relpos_fwd": AttentionRelposArgs,
    "mvp_knn_ratio": KnnRatioArgs,
    "mvp_knn_workspace_bytes": None,
    "mvp_bn_act_fwd": BnActArgs,
    "mvp_bn_act_bwd": BnActArgs,
    "mvp_bce_loss_fwd_bwd": BceLossArgs,
    "mvp_binary_counts": BinaryCountsArgs,
    "mvp_pointcloud_sample": PointcloudSampleArgs,
    "mvp_twoafc_score": TwoafcArgs,
    "mvp_twoafc_workspace_bytes": None,
    "mvp_pixel_score": PixelScoreArgs,
    "mvp_pixel_score_workspace_bytes": None,
    "mvp_ncut_workspace_bytes": None,
    "mvp_ncut_affinity": NcutAffinityArgs,
    "mvp_ncut_threshold": NcutThresholdArgs,
    "mvp_ncut_fiedler": NcutFiedlerArgs,
    "mvp_ncut_partition": NcutPartitionArgs,
    "mvp_dwconv7_ln_fwd": Dwconv7LnArgs,
    "mvp_grn_workspace_bytes": None,
    "mvp_grn_stats": GrnArgs,
    "mvp_grn_apply": GrnArgs,
    "mvp_crf_filter": CrfFilterArgs,
    "mvp_crf_update": CrfUpdateArgs,
    "mvp_mask_finish": MaskFinishArgs,
    "mvp_augment_partials_bytes": None,
    "mvp_augment_stats": AugmentStatsArgs,
    "mvp_augment_apply": AugmentApplyArgs,
    "mvp_swiglu_fwd": SwigluArgs,
    "mvp_task_prepare": TaskPrepareArgs,
    "mvp_masked_l1_fwd_bwd": MaskedL1Args,
    "mvp_task_metrics": TaskMetricsArgs,
    "mvp_f16_range_scan": F16ScanArgs,
}

# the exports that are not `int f(const args*, void* stream)` (None above): name -> (restype, argtypes)
SIGNATURES = {
    "mvp_get_info": (_i, [C.POINTER(Info)]),
    "mvp_strerror": (C.c_char_p, [_i]),
    "mvp_sizeof": (_i, [C.c_char_p]),
    "mvp_gemm_splitk_workspace_bytes": (_i64, [_i, _i, _i]),
    "mvp_gemm_route": (_i, [C.POINTER(GemmArgs), C.POINTER(GemmRoute)]),
    "mvp_bn_tokens_workspace_bytes": (_i64, [_i, _i]),
    "mvp_bn_running_update_n": (_i, [C.POINTER(BnRunningUpdateArgs), _i, _vp]),
    "mvp_depth_loss_workspace_bytes": (_i64, [_i, _i64]),
    "mvp_colsum_workspace_bytes": (_i64, [_i, _i]),
    "mvp_corr_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "mvp_metrics_breakdown_workspace_bytes": (_i64, [_i, _i, _i]),
    "mvp_metrics_workspace_bytes": (_i64, [_i]),
    "mvp_gemm_tn_workspace_bytes": (_i64, [_i, _i, _i, _i, _i]),
    "mvp_knn_workspace_bytes": (_i64, [_i, _i, _i]),
    "mvp_twoafc_workspace_bytes": (_i64, [_i, _i, _i]),
    "mvp_pixel_score_workspace_bytes": (_i64, [_i, _i, _i, _i, _i]),
    "mvp_ncut_workspace_bytes": (_i64, [_i, _i]),
    "mvp_grn_workspace_bytes": (_i64, [_i, _i, _i]),
    "mvp_augment_partials_bytes": (_i64, [_i]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libmvp_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MvpError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C midvision-probe_amd/csrc`). There is no CPU fallback for the product path."
        )
    lib = C.CDLL(LIB_PATH)
    assert set(SIGNATURES) == {name for name, st in SYMBOLS.items() if st is None}
    for name, st in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = (_i, [C.POINTER(st), _vp]) if st is not None else SIGNATURES[name]
    _lib = lib
    return lib


def info() -> Info:
    out = Info()
    check(load().mvp_get_info(C.byref(out)), "mvp_get_info")
    return out


def check(code: int, what: str) -> None:
    if code != 0:
        raise MvpError(f"{what} failed: {load().mvp_strerror(code).decode()} (code {code})")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr() -> int:
    """Handle of the calling thread's current HIP stream on the current device.  Every launch asks for it: the raw accessors cost
    ~0.3 us against ~8 us for torch.cuda.current_stream().cuda_stream (a tenth of a probe step's host time, tools/micro/host_profile.py)."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise MvpError("expected a device tensor (the HIP path has no CPU fallback)")
    return t.data_ptr()


# Diagnostic hook (tools/micro/chain_timeline.py): when a list is installed, EVERY entry-point call is bracketed by HIP events recorded on
# the stream it is launched on -> (name, stream, start event, end event).  None in production.
TRACE_CALLS = None


def call(name: str, args: C.Structure) -> None:
    if TRACE_CALLS is None:
        check(getattr(load(), name)(C.byref(args), stream_ptr()), name)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(getattr(load(), name)(C.byref(args), stream_ptr()), name)
    e1.record()
    TRACE_CALLS.append((name, stream_ptr(), e0, e1))
