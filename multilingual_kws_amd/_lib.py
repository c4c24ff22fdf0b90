"""ctypes loader for lib/libmkws_hip.so (C-ABI: include/mkws.h).  Fails loudly; no fallback."""
import ctypes
import itertools
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MKWS_LIB selects another build of the same library (e.g. the phase-timing build of tools/README.md)
LIB_PATH = os.environ.get("MKWS_LIB") or os.path.join(_HERE, "lib", "libmkws_hip.so")

MKWS_OK = 0
MKWS_ERR_EXCHANGE = -7
ABI_VERSION = 5


class MkwsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmkws_hip error {code}: {msg}")
        self.code = code


class MkwsValueError(MkwsError, ValueError):
    """A wrapper's own refusal of what the library refuses as well (MKWS_ERR_INVALID_ARG), made before any device call: a ValueError like
    every refusal of a wrapper, and still the MkwsError a caller of the earlier wrapper caught."""

    def __init__(self, msg):
        MkwsError.__init__(self, -1, msg)


class FrontendCfg(ctypes.Structure):
    """mkws_frontend_cfg (include/mkws.h)."""
    _fields_ = [
        ("sample_rate", ctypes.c_int32), ("window_size_ms", ctypes.c_int32),
        ("window_step_ms", ctypes.c_int32), ("num_channels", ctypes.c_int32),
        ("upper_band_limit", ctypes.c_float), ("lower_band_limit", ctypes.c_float),
        ("smoothing_bits", ctypes.c_int32), ("even_smoothing", ctypes.c_float),
        ("odd_smoothing", ctypes.c_float), ("min_signal_remaining", ctypes.c_float),
        ("enable_pcan", ctypes.c_int32), ("pcan_strength", ctypes.c_float),
        ("pcan_offset", ctypes.c_float), ("gain_bits", ctypes.c_int32),
        ("enable_log", ctypes.c_int32), ("scale_shift", ctypes.c_int32),
    ]


class DetectEvent(ctypes.Structure):
    """mkws_detect_event (include/mkws.h)."""
    _fields_ = [("window", ctypes.c_int32), ("fired", ctypes.c_int32), ("score", ctypes.c_double)]


class ResampleCfg(ctypes.Structure):
    """mkws_resample_cfg (include/mkws.h)."""
    _fields_ = [("rate_in", ctypes.c_int32), ("rate_out", ctypes.c_int32), ("zero_crossings", ctypes.c_int32),
                ("kaiser_beta", ctypes.c_float), ("rolloff", ctypes.c_float)]


class LoudnessCfg(ctypes.Structure):
    """mkws_loudness_cfg (include/mkws.h)."""
    _fields_ = [("rate", ctypes.c_int32), ("mode", ctypes.c_int32), ("target_lufs", ctypes.c_double), ("true_peak_db", ctypes.c_double),
                ("headroom_db", ctypes.c_double), ("zero_crossings", ctypes.c_int32), ("kaiser_beta", ctypes.c_float), ("rolloff", ctypes.c_float)]


class SpectralCfg(ctypes.Structure):
    """mkws_spectral_cfg (include/mkws.h)."""
    _fields_ = [("sample_rate", ctypes.c_int32), ("window_size_samples", ctypes.c_int32), ("window_stride_samples", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("num_features", ctypes.c_int32), ("filterbank_channels", ctypes.c_int32),
                ("lower_frequency_limit", ctypes.c_float), ("upper_frequency_limit", ctypes.c_float), ("average_window_width", ctypes.c_int32)]


class PcmItem(ctypes.Structure):
    """mkws_pcm_item (include/mkws.h)."""
    _fields_ = [("byte_offset", ctypes.c_int64), ("n_frames", ctypes.c_int64), ("out_offset", ctypes.c_int64), ("out_len", ctypes.c_int64),
                ("format", ctypes.c_int32), ("channels", ctypes.c_int32), ("channel", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class PcmEncodeItem(ctypes.Structure):
    """mkws_pcm_encode_item (include/mkws.h)."""
    _fields_ = [("src_offset", ctypes.c_int64), ("src_len", ctypes.c_int64), ("start", ctypes.c_int64), ("n_frames", ctypes.c_int64),
                ("byte_offset", ctypes.c_int64), ("fade_in", ctypes.c_int64), ("fade_out", ctypes.c_int64), ("gain", ctypes.c_float),
                ("format", ctypes.c_int32)]


class StreamItem(ctypes.Structure):
    """mkws_stream_item (include/mkws.h)."""
    _fields_ = [("src_offset", ctypes.c_int64), ("src_len", ctypes.c_int64), ("start", ctypes.c_int64), ("n_frames", ctypes.c_int64),
                ("out_start", ctypes.c_int64), ("fade_in", ctypes.c_int64), ("fade_out", ctypes.c_int64), ("gain", ctypes.c_float),
                ("stream", ctypes.c_int32)]


class StreamDesc(ctypes.Structure):
    """mkws_stream_desc (include/mkws.h)."""
    _fields_ = [("out_offset", ctypes.c_int64), ("n_out", ctypes.c_int64), ("bed_offset", ctypes.c_int64), ("bed_len", ctypes.c_int64),
                ("bed_start", ctypes.c_int64), ("max_frames", ctypes.c_int64), ("first_item", ctypes.c_int32), ("n_items", ctypes.c_int32)]


class W2v2Cfg(ctypes.Structure):
    """mkws_w2v2_cfg (include/mkws.h)."""
    _fields_ = [("conv_dim", ctypes.c_int32 * 7), ("conv_kernel", ctypes.c_int32 * 7), ("conv_stride", ctypes.c_int32 * 7),
                ("hidden_size", ctypes.c_int32), ("num_hidden_layers", ctypes.c_int32), ("num_attention_heads", ctypes.c_int32),
                ("intermediate_size", ctypes.c_int32), ("num_conv_pos_embeddings", ctypes.c_int32),
                ("num_conv_pos_embedding_groups", ctypes.c_int32), ("layer_norm_eps", ctypes.c_float), ("group_norm", ctypes.c_int32),
                ("conv_bias", ctypes.c_int32), ("stable_layer_norm", ctypes.c_int32), ("exact_gelu", ctypes.c_int32)]


# every symbol include/mkws.h declares: (name, restype, argtypes)
_P, _I, _F, _SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
_CFG = ctypes.POINTER(FrontendCfg)
_RCFG, _I64 = ctypes.POINTER(ResampleCfg), ctypes.c_int64
_SCFG, _IP = ctypes.POINTER(SpectralCfg), ctypes.POINTER(ctypes.c_int)
_WCFG = ctypes.POINTER(W2v2Cfg)
_LCFG = ctypes.POINTER(LoudnessCfg)
SYMBOLS = [
    ("mkws_abi_version", _I, []),
    ("mkws_last_error", ctypes.c_char_p, []),
    ("mkws_build_arch", ctypes.c_char_p, []),
    ("mkws_frontend_default_cfg", None, [_CFG]),
    ("mkws_frontend_host_table", _I, [_CFG, _I, _P, _SZ]),
    ("mkws_frontend_num_frames", _I, [_CFG, _I]),
    ("mkws_frontend_create", _I, [_CFG, _I, ctypes.POINTER(_P)]),
    ("mkws_frontend_destroy", None, [_P]),
    ("mkws_frontend_forward_f32", _I, [_P, _P, _I, _I, _P, _P, _P]),
    ("mkws_frontend_forward_i16", _I, [_P, _P, _I, _I, _P, _P, _P]),
    ("mkws_frontend_stream_f32", _I, [_P, _P, _I, _I, _I, _P, _P, _I, _P]),
    ("mkws_frontend_live_state_bytes", _SZ, [_P, _I, _I, _I]),
    ("mkws_frontend_live_push_f32", _I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    ("mkws_frontend_live_push_many_f32", _I, [_P, _P, _SZ, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    ("mkws_spectral_default_cfg", None, [_SCFG]),
    ("mkws_spectral_geometry", _I, [_SCFG, _IP, _IP, _IP]),
    ("mkws_spectral_num_frames", _I, [_SCFG, _I]),
    ("mkws_spectral_host_table", _I, [_SCFG, _I, _P, _SZ]),
    ("mkws_spectral_create", _I, [_SCFG, _I, ctypes.POINTER(_P)]),
    ("mkws_spectral_destroy", None, [_P]),
    ("mkws_spectral_forward_f32", _I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    ("mkws_spectral_forward_i16", _I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    ("mkws_spectral_stream_f32", _I, [_P, _P, _I, _I, _I, _P, _I, _P]),
    ("mkws_resample_default_cfg", None, [_RCFG, _I, _I]),
    ("mkws_resample_geometry", _I, [_RCFG, _P]),
    ("mkws_resample_host_taps", _I, [_RCFG, _P, _SZ]),
    ("mkws_resample_out_samples", _I64, [_RCFG, _I64]),
    ("mkws_resample_create", _I, [_RCFG, ctypes.POINTER(_P)]),
    ("mkws_resample_destroy", None, [_P]),
    ("mkws_resample_forward", _I, [_P, _P, _I, _I, _I64, _I64, _I, _P, _I64, _P]),
    ("mkws_resample_live_in_samples", _I, [_P, _I]),
    ("mkws_resample_live_state_bytes", _SZ, [_P]),
    ("mkws_resample_live_push_many", _I, [_P, _P, _SZ, _I, _P, _P, _I, _I, _P, _P]),
    ("mkws_loudness_default_cfg", None, [_LCFG, _I]),
    ("mkws_loudness_coeffs", _I, [_LCFG, _P]),
    ("mkws_loudness_geometry", _I, [_LCFG, _P]),
    ("mkws_loudness_create", _I, [_LCFG, _I, _I64, ctypes.POINTER(_P)]),
    ("mkws_loudness_destroy", None, [_P]),
    ("mkws_loudness_measure", _I, [_P, _P, _I, _I, _I64, _I64, _P, _P, _P, _P, _P]),
    ("mkws_loudness_apply", _I, [_P, _P, _I, _I, _I64, _I64, _P, _P, _P, _I64, _P]),
    ("mkws_pcm_frame_bytes", _I, [_I, _I]),
    ("mkws_pcm_decode", _I, [_P, _I64, _P, _I, _I64, _P, _I64, _P, _P]),
    ("mkws_pcm_encode", _I, [_P, _I64, _P, _I, _I64, _P, _I64, _P, _P]),
    ("mkws_stream_mix", _I, [_P, _I64, _P, _I, _P, _I, _P, _I, _I64, _P, _I64, _P, _P]),
    ("mkws_stream_power", _I, [_P, _I64, _P, _I, _P, _I, _I64, _P, _P, _P]),
    ("mkws_stream_bed_gain", _I, [_P, _P, _I, _I64, _P, _P, _P]),
    ("mkws_embed_weight_count", _SZ, []),
    ("mkws_embed_weight_manifest", _I, [ctypes.c_char_p, _SZ]),
    ("mkws_embed_create", _I, [_P, _SZ, _I, ctypes.POINTER(_P)]),
    ("mkws_embed_destroy", None, [_P]),
    ("mkws_embed_forward", _I, [_P, _P, _I, _P, _P]),
    ("mkws_embed_set_option", _I, [_P, ctypes.c_char_p, _I]),
    ("mkws_embed_get_option", _I, [_P, ctypes.c_char_p]),
    ("mkws_embed_profile", _I, [_P, _P, _I, _I, _P, ctypes.c_char_p, _SZ, _P]),
    ("mkws_embed_forward_tap", _I, [_P, _P, _I, ctypes.c_char_p, _P, _SZ, _P]),
    ("mkws_detect_stream", _I, [_P, _I, _I, _I, _I, _I, _P, _P, _I, ctypes.c_double, ctypes.c_double, _I, _I, _P, _I, _P, _P, _P, _P]),
    ("mkws_detect_live_state_bytes", _SZ, [_I, _I, _I]),
    ("mkws_detect_live_step", _I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, ctypes.c_double, ctypes.c_double, _I, _I, _I, _P, _P, _P, _P]),
    ("mkws_detect_live_step_many", _I, [_P, _SZ, _I, _P, _P, _I, _I, _I, _I, _P, _I, ctypes.c_double, ctypes.c_double, _I, _I, _I, _P, _P, _P, _P]),
    ("mkws_detect_live_step_routes", _I, [_P, _SZ, _I, _P, _I, _P, _P, _I, _I, _I, _P, _I, ctypes.c_double, ctypes.c_double, _I, _I, _I, _P, _P, _P, _P]),
    ("mkws_detect_score", _I, [_P, _P, _I, _I, _I, _P, _I, _P, _P, ctypes.c_double, _P, _P]),
    ("mkws_detect_segments", _I, [_P, _I, _P, _I, _I, _I, _I, _P, _P, _I, ctypes.c_double, ctypes.c_double, _I, _I, _P, _I, _P, _P, _P, _P]),
    ("mkws_detect_score_segments", _I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, ctypes.c_double, _P, _P]),
    ("mkws_roc_count", _I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    ("mkws_score_work_bytes", _SZ, [_I, _I]),
    ("mkws_score_accumulate", _I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("mkws_kmeans_fit", _I, [_P, _I, _P, _I, _I, _P, _I, _I, ctypes.c_double, _P, _P, _P, _P, _P, _P]),
    ("mkws_kmeans_nearest", _I, [_P, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P]),
    ("mkws_logreg_work_floats", _SZ, [_I, _I, _I]),
    ("mkws_logreg_fit", _I, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _I, _I, ctypes.c_double, _P, _P, _P, _P, _P, _SZ, _P]),
    ("mkws_logreg_score", _I, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P]),
    ("mkws_lr_l1_work_floats", _SZ, [_I, _I, _I]),
    ("mkws_lr_l1_fit", _I, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _I, ctypes.c_double, _P, _P, _P, _P, _P, _SZ, _P]),
    ("mkws_svc_work_bytes", _SZ, [_I, _I]),
    ("mkws_svc_prepare", _I, [_P, _I, _I, _P, _P, _P, _I, _I, _I, _I, ctypes.c_double, _P, _P, _P, _P, _P, _P]),
    ("mkws_svc_kernel", _I, [_P, _I, _I, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    ("mkws_svc_fit", _I, [_P, _P, _I, _I, _I, _P, ctypes.c_double, _I, _P, _SZ, _P, _P, _P, _P, _P]),
    ("mkws_svc_score", _I, [_P, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    ("mkws_svc_fit_cv", _I, [_P, _P, _P, _I, _I, _I, _I, _P, ctypes.c_double, _I, _P, _SZ, _P, _P, _P, _P]),
    ("mkws_svc_platt", _I, [_P, _P, _I, _I, _I, _P, _P, _P, ctypes.c_double, _P, _P, _P, _P]),
    ("mkws_svc_couple", _I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    ("mkws_soft_vote", _I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    ("mkws_dscnn_param_count", _SZ, [_I]),
    ("mkws_dscnn_weight_manifest", _I, [_I, ctypes.c_char_p, _SZ]),
    ("mkws_dscnn_create", _I, [_P, _SZ, _I, _I, ctypes.POINTER(_P)]),
    ("mkws_dscnn_destroy", None, [_P]),
    ("mkws_dscnn_grid", _I, [_P]),
    ("mkws_dscnn_forward", _I, [_P, _P, _I, _P, _P, _P]),
    ("mkws_dscnn_tap", _I, [_P, _P, _I, _I, _P, _P]),
    ("mkws_w2v2_default_cfg", None, [_WCFG]),
    ("mkws_w2v2_param_count", _SZ, [_WCFG]),
    ("mkws_w2v2_weight_manifest", _I, [_WCFG, ctypes.c_char_p, _SZ]),
    ("mkws_w2v2_num_frames", _I, [_WCFG, _I]),
    ("mkws_w2v2_create", _I, [_WCFG, _P, _SZ, _I, _I, ctypes.POINTER(_P)]),
    ("mkws_w2v2_destroy", None, [_P]),
    ("mkws_w2v2_forward", _I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    ("mkws_w2v2_tap", _I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    # DS-CNN training operators
    ("mkws_op_dscnn_stem_fwd", _I, [_P, _P, _P, _I, _P]),
    ("mkws_op_dscnn_stem_bwd_weight", _I, [_P, _P, _P, _I, _P]),
    ("mkws_op_dropout_fwd", _I, [_P, _P, _I64, _F, ctypes.c_uint64, _P, _I, _P]),
    ("mkws_op_dropout_bwd", _I, [_P, _P, _I64, _F, ctypes.c_uint64, _P, _I, _P]),
    ("mkws_op_dscnn_pool_fwd", _I, [_P, _I, _F, ctypes.c_uint64, _P, _I, _P, _P]),
    ("mkws_op_dscnn_pool_bwd", _I, [_P, _I, _F, ctypes.c_uint64, _P, _I, _P, _P]),
    ("mkws_augment_batch", _I, [_P, _P, _P, ctypes.c_int64, _P, _I, _I, _P, _P]),
    ("mkws_specaug_apply", _I, [_P, _P, _I, _I, _I, _P]),
    ("mkws_specaug_apply_n", _I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    ("mkws_head_create", _I, [_I, _I, _I, _I, ctypes.POINTER(_P)]),
    ("mkws_head_destroy", None, [_P]),
    ("mkws_head_param_count", _I, [_P]),
    ("mkws_head_params", _P, [_P]),
    ("mkws_head_grads", _P, [_P]),
    ("mkws_head_state_floats", _I, [_P]),
    ("mkws_head_grad_count", _I, [_P]),
    ("mkws_head_set_params", _I, [_P, _P, _I, _P]),
    ("mkws_head_get_params", _I, [_P, _P, _I, _P]),
    ("mkws_head_forward", _I, [_P, _P, _I, _P, _P]),
    ("mkws_heads_forward", _I, [ctypes.POINTER(_P), _I, _P, _I, _P, _P]),
    ("mkws_head_loss_grad", _I, [_P, _P, _P, _I, _P, _P]),
    ("mkws_head_adam_step", _I, [_P, _F, _F, _F, _F, _I, _F, _P]),
    ("mkws_head_input_grad", _I, [_P, _P, _I, _P]),
    ("mkws_head_adam_step_dev", _I, [_P, _F, _F, _F, _F, _P, _F, _P]),
    # side-by-side training of several heads
    ("mkws_head_group_create", _I, [ctypes.POINTER(_P), _I, ctypes.POINTER(_P)]),
    ("mkws_head_group_destroy", None, [_P]),
    ("mkws_head_group_size", _I, [_P]),
    ("mkws_head_group_forward_segments", _I, [_P, _P, _I, ctypes.c_int64, _P, _P, _I, _P, _P, _P]),
    ("mkws_head_group_forward_routes", _I, [_P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _P]),
    ("mkws_head_group_loss_grad", _I, [_P, _P, ctypes.c_int64, _P, ctypes.c_int64, _I, _P, _P]),
    ("mkws_head_group_adam_step", _I, [_P, _F, _F, _F, _F, _I, _F, _P]),
    # training operators (backprop_into_embedding)
    ("mkws_train_ctx_create", _I, [_P, _SZ, ctypes.POINTER(_P)]),
    ("mkws_train_ctx_destroy", None, [_P]),
    ("mkws_train_ctx_bind", _I, [_P]),
    ("mkws_op_set_scratch", _I, [_P, _SZ]),
    ("mkws_op_stream_wait", _I, [_P, _P]),
    ("mkws_op_set_option", _I, [ctypes.c_char_p, _I]),
    ("mkws_op_get_option", _I, [ctypes.c_char_p]),
    ("mkws_op_fold_defer", _I, [_I, _P]),
    ("mkws_op_fold_flush", _I, [_P]),
    ("mkws_op_bn_train_fwd", _I, [_P, _I, _I, _P, _P, _F, _I, _F, _P, _P, _P, _P, _P, _P]),
    ("mkws_op_bn_train_fwd_res", _I, [_P, _I, _I, _P, _P, _F, _I, _F, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    ("mkws_op_step_inc", _I, [_P, _P]),
    ("mkws_op_softmax_ce", _I, [_P, _P, _I, _I, _P, _P, _P]),
    ("mkws_op_dense_fwd", _I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    ("mkws_op_adam_dev", _I, [_P, _P, _P, _P, ctypes.c_int64, _F, _F, _F, _F, _P, _F, _P]),
    ("mkws_op_gemm", _I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    ("mkws_op_bn_stats", _I, [_P, _I, _I, _P, _P, _P]),
    ("mkws_op_bn_act_fwd", _I, [_P, _P, _P, _P, _P, _F, _I, _P, _I, _I, _P]),
    ("mkws_op_bn_act_bwd", _I, [_P, _P, _P, _P, _P, _F, _I, _P, _P, _P, _P, _I, _I, _P]),
    ("mkws_op_bn_act_bwd_ex", _I, [_P, _P, _P, _P, _P, _F, _I, _P, _P, _P, _P, _F, _I, _P, _P, _I, _I, _P]),
    ("mkws_op_bn_update_moving", _I, [_P, _P, _P, _P, _F, _I, _I, _P]),
    ("mkws_op_dwconv_fwd", _I, [_P, _P, _P] + [_I] * 10 + [_P]),
    ("mkws_op_conv_bn_fwd", _I, [_P, _P, _P, _I, _I, _I, _P, _P, _F, _I, _F, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    ("mkws_op_dwconv_bn_fwd", _I, [_P, _P, _P] + [_I] * 10 + [_P, _P, _F, _I, _F, _P, _P, _P, _P, _P, _P]),
    ("mkws_op_dwconv_bwd", _I, [_P, _P, _P, _P, _P] + [_I] * 10 + [_P]),
    ("mkws_op_stem_fwd", _I, [_P, _P, _F, _F, _P, _I, _P]),
    ("mkws_op_stem_bwd_weight", _I, [_P, _P, _F, _F, _P, _I, _P]),
    ("mkws_op_pool_hw", _I, [_P, _P, _I, _I, _I, _P]),
    ("mkws_op_scale_channels", _I, [_P, _P, _P, _I, _I, _I, _P]),
    ("mkws_op_se_bwd", _I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    ("mkws_op_se_fwd", _I, [_P] * 11 + [_I, _I, _I, _I, _P]),
    ("mkws_op_se_bwd_fused", _I, [_P] * 17 + [_I, _I, _I, _I, _P]),
    ("mkws_op_se_wgrad", _I, [_P] * 8 + [_I, _I, _I, _P]),
    ("mkws_op_add_bcast", _I, [_P, _P, _F, _I, _I, _I, _P]),
    ("mkws_op_bias_act_fwd", _I, [_P, _P, _I, _P, _I, _I, _P]),
    ("mkws_op_bias_act_bwd", _I, [_P, _P, _I, _P, _P, _I, _I, _P]),
    ("mkws_op_row_scale_add", _I, [_P, _P, _P, _P, _I, ctypes.c_int64, _P]),
    ("mkws_op_axpy", _I, [_P, _P, _F, ctypes.c_int64, _P]),
    ("mkws_op_adam", _I, [_P, _P, _P, _P, ctypes.c_int64, _F, _F, _F, _F, _I, _F, _P]),
]

_lib = None


def lib():
    """Returns the loaded library; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C multilingual_kws_amd/csrc`).  multilingual_kws_amd has no CPU fallback.")
        try:
            # Load order matters: PyTorch brings its own HIP runtime.  If this library (linked against
            # /opt/rocm's libamdhip64) is loaded first, the process ends up with a runtime that sees no device
            # on the GPU box; with torch first both share torch's.  torch is required anyway (device memory).
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)       # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        got = L.mkws_abi_version()
        if got != ABI_VERSION:
            raise ImportError(f"{LIB_PATH} has ABI version {got}, this package binds version {ABI_VERSION}: rebuild it (make -C multilingual_kws_amd/csrc)")
        _lib = L
    return _lib


_generation = itertools.count(1)


def next_generation():
    """Process-unique serial for every handle wrapper: caches keyed on raw handle addresses add it, so that a handle destroyed and
    re-created at the same address is not mistaken for the old one."""
    return next(_generation)


def forget_graphs(obj):
    """Called by the wrappers' close(): drops captured graphs that point into the handle being destroyed."""
    import sys
    m = sys.modules.get("multilingual_kws_amd.embedding.batch_streaming_analysis")
    if m is not None:
        m._BatchGraph.forget(obj)


def check(code):
    if code < 0:
        raise MkwsError(code, lib().mkws_last_error().decode("utf-8", "replace"))
    return code


def indexed_device(device=None):
    """The torch.device a handle lives on, always with its index ("cuda" and None mean the current device), so that it compares equal
    to the .device of the tensors allocated there."""
    import torch
    d = torch.device(device if device is not None else "cuda")
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def current_stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def pack_words(parts):
    """The host side of "one upload": contiguous numpy arrays of int64, float64 or int32 -> (int64 words, the byte offset of every part).
    8-byte parts go in as their bit patterns; an int32 part is padded with a zero to whole words, so every offset is a multiple of 8.
    An empty part gets the offset of whatever follows it."""
    words, offsets, at = [], [], 0
    for part in parts:
        a = part if part.ndim == 1 else part.reshape(-1)
        if a.dtype.char not in "lqdi":
            raise TypeError(f"pack_words takes int64, float64 and int32 parts, not {a.dtype}")
        if a.itemsize == 4 and a.size % 2:
            a = np.concatenate([a, np.zeros(1, np.int32)])
        offsets.append(at)
        words.append(a.view(np.int64))
        at += a.nbytes
    return (np.concatenate(words) if words else np.zeros(0, np.int64)), offsets


def upload_words(parts, device):
    """pack_words and its single non-blocking copy to `device` -> (the device tensor, which owns the memory, [device pointer of every part])."""
    import torch
    words, offsets = pack_words(parts)
    d_words = torch.from_numpy(words).to(device, non_blocking=True)
    return d_words, [d_words.data_ptr() + o for o in offsets]


def word_layout(parts):
    """The host side of "one copy back": parts (name, dtype, shape) of int32, float32 or float64 laid out one after the other in ONE
    buffer of 4-byte words -> [first word of every part, ..., total words].  An 8-byte part must start on an even word (put them first)."""
    at = [0]
    for name, dtype, shape in parts:
        size = np.dtype(dtype).itemsize
        if np.dtype(dtype).char not in "ifd":
            raise TypeError(f"word_layout takes int32, float32 and float64 parts, not {np.dtype(dtype)} ({name})")
        if size == 8 and at[-1] % 2:
            raise ValueError(f"8-byte part {name} would start at word {at[-1]}: put the 8-byte parts first")
        at.append(at[-1] + int(np.prod(shape, dtype=np.int64)) * (size // 4))
    return at


class OutputWords:
    """Every output of a call in ONE device buffer of 4-byte words (word_layout), so that they cross in one copy.  Every word starts as 0;
    with fill = {name: int32} those parts are preset and the rest is left for the kernel to write."""

    def __init__(self, parts, device, fill=None):
        import torch
        at = word_layout(parts)
        self.parts = {name: (slice(a, b), np.dtype(dtype), tuple(shape)) for (name, dtype, shape), a, b in zip(parts, at, at[1:])}
        self.d_words = (torch.empty if fill else torch.zeros)(at[-1], dtype=torch.int32, device=device)
        for name, value in (fill or {}).items():
            self.d_words[self.parts[name][0]] = value

    def ptr(self, name, first=0):
        """Device pointer of element `first` of the flattened part."""
        cut, dtype, _ = self.parts[name]
        return self.d_words.data_ptr() + 4 * cut.start + dtype.itemsize * int(first)

    def fetch(self):
        """The call's one copy back (it synchronises); host() reads from it."""
        self.words = self.d_words.cpu().numpy()

    def host(self, name):
        cut, dtype, shape = self.parts[name]
        return self.words[cut].view(dtype).reshape(shape)

    def device(self, name):
        import torch
        cut, dtype, shape = self.parts[name]
        return self.d_words[cut].view(getattr(torch, dtype.name)).view(shape)
