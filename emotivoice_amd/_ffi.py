"""ctypes binding of libevhip.so (include/evhip.h, include/evhip_ops.h).

There is NO fallback: if the library has not been built (``python emotivoice_amd/csrc/build.py`` or
``__graft_entry__.build()``) importing this module raises, and ``ev_create`` itself fails when no HIP
device is present.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EVHIP_LIB", os.path.join(_HERE, "csrc", "libevhip.so"))
EV_ABI_VERSION = 7
EV_PREC_F16, EV_PREC_F32, EV_PREC_X3, EV_PREC_MX = 0, 1, 2, 3
EV_FLAG_DEVICE_INPUTS, EV_FLAG_NO_VOCODER, EV_FLAG_WANT_INT16, EV_FLAG_FORCED_DURATIONS = 1, 2, 4, 8
EV_FLAG_DEVICE_MEL = 16      # ev_align: mel / pitch_frames / energy_frames are device pointers (an ev_features_result), the rest host


class ev_config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("n_vocab", C.c_int32), ("n_speaker", C.c_int32), ("n_mels", C.c_int32),
        ("hidden", C.c_int32), ("heads", C.c_int32), ("enc_layers", C.c_int32), ("dec_layers", C.c_int32),
        ("ffn_kernel", C.c_int32), ("bert_dim", C.c_int32), ("dur_layers", C.c_int32), ("pitch_layers", C.c_int32),
        ("energy_layers", C.c_int32), ("var_kernel", C.c_int32), ("var_embed_kernel", C.c_int32), ("n_up", C.c_int32),
        ("up_rates", C.c_int32 * 8), ("up_kernels", C.c_int32 * 8), ("up_init_ch", C.c_int32), ("n_rb", C.c_int32),
        ("rb_kernels", C.c_int32 * 8), ("rb_dils", (C.c_int32 * 4) * 8), ("n_rb_dils", C.c_int32),
        ("sample_rate", C.c_int32), ("decoder_precision", C.c_int32), ("keep_stages", C.c_int32),
        ("token_rate_split", C.c_int32), ("vocoder_chunk_mb", C.c_int32), ("vocoder_streams", C.c_int32),
        ("vocoder_precision", C.c_int32), ("mx_residual", C.c_int32), ("decoder_attention", C.c_int32),
        ("fused_pairs", C.c_int32), ("mx_mrf", C.c_int32), ("decoder_ln_planes", C.c_int32), ("token_splitk", C.c_int32), ("mx_act_format", C.c_int32),
        ("mx_group", C.c_int32),
    ]


class ev_result(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("total_tokens", C.c_int32), ("total_frames", C.c_int64), ("total_samples", C.c_int64),
        ("wav", C.c_void_p), ("wav_i16", C.c_void_p), ("mel", C.c_void_p), ("durations", C.c_void_p),
        ("log_durations", C.c_void_p), ("pitch", C.c_void_p), ("energy", C.c_void_p),
        ("mel_lens", C.POINTER(C.c_int32)), ("mel_offsets", C.POINTER(C.c_int64)),
    ]


EV_PROSODY_MAX_DURATION = 1024


class ev_prosody(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("alpha", C.c_void_p), ("pitch_scale", C.c_void_p),
        ("pitch_shift", C.c_void_p), ("energy_scale", C.c_void_p), ("energy_shift", C.c_void_p), ("pitch", C.c_void_p),
        ("energy", C.c_void_p), ("durations", C.c_void_p),
    ]


EV_ALIGN_MAX_TOKENS, EV_ALIGN_MAX_FRAMES = 2048, 16384


class ev_align_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total_tokens", C.c_int32), ("reserved0", C.c_int32), ("total_frames", C.c_int64),
        ("durations", C.c_void_p), ("pitch", C.c_void_p), ("energy", C.c_void_p), ("score", C.c_void_p),
        ("mel_lens", C.POINTER(C.c_int32)), ("mel_offsets", C.POINTER(C.c_int64)),
    ]


EV_FEATURES_MAX_NFFT, EV_FEATURES_MAX_MELS, EV_FEATURES_MAX_RUN = 2048, 128, 24576


class ev_features_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_fft", C.c_int32), ("hop", C.c_int32), ("n_mels", C.c_int32), ("mel_clip", C.c_float),
        ("energy_floor", C.c_float), ("mel_basis", C.c_void_p), ("window", C.c_void_p),
    ]


class ev_features_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total_frames", C.c_int64), ("mel", C.c_void_p), ("energy", C.c_void_p),
        ("mel_lens", C.POINTER(C.c_int32)), ("mel_offsets", C.POINTER(C.c_int64)),
    ]


EV_PITCH_TILE_FRAMES, EV_PITCH_MAX_WIN, EV_PITCH_MAX_LDS = 8, 2048, 65536


class ev_pitch_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("sample_rate", C.c_int32), ("hop", C.c_int32), ("win", C.c_int32), ("f_min", C.c_float),
        ("f_max", C.c_float), ("threshold", C.c_float), ("silence_rms", C.c_float),
    ]


class ev_pitch_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total_frames", C.c_int64), ("pitch", C.c_void_p), ("f0_hz", C.c_void_p),
        ("aperiodicity", C.c_void_p), ("mel_lens", C.POINTER(C.c_int32)), ("mel_offsets", C.POINTER(C.c_int64)),
    ]


EV_RESAMPLE_MAX_RATIO, EV_RESAMPLE_MAX_TAPS, EV_RESAMPLE_TILE = 1024, 32769, 256


class ev_resample_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("sr_in", C.c_int32), ("sr_out", C.c_int32), ("half_len", C.c_int32), ("taps", C.c_void_p),
        ("trim_frac", C.c_float), ("trim_pad", C.c_int32),
    ]


class ev_resample_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total_samples", C.c_int64), ("wav", C.c_void_p), ("wav_lens", C.POINTER(C.c_int64)),
        ("wav_offsets", C.POINTER(C.c_int64)), ("trim_start", C.POINTER(C.c_int64)), ("trim_end", C.POINTER(C.c_int64)),
    ]


EV_STITCH_MAX_FADE, EV_STITCH_MAX_PAUSE, EV_STITCH_MAX_DOC = 4096, 1 << 24, 1 << 30


class ev_stitch_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("trim_frac", C.c_float), ("trim_abs", C.c_float), ("keep", C.c_int32), ("fade", C.c_int32),
        ("lead", C.c_int32), ("tail", C.c_int32), ("want_i16", C.c_int32),
    ]


class ev_stitch_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch_docs", C.c_int32), ("batch_segs", C.c_int32), ("reserved", C.c_int32), ("total_samples", C.c_int64),
        ("wav", C.c_void_p), ("wav_i16", C.c_void_p), ("doc_lens", C.POINTER(C.c_int64)), ("doc_offsets", C.POINTER(C.c_int64)),
        ("seg_pos", C.POINTER(C.c_int64)), ("seg_start", C.POINTER(C.c_int64)), ("seg_end", C.POINTER(C.c_int64)), ("seg_peak", C.POINTER(C.c_float)),
    ]


EV_COMPARE_CHUNK, EV_COMPARE_FLOOR = 4096, 1e-60


class ev_compare_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total", C.c_int64),
        ("sum_d", C.POINTER(C.c_double)), ("sum_d2", C.POINTER(C.c_double)), ("sum_y", C.POINTER(C.c_double)), ("sum_y2", C.POINTER(C.c_double)),
        ("rel_l2", C.POINTER(C.c_double)), ("rel_l2_ac", C.POINTER(C.c_double)), ("max_abs_d", C.POINTER(C.c_float)),
        ("argmax_d", C.POINTER(C.c_int64)), ("peak_y", C.POINTER(C.c_float)), ("nonfinite", C.POINTER(C.c_int64)),
        ("chunk_d2", C.POINTER(C.c_double)), ("chunk_y2", C.POINTER(C.c_double)), ("chunk_offsets", C.POINTER(C.c_int64)),
    ]


EV_SCORE_MAX_FRAMES, EV_SCORE_MAX_CEPS, EV_SCORE_Q, EV_SCORE_CLAMP, EV_SCORE_LINEAR, EV_SCORE_WORKSPACE = 4096, 32, 65536, 1 << 27, 1, 1 << 30
SCORE_INT_FIELDS = ("path_len", "n_diag", "n_a", "n_b", "n_vv", "n_vu", "n_uv", "n_uu")
SCORE_FLOAT_FIELDS = ("sum_c", "sum_c2", "mcd_db", "f0_rmse_cents", "f0_bias_cents", "vuv_error", "warp")


class ev_score_result(C.Structure):
    _fields_ = ([("struct_size", C.c_uint32), ("batch", C.c_int32), ("n_ceps", C.c_int32), ("linear", C.c_int32), ("total_frames_a", C.c_int64),
                 ("total_frames_b", C.c_int64), ("sum_dist", C.POINTER(C.c_int64))]
                + [(k, C.POINTER(C.c_int32)) for k in SCORE_INT_FIELDS] + [(k, C.POINTER(C.c_double)) for k in SCORE_FLOAT_FIELDS]
                + [(k, C.POINTER(C.c_int32)) for k in ("lens_a", "lens_b", "nonfinite_a", "nonfinite_b")]
                + [("path_offsets", C.POINTER(C.c_int64)), ("path_a", C.c_void_p), ("path_b", C.c_void_p), ("cq_a", C.c_void_p), ("cq_b", C.c_void_p)])


EV_FLAC_WRAP, EV_FLAC_CLAMP, EV_FLAC_MAX_SAMPLES = 0, 1, 1 << 30


class ev_flac_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sample_rate", C.c_int32), ("block_size", C.c_int32), ("max_fixed_order", C.c_int32),
                ("max_partition_order", C.c_int32), ("convert", C.c_int32)]


class ev_flac_ext(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_lpc_order", C.c_int32), ("qlp_precision", C.c_int32), ("md5", C.c_int32), ("reserved", C.c_int32 * 4)]


class ev_flac_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total_bytes", C.c_int64), ("total_frames", C.c_int64),
        ("bytes", C.c_void_p),
        ("stream_offsets", C.POINTER(C.c_int64)), ("stream_frames", C.POINTER(C.c_int64)), ("frame_offsets", C.POINTER(C.c_int64)),
        ("frame_kind", C.POINTER(C.c_uint8)), ("frame_porder", C.POINTER(C.c_uint8)),
    ]


EV_LOUDNESS_MAX_SAMPLES, EV_LOUDNESS_TILE = 1 << 30, 4096
EV_LOUDNESS_UNDEFINED, EV_LOUDNESS_BOOST_LIMITED, EV_LOUDNESS_PEAK_LIMITED = 1, 2, 4


class ev_loudness_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sample_rate", C.c_int32), ("target_lufs", C.c_double), ("max_gain_db", C.c_double),
                ("peak_ceiling", C.c_float), ("want_i16", C.c_int32)]


class ev_loudness_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total", C.c_int64),
        ("wav", C.c_void_p), ("wav_i16", C.c_void_p),
        ("loudness", C.POINTER(C.c_double)), ("rel_threshold", C.POINTER(C.c_double)), ("gain", C.POINTER(C.c_float)), ("peak", C.POINTER(C.c_float)),
        ("flags", C.POINTER(C.c_uint8)), ("nonfinite", C.POINTER(C.c_int64)), ("block_offsets", C.POINTER(C.c_int64)),
        ("block_ms", C.POINTER(C.c_double)), ("block_state", C.POINTER(C.c_uint8)),
    ]


EV_LIMIT_MAX_SAMPLES, EV_LIMIT_MAX_LOOKAHEAD, EV_LIMIT_MAX_HOLD, EV_LIMIT_TILE, EV_LIMIT_MAX_LDS = 1 << 30, 1024, 8192, 4096, 160 * 1024


class ev_limit_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sample_rate", C.c_int32), ("ceiling", C.c_float), ("lookahead", C.c_int32), ("hold", C.c_int32),
                ("want_i16", C.c_int32)]


class ev_limit_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total", C.c_int64),
        ("wav", C.c_void_p), ("wav_i16", C.c_void_p),
        ("true_peak_in", C.POINTER(C.c_float)), ("sample_peak_in", C.POINTER(C.c_float)), ("true_peak_out", C.POINTER(C.c_float)),
        ("sample_peak_out", C.POINTER(C.c_float)), ("min_gain", C.POINTER(C.c_float)), ("limited", C.POINTER(C.c_int64)),
        ("nonfinite", C.POINTER(C.c_int64)),
    ]


EV_DELIVER_F32, EV_DELIVER_S16, EV_DELIVER_ULAW, EV_DELIVER_ALAW, EV_DELIVER_TILE = 0, 1, 2, 3, 1024


class ev_deliver_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sr_in", C.c_int32), ("sr_out", C.c_int32), ("encoding", C.c_int32), ("dither", C.c_int32),
                ("seed", C.c_uint32), ("half_len", C.c_int32), ("taps", C.c_void_p)]


class ev_deliver_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total_bytes", C.c_int64), ("data", C.c_void_p),
        ("byte_offsets", C.POINTER(C.c_int64)), ("n_samples", C.POINTER(C.c_int64)), ("peak", C.POINTER(C.c_float)), ("clipped", C.POINTER(C.c_int64)),
    ]


EV_DENOISE_MAX_R, EV_DENOISE_BIAS_FRAMES = 8, 88


class ev_denoise_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_fft", C.c_int32), ("hop", C.c_int32), ("want_i16", C.c_int32), ("strength", C.c_float),
                ("window", C.c_void_p)]


class ev_denoise_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total", C.c_int64), ("wav", C.c_void_p), ("wav_i16", C.c_void_p),
        ("lens_out", C.POINTER(C.c_int64)), ("offsets", C.POINTER(C.c_int64)),
    ]


EV_STRETCH_FRAME, EV_STRETCH_HOP, EV_STRETCH_LAGS, EV_STRETCH_MAX_SAMPLES = 512, 256, 256, 1 << 30


class ev_stretch_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("want_int16", C.c_int32)]


class ev_stretch_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total", C.c_int64), ("wav", C.c_void_p), ("wav_i16", C.c_void_p),
        ("lens_out", C.POINTER(C.c_int64)), ("offsets", C.POINTER(C.c_int64)), ("frames", C.POINTER(C.c_int32)),
        ("frame_offsets", C.POINTER(C.c_int64)), ("deltas", C.c_void_p), ("edge_frames", C.POINTER(C.c_int32)),
        ("sum_dist", C.POINTER(C.c_uint64)), ("nonfinite", C.POINTER(C.c_int64)),
    ]


EV_WATERMARK_CHIPS, EV_WATERMARK_BANDS, EV_WATERMARK_MAX_BITS = 768, 48, 16


class ev_watermark_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("key", C.c_uint32), ("want_i16", C.c_int32), ("nbits", C.c_int32), ("payload", C.c_uint32),
                ("strength_db", C.c_float)]


class ev_watermark_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("total", C.c_int64), ("wav", C.c_void_p), ("wav_i16", C.c_void_p),
        ("lens_out", C.POINTER(C.c_int64)), ("offsets", C.POINTER(C.c_int64)),
    ]


class ev_watermark_detect_result(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int32), ("nbits", C.c_int32), ("reserved", C.c_int32),
        ("offset", C.POINTER(C.c_int32)), ("C", C.POINTER(C.c_int32)), ("n", C.POINTER(C.c_int32)), ("bit_C", C.POINTER(C.c_int32)),
        ("bit_n", C.POINTER(C.c_int32)), ("frames", C.POINTER(C.c_int32)), ("frame_offsets", C.POINTER(C.c_int64)), ("q", C.c_void_p),
    ]


class ev_bert_config(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32),
                ("intermediate", C.c_int32), ("max_position", C.c_int32), ("type_vocab", C.c_int32), ("ln_eps", C.c_float),
                ("reserved", C.c_int32 * 8)]


class ev_kernel_stat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int32), ("ms", C.c_float), ("flops", C.c_double),
                ("bytes", C.c_double)]


class ev_launch_record(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("taps", C.c_int32), ("dil", C.c_int32),
                ("ms", C.c_float), ("flops", C.c_double), ("bytes", C.c_double)]


class ev_conv_gemm_desc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("A", C.c_void_p), ("lda", C.c_int), ("W", C.c_void_p), ("W_lo", C.c_void_p), ("bias", C.c_void_p),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("taps", C.c_int), ("dil", C.c_int), ("center", C.c_int),
        ("row_valid", C.c_void_p), ("valid_shift", C.c_int), ("row_seq", C.c_void_p), ("seq_bias", C.c_void_p),
        ("ld_seq_bias", C.c_int), ("act", C.c_int), ("act_slope", C.c_float), ("pro_lrelu", C.c_int),
        ("pro_slope", C.c_float), ("res", C.c_void_p), ("res_dtype", C.c_int), ("ldres", C.c_int),
        ("out_scale", C.c_float), ("acc32", C.c_void_p), ("ldacc", C.c_int), ("post_lrelu", C.c_int),
        ("post_slope", C.c_float), ("out16", C.c_void_p), ("out32", C.c_void_p), ("ldo", C.c_int),
        ("out32_before_post", C.c_int), ("reserved0", C.c_int),
        ("add16_a", C.c_void_p), ("add16_b", C.c_void_p), ("ldadd", C.c_int), ("ksplit", C.c_int),
        ("W_mx", C.c_void_p), ("mx_scratch", C.c_void_p), ("mx_scratch_size", C.c_size_t),
        ("mx_x4", C.c_void_p * 2), ("mx_xs", C.c_void_p * 2), ("mx_xs_stride", C.c_uint), ("polyphase_cout", C.c_int),
        ("mxo_h", C.c_void_p), ("mxo_q4", C.c_void_p * 2), ("mxo_qs", C.c_void_p * 2), ("mxo_qs_stride", C.c_uint),
        ("mxo_logC", C.c_int), ("mxo_slope", C.c_float), ("reserved3", C.c_int),
        ("res_x4", C.c_void_p), ("res_xs", C.c_void_p), ("res_xs_stride", C.c_uint), ("res_inv_slope", C.c_float),
        ("acc_h", C.c_void_p), ("acc_x4", C.c_void_p), ("acc_xs", C.c_void_p), ("acc_xs_stride", C.c_uint), ("mxo_partial", C.c_int),
    ]


class ev_res_pair_desc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p),
                ("M", C.c_int), ("k", C.c_int), ("dil", C.c_int), ("gmin", C.c_int), ("gmax", C.c_int),
                ("w1_mx", C.c_void_p), ("w2_mx", C.c_void_p), ("epi", ev_conv_gemm_desc)]


# every symbol include/evhip.h and include/evhip_ops.h declare: (restype, argtypes)
_P = C.c_void_p
SIGNATURES = {
    "ev_default_config": (None, [C.POINTER(ev_config)]),
    "ev_abi_info": (C.c_int, [C.POINTER(C.c_size_t)]),
    "ev_create": (C.c_int, [C.c_int, C.POINTER(ev_config), C.POINTER(_P)]),
    "ev_destroy": (None, [_P]),
    "ev_last_error": (C.c_char_p, [_P]),
    "ev_set_stream": (C.c_int, [_P, _P]),
    "ev_load_weights": (C.c_int, [_P, _P, C.c_size_t, C.c_char_p]),
    "ev_load_weights_device": (C.c_int, [_P, _P, C.c_size_t, C.c_char_p]),
    "ev_synthesize": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, C.c_float, C.c_uint32, C.POINTER(ev_result)]),
    "ev_synthesize_prosody": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, C.c_float, C.POINTER(ev_prosody), C.c_uint32, C.POINTER(ev_result)]),
    "ev_align": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_uint32, C.POINTER(ev_align_result)]),
    "ev_default_features_config": (None, [C.POINTER(ev_features_config)]),
    "ev_features_setup": (C.c_int, [_P, C.POINTER(ev_features_config)]),
    "ev_features": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_float, C.c_float, C.c_uint32, C.POINTER(ev_features_result)]),
    "ev_default_pitch_config": (None, [C.POINTER(ev_pitch_config)]),
    "ev_pitch": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.POINTER(ev_pitch_config), C.c_float, C.c_float, C.c_uint32, C.POINTER(ev_pitch_result)]),
    "ev_default_resample_config": (None, [C.POINTER(ev_resample_config)]),
    "ev_resample_design": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _P, C.c_int]),
    "ev_resample_setup": (C.c_int, [_P, C.POINTER(ev_resample_config)]),
    "ev_resample": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_uint32, C.POINTER(ev_resample_result)]),
    "ev_default_stitch_config": (None, [C.POINTER(ev_stitch_config)]),
    "ev_stitch_ramp": (C.c_int, [C.c_int, _P]),
    # n, seg_doc, pause_after in; pos, fl, fr, doc_lens out: HOST arrays
    "ev_stitch_plan": (C.c_int, [C.c_int, _P, _P, _P, C.POINTER(ev_stitch_config), _P, _P, _P, _P]),
    "ev_stitch": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, C.POINTER(ev_stitch_config), C.c_uint32, C.POINTER(ev_stitch_result)]),
    # lens is a HOST array; a and b are host pointers, or device pointers with EV_FLAG_DEVICE_INPUTS
    "ev_compare": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_uint32, C.POINTER(ev_compare_result)]),
    "ev_default_flac_config": (None, [C.POINTER(ev_flac_config)]),
    "ev_flac_bound": (C.c_int64, [C.c_int64, C.c_int]),      # host only
    # lens is a HOST array; pcm is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS
    "ev_flac": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.POINTER(ev_flac_config), C.c_uint32, C.POINTER(ev_flac_result)]),
    "ev_default_flac_ext": (None, [C.POINTER(ev_flac_ext)]),
    "ev_flac_lpc": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.POINTER(ev_flac_config), C.POINTER(ev_flac_ext), C.c_uint32, C.POINTER(ev_flac_result)]),
    "ev_default_loudness_config": (None, [C.POINTER(ev_loudness_config)]),
    "ev_loudness_design": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),      # host only
    # lens is a HOST array; wav is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS
    "ev_loudness": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.POINTER(ev_loudness_config), C.c_uint32, C.POINTER(ev_loudness_result)]),
    "ev_default_limit_config": (None, [C.POINTER(ev_limit_config)]),
    "ev_limit_design": (C.c_int, [C.c_int, _P]),      # host only
    # lens and gains are HOST arrays; wav is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS
    "ev_limit": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.POINTER(ev_limit_config), C.c_uint32, C.POINTER(ev_limit_result)]),
    "ev_default_deliver_config": (None, [C.POINTER(ev_deliver_config)]),
    "ev_deliver_setup": (C.c_int, [_P, C.POINTER(ev_deliver_config)]),
    "ev_deliver": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.c_uint32, C.POINTER(ev_deliver_result)]),
    "ev_default_denoise_config": (None, [C.POINTER(ev_denoise_config)]),
    "ev_denoise_setup": (C.c_int, [_P, C.POINTER(ev_denoise_config), _P]),      # bias: a HOST array or None
    "ev_denoise_bias": (C.c_int, [_P, _P]),
    # lens and strengths are HOST arrays; wav is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS
    "ev_denoise": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.c_uint32, C.POINTER(ev_denoise_result)]),
    "ev_default_stretch_config": (None, [C.POINTER(ev_stretch_config)]),
    "ev_stretch_window": (C.c_int, [_P]),      # host only
    "ev_stretch_plan": (C.c_int, [C.c_int, _P, _P, _P, _P]),      # host only; the message of a rejection: ev_last_error(None)
    # lens and lens_out are HOST arrays; wav is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS
    "ev_stretch": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.POINTER(ev_stretch_config), C.c_uint32, C.POINTER(ev_stretch_result)]),
    "ev_default_watermark_config": (None, [C.POINTER(ev_watermark_config)]),
    "ev_watermark_pattern": (C.c_int, [C.c_uint32, C.c_int, C.c_uint32, _P]),      # host only
    # lens, payloads, nbits and strengths_db are HOST arrays; wav is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS
    "ev_watermark": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.POINTER(ev_watermark_config), _P, _P, _P, C.c_uint32, C.POINTER(ev_watermark_result)]),
    "ev_watermark_detect": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(ev_watermark_detect_result)]),
    "ev_score_design": (C.c_int, [C.c_int, C.c_int, _P]),      # host only
    # lens is a HOST array; mel and f0_hz are host pointers, or device pointers with EV_FLAG_DEVICE_INPUTS
    "ev_score_load": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_uint32]),
    "ev_score": (C.c_int, [_P, C.c_uint32, C.POINTER(ev_score_result)]),
    "ev_score_plan": (C.c_int, [C.c_int, _P, _P, _P, _P]),      # host only
    "ev_set_forced_durations": (C.c_int, [_P, _P, C.c_int64]),
    "ev_vocoder": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_uint32, C.POINTER(ev_result)]),
    "ev_get_stage": (C.c_int64, [_P, C.c_char_p, _P, C.c_size_t]),
    "ev_set_profiling": (C.c_int, [_P, C.c_int]),
    "ev_get_timing": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_float)]),
    "ev_kernel_stat_count": (C.c_int, [_P]),
    "ev_get_kernel_stat": (C.c_int, [_P, C.c_int, C.POINTER(ev_kernel_stat)]),
    "ev_memcpy_d2h": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "ev_launch_record_count": (C.c_int, [_P]),
    "ev_get_launch_record": (C.c_int, [_P, C.c_int, C.POINTER(ev_launch_record)]),
    "ev_default_bert_config": (None, [C.POINTER(ev_bert_config)]),
    "ev_style_load_weights": (C.c_int, [_P, C.POINTER(ev_bert_config), _P, C.c_size_t]),
    "ev_style_embed": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_uint32, _P]),
    "ev_op_conv_gemm": (C.c_int, [C.POINTER(ev_conv_gemm_desc), _P]),
    "ev_op_conv_gemm_group3": (C.c_int, [C.POINTER(ev_conv_gemm_desc), C.c_int, _P]),
    "ev_op_mx_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ev_op_mx_scratch_planes": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),      # host only: six addresses / the scale stride
    "ev_op_resblock_pair_c32": (C.c_int, [C.POINTER(ev_res_pair_desc), _P]),
    "ev_op_resblock_pair_c64": (C.c_int, [C.POINTER(ev_res_pair_desc), _P]),
    "ev_op_resblock_pair_c32_mx": (C.c_int, [C.POINTER(ev_res_pair_desc), _P]),
    "ev_op_resblock_pair_c64_mx": (C.c_int, [C.POINTER(ev_res_pair_desc), _P]),
    "ev_op_layernorm": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_float, _P, _P, _P, _P, C.c_float, _P, _P]),
    "ev_op_layernorm_planes": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_float, _P, _P, _P, _P, _P, _P, C.c_uint, _P]),
    "ev_op_attention": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P]),
    "ev_op_embed_pe": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, C.c_float, _P, _P, C.c_int, C.c_int, _P]),
    "ev_op_bert_embed": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P]),
    "ev_op_bert_pooler": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "ev_op_cond_vector": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ev_op_var_embed_add": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ev_op_prosody_tracks": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P, C.c_int, _P]),
    "ev_op_durations": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, _P, _P, _P, _P, _P, _P, _P]),
    "ev_op_durations_prosody": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "ev_op_gauss_upsample": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, _P, _P, C.c_int, C.c_int, _P]),
    "ev_op_mel_to_rows": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ev_op_conv_post": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_float, C.c_int, C.c_float, _P, C.c_int, _P, C.c_int, C.c_int, _P]),
    "ev_op_row_maps": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_int, _P]),
    "ev_op_pack_rows": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int64, _P, _P]),
    "ev_op_wav_to_i16": (C.c_int, [_P, _P, C.c_int64, _P]),
    "ev_op_pe_extend": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    # the per-utterance arrays of the two aligner ops are HOST arrays (the wrapper builds the device table)
    "ev_op_align_score": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "ev_op_align_mas": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # wav_lens, mel_basis and window are HOST arrays (the wrapper packs the basis planes)
    "ev_op_stft_mel": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P, _P, _P]),
    # wav_lens / frames are HOST arrays
    "ev_op_pitch_yin": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P, _P, _P]),
    "ev_op_pitch_fill": (C.c_int, [_P, C.c_int, _P, C.c_float, C.c_float, _P, _P]),
    # wav_lens / lens / out_lens / trim_start / trim_end and the taps are HOST arrays
    "ev_op_resample": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P]),
    "ev_op_trim": (C.c_int, [_P, C.c_int, _P, C.c_float, C.c_int, _P, _P, _P, _P, _P]),
    # everything but wav / out / out_i16 is a HOST array
    "ev_op_stitch_scan": (C.c_int, [_P, C.c_int, _P, _P, C.c_float, C.c_float, _P, _P, _P, _P]),
    "ev_op_flac_encode": (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(ev_flac_config), _P, _P, _P, _P, _P]),
    "ev_op_flac_lpc": (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(ev_flac_config), C.c_int, C.c_int, _P, _P, _P, _P]),
    # lens, gains and the per-segment outputs are HOST arrays; wav, r, out, out_i16 and s are device buffers
    "ev_op_limit_peak": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_float, _P, _P, _P, _P, _P]),
    "ev_op_limit_apply": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    # wav_lens, frames and window are HOST arrays (the wrappers pack the tables)
    "ev_op_stft_gain": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    "ev_op_istft": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "ev_op_stitch_mix": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P]),
}

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build the HIP extension first (python emotivoice_amd/csrc/build.py). "
                "emotivoice_amd has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        # a stale library (or a stale copy of this file) must fail here with the rebuild hint, not with a bare "undefined symbol" from the
        # binding loop below and not by mis-parsing a descriptor later: ev_abi_info is resolved and checked BEFORE any other symbol
        mine = (C.sizeof(ev_config), C.sizeof(ev_result), C.sizeof(ev_conv_gemm_desc), C.sizeof(ev_res_pair_desc))
        hint = "rebuild with python emotivoice_amd/csrc/build.py"
        try:
            abi_info = l.ev_abi_info
        except AttributeError:
            raise ImportError(f"{LIB_PATH} predates ev_abi_info (ABI < 2); this binding is ABI {EV_ABI_VERSION}: {hint}") from None
        abi_info.restype, abi_info.argtypes = SIGNATURES["ev_abi_info"]
        sizes = (C.c_size_t * 4)()
        ver = abi_info(sizes)
        if ver != EV_ABI_VERSION or tuple(sizes) != mine:
            raise ImportError(f"{LIB_PATH}: ABI version {ver} / struct sizes {tuple(sizes)} do not match this binding "
                              f"({EV_ABI_VERSION} / {mine}): {hint}")
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(l, name)
            except AttributeError:
                raise ImportError(f"{LIB_PATH} does not export {name} although it reports ABI {ver}: {hint}") from None
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib
