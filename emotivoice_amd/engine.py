"""Object wrapper over the libevhip.so handle: numpy / raw-pointer in, numpy out.  No torch needed."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _ffi
from .config import EVShapes


class EVError(RuntimeError):
    pass


_PREC = {"f16": _ffi.EV_PREC_F16, "f32": _ffi.EV_PREC_F32, "x3": _ffi.EV_PREC_X3, "mx": _ffi.EV_PREC_MX}


def resolve_precision(precision, decoder_precision, vocoder_precision):
    """``precision`` is the one-knob form: "fast" = fp16 MFMA operands on the frame-rate path (BASELINE.json's bf16 / fp16
    configs; 2.4e-3 on zero-mean waveforms), "strict" = split precision (three fp16 MFMAs per product on hi/lo parts, fp32
    activations: fp32-class accuracy, ~1e-6 relative L2 on the waveform), "mx" = the contract mode: the strict data flow, but the
    generator's layers with >= 128 channels evaluate a product as one fp16 MFMA + two block-scaled fp4 MFMAs for the cross terms
    (waveform ~4e-4 from the reference, inside north_star's 1e-3, at half the matrix work of strict).
    ``decoder_precision`` / ``vocoder_precision`` override it per component.  ``None`` everywhere = "mx", which is also what
    ``ev_default_config`` hands a C caller (ABI 5): "fast" and "strict" are explicit opt-ins."""
    if precision not in (None, "fast", "strict", "mx"):
        raise ValueError("precision must be 'fast', 'strict' or 'mx'")
    base = {None: "mx", "mx": "mx", "strict": "x3", "fast": "f16"}[precision]      # no argument = ev_default_config's own default = the contract mode
    return decoder_precision or base, vocoder_precision or base


def make_ev_config(shapes: EVShapes, decoder_precision: str = "mx", keep_stages: bool = False,
                   token_rate: str = "split", vocoder_chunk_mb: int = 0, vocoder_streams: int = 0,
                   vocoder_precision: str = "mx", mx_residual: str = "planes", decoder_attention: str = "split",
                   fused_pairs: bool = True, mx_mrf: str = "planes", decoder_ln: str = "planes", token_splitk: bool = True,
                   mx_act_format: str = "e5m2", mx_group: bool = True) -> _ffi.ev_config:
    cfg = _ffi.ev_config()
    _ffi.lib().ev_default_config(C.byref(cfg))
    for f in ("n_vocab", "n_speaker", "n_mels", "hidden", "heads", "enc_layers", "dec_layers", "ffn_kernel", "bert_dim",
              "dur_layers", "pitch_layers", "energy_layers", "var_kernel", "var_embed_kernel", "up_init_ch"):
        setattr(cfg, f, int(getattr(shapes, f)))
    cfg.n_up = len(shapes.up_rates)
    for i, (u, k) in enumerate(zip(shapes.up_rates, shapes.up_kernels)):
        cfg.up_rates[i], cfg.up_kernels[i] = int(u), int(k)
    cfg.n_rb = len(shapes.rb_kernels)
    cfg.n_rb_dils = len(shapes.rb_dils[0])
    for j, k in enumerate(shapes.rb_kernels):
        cfg.rb_kernels[j] = int(k)
        for d, v in enumerate(shapes.rb_dils[j]):
            cfg.rb_dils[j][d] = int(v)
    cfg.sample_rate = int(shapes.sr)
    cfg.decoder_precision = _PREC[decoder_precision]
    if vocoder_precision not in ("f16", "x3", "mx"):
        raise ValueError("vocoder_precision must be 'f16', 'x3' or 'mx'")
    cfg.vocoder_precision = _PREC[vocoder_precision]
    cfg.keep_stages = 1 if keep_stages else 0
    cfg.vocoder_chunk_mb = int(vocoder_chunk_mb)
    cfg.vocoder_streams = int(vocoder_streams)
    cfg.token_rate_split = {"split": 1, "f32": 0}[token_rate]
    # engine switches (ev_config; they were environment variables until round 3)
    cfg.mx_residual = {"planes": 0, "fp32": 1}[mx_residual]
    cfg.decoder_attention = {"split": 0, "f32": 1}[decoder_attention]
    cfg.fused_pairs = 0 if fused_pairs else 1
    cfg.mx_mrf = {"planes": 0, "fp32": 1}[mx_mrf]                    # running MRF sum of an MX stage: partial plane sets / an fp32 tensor
    cfg.decoder_ln_planes = {"planes": 0, "fp32": 1}[decoder_ln]     # MX decoder: LayerNorm writes its consumer's plane set / fp32 + a planes pass
    cfg.token_splitk = 0 if token_splitk else 1                       # the token-rate conv-FFN's second conv split-K (shape rule) / one pass
    cfg.mx_act_format = {"e5m2": 0, "fp4": 1}[mx_act_format]          # activation operand of the cross terms where a kernel offers both (fused C = 32 pairs)
    cfg.mx_group = 0 if mx_group else 1                               # same-level convs of a stage's three ResBlocks as one grouped launch / one launch per conv
    return cfg


class EVEngine:
    """One handle = one GPU + one stream + one workspace (include/evhip.h).  Not thread-safe."""

    def __init__(self, shapes: Optional[EVShapes] = None, device_id: int = 0, decoder_precision: Optional[str] = None,
                 keep_stages: bool = False, token_rate: str = "split", vocoder_chunk_mb: int = 0,
                 vocoder_streams: int = 0, vocoder_precision: Optional[str] = None, precision: Optional[str] = None,
                 mx_residual: str = "planes", decoder_attention: str = "split", fused_pairs: bool = True, mx_mrf: str = "planes",
                 decoder_ln: str = "planes", token_splitk: bool = True, mx_act_format: str = "e5m2", mx_group: bool = True):
        self.shapes = shapes or EVShapes()
        self._lib = _ffi.lib()
        self._h = C.c_void_p()
        decoder_precision, vocoder_precision = resolve_precision(precision, decoder_precision, vocoder_precision)
        self.decoder_precision, self.vocoder_precision = decoder_precision, vocoder_precision
        cfg = make_ev_config(self.shapes, decoder_precision, keep_stages, token_rate, vocoder_chunk_mb, vocoder_streams,
                             vocoder_precision, mx_residual, decoder_attention, fused_pairs, mx_mrf, decoder_ln, token_splitk, mx_act_format, mx_group)
        if self._lib.ev_create(device_id, C.byref(cfg), C.byref(self._h)) != 0:
            raise EVError(self._lib.ev_last_error(None).decode())
        self.device_id = device_id
        self._blob_keepalive = None
        self.last: Optional[_ffi.ev_result] = None
        self.feature_config = None                  # set by features_setup()
        self.last_features: Optional[_ffi.ev_features_result] = None
        self.last_pitch: Optional[_ffi.ev_pitch_result] = None
        self.resample_config = None                 # set by resample_setup()
        self.last_resample: Optional[_ffi.ev_resample_result] = None
        self.last_stitch: Optional[_ffi.ev_stitch_result] = None
        self.last_compare: Optional[_ffi.ev_compare_result] = None
        self.last_flac: Optional[_ffi.ev_flac_result] = None
        self.last_loudness: Optional[_ffi.ev_loudness_result] = None
        self.last_limit: Optional[_ffi.ev_limit_result] = None

    # -- lifecycle
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ev_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EVError(self._lib.ev_last_error(self._h).decode())

    def set_stream(self, hip_stream_ptr: int):
        self._check(self._lib.ev_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def set_profiling(self, on: bool):
        self._check(self._lib.ev_set_profiling(self._h, 1 if on else 0))

    # -- weights
    def load_blob(self, blob: bytes, manifest_json: Optional[str] = None):
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        self._check(self._lib.ev_load_weights(self._h, C.cast(buf, C.c_void_p), len(blob),
                                              manifest_json.encode() if manifest_json else None))

    def load_blob_device(self, dptr: int, nbytes: int, keepalive=None):
        """Borrow a blob that already lives in device memory (e.g. after an RCCL broadcast)."""
        self._blob_keepalive = keepalive
        self._check(self._lib.ev_load_weights_device(self._h, C.c_void_p(dptr), nbytes, None))

    # -- SimBERT prompt / content encoder (ev_style_*)
    def style_load(self, blob: bytes, cfg: dict):
        """blob / cfg from packer.pack_bert_state_dict."""
        bc = _ffi.ev_bert_config()
        self._lib.ev_default_bert_config(C.byref(bc))
        for k in ("vocab_size", "hidden", "layers", "intermediate", "max_position", "type_vocab"):
            setattr(bc, k, int(cfg[k]))
        bc.heads = int(cfg.get("heads", bc.hidden // 64))
        bc.ln_eps = float(cfg.get("ln_eps", 1e-12))
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        self._check(self._lib.ev_style_load_weights(self._h, C.byref(bc), C.cast(buf, C.c_void_p), len(blob)))
        self.style_hidden = int(bc.hidden)

    def style_embed(self, id_lists: Sequence[np.ndarray], type_lists: Optional[Sequence[np.ndarray]] = None) -> np.ndarray:
        """pooled_output (B, hidden) of B token-id sequences (one text each: [CLS] ... [SEP])."""
        B = len(id_lists)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in id_lists]))
        cu = np.zeros(B + 1, np.int32)
        cu[1:] = np.cumsum([len(x) for x in id_lists])
        tt = None
        if type_lists is not None:
            tt = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in type_lists]))
        out = np.empty((B, self.style_hidden), np.float32)
        self._check(self._lib.ev_style_embed(self._h, B, ids.ctypes.data_as(C.c_void_p), tt.ctypes.data_as(C.c_void_p) if tt is not None else None,
                                             cu.ctypes.data_as(C.c_void_p), 0, out.ctypes.data_as(C.c_void_p)))
        return out

    # -- raw calls (host or device pointers)
    def synthesize_raw(self, B: int, ling_ptr: int, cu_seqlens: np.ndarray, speaker_ptr: int, style_ptr: int,
                       content_ptr: int, alpha: float = 1.0, flags: int = 0) -> _ffi.ev_result:
        cu = np.ascontiguousarray(cu_seqlens, np.int32)
        res = _ffi.ev_result()
        self._check(self._lib.ev_synthesize(self._h, B, C.c_void_p(ling_ptr), cu.ctypes.data_as(C.c_void_p),
                                            C.c_void_p(speaker_ptr), C.c_void_p(style_ptr), C.c_void_p(content_ptr),
                                            C.c_float(alpha), flags, C.byref(res)))
        self.last = res
        return res

    def synthesize_prosody_raw(self, B: int, ling_ptr: int, cu_seqlens: np.ndarray, speaker_ptr: int, style_ptr: int,
                               content_ptr: int, alpha: float = 1.0, prosody=None, flags: int = 0) -> _ffi.ev_result:
        """ev_synthesize_prosody.  ``prosody``: a PackedProsody (emotivoice_amd.prosody.pack_prosody, packed with device=True when
        ``flags`` has EV_FLAG_DEVICE_INPUTS) or None (= ev_synthesize)."""
        if prosody is not None and prosody.device != bool(flags & _ffi.EV_FLAG_DEVICE_INPUTS):
            raise ValueError("the prosody arrays were packed for %s inputs, the call passes %s inputs"
                             % ("device" if prosody.device else "host", "device" if flags & _ffi.EV_FLAG_DEVICE_INPUTS else "host"))
        cu = np.ascontiguousarray(cu_seqlens, np.int32)
        res = _ffi.ev_result()
        self._check(self._lib.ev_synthesize_prosody(self._h, B, C.c_void_p(ling_ptr), cu.ctypes.data_as(C.c_void_p),
                                                    C.c_void_p(speaker_ptr), C.c_void_p(style_ptr), C.c_void_p(content_ptr),
                                                    C.c_float(alpha), C.byref(prosody.struct) if prosody is not None else None,
                                                    flags, C.byref(res)))
        self.last = res
        return res

    def vocoder_raw(self, B: int, mel_ptr: int, mel_is_f16: bool, mel_lens: np.ndarray, flags: int = 0) -> _ffi.ev_result:
        ml = np.ascontiguousarray(mel_lens, np.int32)
        res = _ffi.ev_result()
        self._check(self._lib.ev_vocoder(self._h, B, C.c_void_p(mel_ptr), 1 if mel_is_f16 else 0,
                                         ml.ctypes.data_as(C.c_void_p), flags, C.byref(res)))
        self.last = res
        return res

    def align_raw(self, B: int, ling_ptr: int, cu_seqlens: np.ndarray, speaker_ptr: int, style_ptr: int, content_ptr: int, mel_ptr: int,
                  mel_is_f16: bool, mel_lens: np.ndarray, pitch_ptr: Optional[int] = None, energy_ptr: Optional[int] = None,
                  flags: int = 0) -> _ffi.ev_align_result:
        """ev_align (include/evhip.h).  The returned struct's device arrays stay valid until the next align on this engine.  flags:
        EV_FLAG_DEVICE_INPUTS (every pointer on the device) or EV_FLAG_DEVICE_MEL (mel / pitch / energy frames only: a features_raw result)."""
        cu = np.ascontiguousarray(cu_seqlens, np.int32)
        ml = np.ascontiguousarray(mel_lens, np.int32)
        res = _ffi.ev_align_result()
        res.struct_size = C.sizeof(_ffi.ev_align_result)
        self._check(self._lib.ev_align(self._h, B, C.c_void_p(ling_ptr), cu.ctypes.data_as(C.c_void_p), C.c_void_p(speaker_ptr),
                                       C.c_void_p(style_ptr), C.c_void_p(content_ptr), C.c_void_p(mel_ptr), 1 if mel_is_f16 else 0,
                                       ml.ctypes.data_as(C.c_void_p), C.c_void_p(pitch_ptr) if pitch_ptr else None,
                                       C.c_void_p(energy_ptr) if energy_ptr else None, flags, C.byref(res)))
        self.last_align = res
        return res

    def align_to_numpy(self, res: _ffi.ev_align_result) -> Dict[str, object]:
        B, NT = res.batch, res.total_tokens
        mel_lens = np.array([res.mel_lens[b] for b in range(B)], np.int32)
        out: Dict[str, object] = dict(mel_lens=mel_lens, mel_offsets=np.array([res.mel_offsets[b] for b in range(B + 1)], np.int64),
                                      durations=self.d2h(res.durations, (NT,), np.int64), score=self.d2h(res.score, (B,), np.float32))
        out["pitch"] = self.d2h(res.pitch, (NT,), np.float32) if res.pitch else None
        out["energy"] = self.d2h(res.energy, (NT,), np.float32) if res.energy else None
        return out

    def align(self, utts: Sequence[dict], mels: Sequence[np.ndarray], pitch: Optional[Sequence[np.ndarray]] = None,
              energy: Optional[Sequence[np.ndarray]] = None) -> Dict[str, object]:
        """Forced alignment of recordings of known text (ev_align).  utts: as synthesize(); mels: one (n_mels, T_b) array per utterance, fp32
        or fp16 (the vocoder() convention); pitch / energy: optional per-frame tracks, one (T_b,) array per utterance, in the checkpoint's
        normalised units.  Returns durations (packed (total_tokens,) int64) and durations_list, pitch / energy (per-token means, packed, or
        None), score (B,) = mean log_p_attn along the path, mel_lens, cu_seqlens."""
        B = len(utts)
        if len(mels) != B:
            raise ValueError("%d mels for %d utterances" % (len(mels), B))
        ling = np.ascontiguousarray(np.concatenate([np.asarray(u["ling"], np.int64) for u in utts]))
        cu = np.zeros(B + 1, np.int32)
        cu[1:] = np.cumsum([len(u["ling"]) for u in utts])
        spk = np.ascontiguousarray([int(u["speaker"]) for u in utts], np.int64)
        style = np.ascontiguousarray(np.stack([np.asarray(u["style"], np.float32) for u in utts]))
        content = np.ascontiguousarray(np.stack([np.asarray(u["content"], np.float32) for u in utts]))
        is16 = np.asarray(mels[0]).dtype == np.float16
        mdt = np.float16 if is16 else np.float32
        for b, m in enumerate(mels):
            if np.asarray(m).ndim != 2 or np.asarray(m).shape[0] != self.shapes.n_mels:
                raise ValueError("mels[%d]: expected (%d, T), got %s" % (b, self.shapes.n_mels, np.asarray(m).shape))
        flat = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(m, mdt).ravel() for m in mels]))
        lens = np.array([np.asarray(m).shape[1] for m in mels], np.int32)

        def track(xs, name):
            if xs is None:
                return None
            if len(xs) != B:
                raise ValueError("%d %s tracks for %d utterances" % (len(xs), name, B))
            for b, x in enumerate(xs):
                if np.asarray(x).reshape(-1).size != lens[b]:
                    raise ValueError("%s[%d]: expected %d frames, got %d" % (name, b, lens[b], np.asarray(x).size))
            return np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in xs]))

        pf, ef = track(pitch, "pitch"), track(energy, "energy")
        res = self.align_raw(B, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data, flat.ctypes.data, is16, lens,
                             pf.ctypes.data if pf is not None else None, ef.ctypes.data if ef is not None else None)
        out = self.align_to_numpy(res)
        out["cu_seqlens"] = cu
        out["durations_list"] = [out["durations"][cu[b]:cu[b + 1]] for b in range(B)]
        return out

    # -- acoustic features (ev_features): wav -> mel, energy on the device
    def features_setup(self, config=None):
        """ev_features_setup.  config: an emotivoice_amd.features.FeatureConfig (default: the reference's values).  Needs no weights."""
        from .features import FeatureConfig
        fc = (config or FeatureConfig()).validate()
        mb, win = fc.tables()
        c = _ffi.ev_features_config()
        self._lib.ev_default_features_config(C.byref(c))
        c.n_fft, c.hop, c.n_mels, c.mel_clip, c.energy_floor = fc.n_fft, fc.hop, fc.n_mels, fc.mel_clip, fc.energy_floor
        c.mel_basis = mb.ctypes.data
        c.window = win.ctypes.data if win is not None else None
        self._check(self._lib.ev_features_setup(self._h, C.byref(c)))
        self.feature_config = fc

    def features_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, wav_lens: np.ndarray, energy_mean: float = 0.0, energy_std: float = 1.0,
                     flags: int = 0) -> _ffi.ev_features_result:
        """ev_features (include/evhip.h).  The returned struct's device arrays stay valid until the next features call on this engine."""
        wl = np.ascontiguousarray(wav_lens, np.int64)
        res = _ffi.ev_features_result()
        res.struct_size = C.sizeof(_ffi.ev_features_result)
        self._check(self._lib.ev_features(self._h, B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, wl.ctypes.data_as(C.c_void_p),
                                          C.c_float(energy_mean), C.c_float(energy_std), flags, C.byref(res)))
        self.last_features = res
        return res

    def features_to_numpy(self, res: _ffi.ev_features_result) -> Dict[str, object]:
        B, n_mels = res.batch, self.feature_config.n_mels
        mel_lens = np.array([res.mel_lens[b] for b in range(B)], np.int32)
        offs = np.array([res.mel_offsets[b] for b in range(B + 1)], np.int64)
        mel = self.d2h(res.mel, (res.total_frames * n_mels,), np.float32)
        energy = self.d2h(res.energy, (res.total_frames,), np.float32)
        return dict(mel_lens=mel_lens, mel_offsets=offs, energy=energy,
                    mel_list=[mel[offs[b] * n_mels:offs[b + 1] * n_mels].reshape(n_mels, mel_lens[b]) for b in range(B)],
                    energy_list=[energy[offs[b]:offs[b + 1]] for b in range(B)])

    def features(self, wavs: Sequence[np.ndarray], energy_stats=(0.0, 1.0)) -> Dict[str, object]:
        """Mel spectrogram and frame energy of recordings (ev_features).  wavs: one 1-D array per utterance, all int16 or all floating in
        [-1, 1]; energy_stats: (mean, std) the energy is standardised with (the corpus statistics of the checkpoint; (0, 1) = raw).
        Returns mel_list ((n_mels, T_b) each: what align() / vocoder() take), energy_list ((T_b,) each) and mel_lens."""
        if self.feature_config is None:
            self.features_setup()
        from .features import pack_wavs
        fc = self.feature_config
        flat, is16, lens = pack_wavs(wavs, fc.n_fft, fc.hop)
        mean, std = float(energy_stats[0]), float(energy_stats[1])
        if not (np.isfinite(mean) and np.isfinite(std) and std > 0):
            raise ValueError("energy_stats: mean must be finite and std positive and finite")
        return self.features_to_numpy(self.features_raw(len(wavs), flat.ctypes.data, is16, lens, mean, std))

    # -- pitch extraction (ev_pitch): wav -> F0 track on the device
    def pitch_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, wav_lens: np.ndarray, pitch_mean: float = 0.0, pitch_std: float = 1.0,
                  config=None, flags: int = 0) -> _ffi.ev_pitch_result:
        """ev_pitch (include/evhip.h).  config: an emotivoice_amd.pitch.PitchConfig or None (= ev_default_pitch_config).  The returned struct's
        device arrays stay valid until the next pitch call on this engine."""
        wl = np.ascontiguousarray(wav_lens, np.int64)
        c = None
        if config is not None:
            c = _ffi.ev_pitch_config()
            self._lib.ev_default_pitch_config(C.byref(c))
            c.sample_rate, c.hop, c.win = int(config.sample_rate), int(config.hop), int(config.win)
            c.f_min, c.f_max, c.threshold, c.silence_rms = config.f_min, config.f_max, config.threshold, config.silence_rms
        res = _ffi.ev_pitch_result()
        res.struct_size = C.sizeof(_ffi.ev_pitch_result)
        self._check(self._lib.ev_pitch(self._h, B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, wl.ctypes.data_as(C.c_void_p),
                                       C.byref(c) if c is not None else None, C.c_float(pitch_mean), C.c_float(pitch_std), flags, C.byref(res)))
        self.last_pitch = res
        return res

    def pitch_to_numpy(self, res: _ffi.ev_pitch_result) -> Dict[str, object]:
        B, n = res.batch, res.total_frames
        mel_lens = np.array([res.mel_lens[b] for b in range(B)], np.int32)
        offs = np.array([res.mel_offsets[b] for b in range(B + 1)], np.int64)
        pitch, f0, ap = (self.d2h(ptr, (n,), np.float32) for ptr in (res.pitch, res.f0_hz, res.aperiodicity))
        cut = lambda x: [x[offs[b]:offs[b + 1]] for b in range(B)]      # noqa: E731
        return dict(mel_lens=mel_lens, mel_offsets=offs, pitch=pitch, pitch_list=cut(pitch), f0_list=cut(f0), aperiodicity_list=cut(ap))

    def pitch(self, wavs: Sequence[np.ndarray], pitch_stats=(0.0, 1.0), config=None) -> Dict[str, object]:
        """F0 track of recordings (ev_pitch: YIN on ev_features' frame grid -- not the reference's dio + stonemask).  wavs: one 1-D array per
        utterance, all int16 or all floating in [-1, 1]; pitch_stats: (mean, std) in Hz the continuous track is standardised with (the
        checkpoint's corpus statistics; (0, 1) = Hz).  Returns pitch_list ((T_b,) each: what align() takes as pitch), f0_list (Hz, 0 =
        unvoiced), aperiodicity_list and mel_lens."""
        from .pitch import PitchConfig, check_stats, pack_wavs
        pc = (config or PitchConfig()).validate()
        mean, std = check_stats(pitch_stats)
        flat, is16, lens = pack_wavs(wavs, pc.hop)
        return self.pitch_to_numpy(self.pitch_raw(len(wavs), flat.ctypes.data, is16, lens, mean, std, pc))

    # -- sample-rate conversion and trimming (ev_resample): wav at any common rate -> wav at the model's rate on the device
    def resample_setup(self, config):
        """ev_resample_setup.  config: an emotivoice_amd.resample.ResampleConfig.  The default design is built by the library; other design
        parameters, or the caller's own taps, go in as taps.  Needs no weights."""
        rc = config.validate()
        c = _ffi.ev_resample_config()
        self._lib.ev_default_resample_config(C.byref(c))
        c.sr_in, c.sr_out = int(rc.sr_in), int(rc.sr_out)
        taps = None
        if not rc.is_default_design():
            taps = np.ascontiguousarray(rc.design(), np.float32)
            c.taps, c.half_len = taps.ctypes.data, (taps.size - 1) // 2
        if rc.trim:
            c.trim_frac, c.trim_pad = rc.trim_frac, rc.pad()
        self._check(self._lib.ev_resample_setup(self._h, C.byref(c)))
        self.resample_config = rc

    def resample_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, wav_lens: np.ndarray, flags: int = 0) -> _ffi.ev_resample_result:
        """ev_resample (include/evhip.h).  The returned struct's device waveform stays valid until the next resample call on this engine."""
        wl = np.ascontiguousarray(wav_lens, np.int64)
        res = _ffi.ev_resample_result()
        res.struct_size = C.sizeof(_ffi.ev_resample_result)
        self._check(self._lib.ev_resample(self._h, B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, wl.ctypes.data_as(C.c_void_p), flags, C.byref(res)))
        self.last_resample = res
        return res

    def resample_to_numpy(self, res: _ffi.ev_resample_result) -> Dict[str, object]:
        B = res.batch
        lens = np.array([res.wav_lens[b] for b in range(B)], np.int64)
        offs = np.array([res.wav_offsets[b] for b in range(B + 1)], np.int64)
        wav = self.d2h(res.wav, (res.total_samples,), np.float32)
        return dict(wav=wav, wav_list=[wav[offs[b]:offs[b + 1]] for b in range(B)], wav_lens=lens, wav_offsets=offs,
                    trim_start=np.array([res.trim_start[b] for b in range(B)], np.int64),
                    trim_end=np.array([res.trim_end[b] for b in range(B)], np.int64))

    def resample(self, wavs: Sequence[np.ndarray], sr_in: int, **config) -> Dict[str, object]:
        """Recordings at ``sr_in`` -> waveforms at ``sr_out`` (default 16 kHz), optionally trimmed and padded as the reference's get_mel does
        (``trim=True``).  wavs: one 1-D array per utterance, all int16 or all floating; further keywords: the fields of
        emotivoice_amd.resample.ResampleConfig.  The filter is this project's polyphase windowed sinc, not librosa's soxr.  Returns wav_list
        (float32), wav_lens, trim_start and trim_end (indices into the untrimmed resampled utterance)."""
        from .resample import ResampleConfig, pack_wavs
        rc = ResampleConfig(sr_in=sr_in, **config).validate()
        if self.resample_config is None or self.resample_config.key() != rc.key():
            self.resample_setup(rc)
        flat, is16, lens = pack_wavs(wavs, rc)
        return self.resample_to_numpy(self.resample_raw(len(wavs), flat.ctypes.data, is16, lens))

    # -- long-form stitching (ev_stitch): the sentences of one batch -> finished documents on the device
    def stitch_raw(self, S: int, wav_ptr: int, seg_offsets: np.ndarray, seg_lens: np.ndarray, seg_doc: np.ndarray, pause_after: np.ndarray,
                   config=None, flags: int = 0) -> _ffi.ev_stitch_result:
        """ev_stitch (include/evhip.h).  config: an emotivoice_amd.longform.StitchConfig, an _ffi.ev_stitch_config or None (the library's default:
        plain concatenation).  wav_ptr is a device pointer with EV_FLAG_DEVICE_INPUTS; the four arrays are host arrays.  The returned struct's
        device documents stay valid until the next stitch call on this engine."""
        so, sl = np.ascontiguousarray(seg_offsets, np.int64), np.ascontiguousarray(seg_lens, np.int64)
        sd, pa = np.ascontiguousarray(seg_doc, np.int32), np.ascontiguousarray(pause_after, np.int32)
        if not (so.size == sl.size == sd.size == pa.size == S):
            raise ValueError("seg_offsets / seg_lens / seg_doc / pause_after must have S = %d entries each" % S)
        c = config.to_struct() if hasattr(config, "to_struct") else config
        res = _ffi.ev_stitch_result()
        res.struct_size = C.sizeof(_ffi.ev_stitch_result)
        self._check(self._lib.ev_stitch(self._h, S, C.c_void_p(wav_ptr), so.ctypes.data_as(C.c_void_p), sl.ctypes.data_as(C.c_void_p),
                                        sd.ctypes.data_as(C.c_void_p), pa.ctypes.data_as(C.c_void_p), C.byref(c) if c is not None else None, flags,
                                        C.byref(res)))
        self.last_stitch = res
        return res

    def stitch_to_numpy(self, res: _ffi.ev_stitch_result, int16_only: bool = False, skip_wav: bool = False) -> Dict[str, object]:
        """One D2H copy of the fp32 documents (or, with ``int16_only`` and a result that has them, of the int16 ones only; without it both) and
        the host arrays of the result.  ``skip_wav``: the host arrays only."""
        D, S = res.batch_docs, res.batch_segs
        lens = np.array([res.doc_lens[d] for d in range(D)], np.int64)
        offs = np.array([res.doc_offsets[d] for d in range(D + 1)], np.int64)
        out: Dict[str, object] = dict(doc_lens=lens, doc_offsets=offs,
                                      seg_pos=np.array([res.seg_pos[s] for s in range(S)], np.int64),
                                      seg_start=np.array([res.seg_start[s] for s in range(S)], np.int64),
                                      seg_end=np.array([res.seg_end[s] for s in range(S)], np.int64),
                                      seg_peak=np.array([res.seg_peak[s] for s in range(S)], np.float32))
        if skip_wav:
            return out
        if not (int16_only and res.wav_i16):
            out["wav"] = self.d2h(res.wav, (res.total_samples,), np.float32)
            out["docs"] = [out["wav"][offs[d]:offs[d + 1]] for d in range(D)]
        if res.wav_i16:
            out["wav_i16"] = self.d2h(res.wav_i16, (res.total_samples,), np.int16)
            out["docs_i16"] = [out["wav_i16"][offs[d]:offs[d + 1]] for d in range(D)]
        return out

    def stitch(self, wavs: Sequence[np.ndarray], docs: Sequence[int], pauses: Sequence, **config) -> Dict[str, object]:
        """Host waveforms -> documents.  wavs: one 1-D float array per segment; docs: the document of every segment (non-decreasing from 0);
        pauses: one entry per segment, the pause after it as a class of emotivoice_amd.longform.pauses_ms, milliseconds (negative: a
        cross-fade) or None; further keywords: the fields of emotivoice_amd.longform.StitchConfig.  Needs no weights."""
        from .longform import StitchConfig, plan_document
        sc = StitchConfig(**config).validate()
        seg_doc, pause_after = plan_document(docs, pauses, sc.sample_rate)
        lens = np.array([np.asarray(w).size for w in wavs], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in wavs]))
        return self.stitch_to_numpy(self.stitch_raw(len(wavs), flat.ctypes.data, offs, lens, seg_doc, pause_after, sc))

    def synthesize_long(self, documents: Sequence, alpha: float = 1.0, prosody=None, config=None, flac=None, loudness=None, limiter=None) -> Dict[str, object]:
        """Documents of several sentences each -> one waveform per document and the time of every sentence in it.  documents: each a
        dict(utts=[utt dicts as ``synthesize`` takes], pauses=[one per joint: a class of emotivoice_amd.longform.pauses_ms, milliseconds, or
        None]) or a pair (utts, pauses); pauses None = "sentence" everywhere.  prosody: as ``synthesize`` takes it, over the sentences of all
        documents in order.  config: an emotivoice_amd.longform.StitchConfig (None: its defaults, which have not been measured on a released
        checkpoint).  One ev_synthesize[_prosody] call, one ev_stitch call on its device waveform and one D2H copy (int16 with
        config.want_int16, else fp32).  All sentences go into one synthesize call: more than it takes raises; splitting is the caller's.
        flac=True adds flac_list, one FLAC stream (``bytes``) per document, encoded on the device from ev_stitch's int16 documents (it turns
        config.want_int16 on, so ``documents`` are the int16 ones a stream decodes to).
        loudness: None, a target in LUFS or an emotivoice_amd.loudness.LoudnessConfig: every document is normalised on the device after ev_stitch
        (ev_loudness: one gain per document, so the balance between its sentences stays) and before ev_flac; ``documents`` (int16 by the
        clamping rule with config.want_int16) then hold the normalised audio and ``loudness`` the per-document figures.
        limiter: as ``synthesize`` takes it, per document: ev_limit after ev_stitch (and after ev_loudness's measurement when ``loudness`` is
        given, whose pre-gain it applies) and before ev_flac; ``documents`` hold the limited audio and ``limiter`` the per-document figures."""
        import dataclasses
        from .longform import StitchConfig, flatten_documents, plan_document
        sc = (config or StitchConfig()).validate()
        if flac and not sc.want_int16:
            sc = dataclasses.replace(sc, want_int16=True).validate()
        if int(sc.sample_rate) != int(self.shapes.sr):
            raise ValueError("config.sample_rate %d is not the engine's %d" % (sc.sample_rate, self.shapes.sr))
        utts, seg_doc, pauses = flatten_documents(documents)
        S = len(utts)
        if S > 65535:
            raise ValueError("%d sentences exceed the 65535 segments of one ev_stitch call; split the documents over several calls" % S)
        seg_doc, pause_after = plan_document(seg_doc, pauses, sc.sample_rate)
        res, _ = self._synthesize_call(utts, alpha, 0, None, prosody)
        up = self.shapes.upsample_factor
        mel_offs = np.array([res.mel_offsets[b] for b in range(S + 1)], np.int64)
        st = self.stitch_raw(S, res.wav, mel_offs[:-1] * up, np.diff(mel_offs) * up, seg_doc, pause_after, sc, _ffi.EV_FLAG_DEVICE_INPUTS)
        out = self.stitch_to_numpy(st, int16_only=sc.want_int16, skip_wav=loudness is not None or limiter is not None)
        empty = [d for d in range(st.batch_docs) if out["doc_lens"][d] < 1]
        pcm_i16 = st.wav_i16
        if limiter is not None:
            if empty:
                raise ValueError("limiter: document %d is empty after the cut" % empty[0])
            lm, lim, meas = self._measure_and_limit(st.batch_docs, st.wav, out["doc_lens"], loudness, limiter, int(sc.sample_rate), sc.want_int16,
                                                    int16_only=sc.want_int16)
            if "wav" in lim:
                out["wav"], out["docs"] = lim.pop("wav"), lim.pop("wav_list")
            if "wav_i16" in lim:
                out["wav_i16"], out["docs_i16"] = lim.pop("wav_i16"), lim.pop("wav_i16_list")
            if meas is not None:
                out["loudness"] = meas
            out["limiter"] = lim
            pcm_i16 = lm.wav_i16
        elif loudness is not None:
            from .loudness import as_config
            if empty:
                raise ValueError("loudness: document %d is empty after the cut" % empty[0])
            ld = self.loudness_raw(st.batch_docs, st.wav, False, out["doc_lens"], as_config(loudness, int(sc.sample_rate), sc.want_int16),
                                   _ffi.EV_FLAG_DEVICE_INPUTS)
            norm = self.loudness_to_numpy(ld, int16_only=sc.want_int16)
            if "wav" in norm:
                out["wav"], out["docs"] = norm.pop("wav"), norm.pop("wav_list")
            if "wav_i16" in norm:
                out["wav_i16"], out["docs_i16"] = norm.pop("wav_i16"), norm.pop("wav_i16_list")
            out["loudness"] = norm
            pcm_i16 = ld.wav_i16
        if flac:
            from .flac import FlacConfig
            if empty:
                raise ValueError("flac: document %d is empty after the cut" % empty[0])
            fr = self.flac_raw(st.batch_docs, pcm_i16, True, out["doc_lens"], FlacConfig(sample_rate=int(sc.sample_rate)), _ffi.EV_FLAG_DEVICE_INPUTS)
            out["flac_list"] = self.flac_to_numpy(fr)["streams"]
        sr = float(sc.sample_rate)
        start = out["seg_pos"] / sr
        end = (out["seg_pos"] + (out["seg_end"] - out["seg_start"])) / sr
        out["documents"] = out["docs_i16"] if sc.want_int16 else out["docs"]
        out["seg_doc"] = seg_doc
        out["sentence_times"] = [[(float(start[s]), float(end[s])) for s in np.nonzero(seg_doc == d)[0]] for d in range(st.batch_docs)]
        out["sample_rate"] = int(sc.sample_rate)
        return out

    # -- signal comparison (ev_compare): how far a signal lies from a yardstick, per segment, on the device
    def compare_raw(self, B: int, a_ptr: int, b_ptr: int, lens: np.ndarray, flags: int = 0) -> _ffi.ev_compare_result:
        """ev_compare (include/evhip.h).  a_ptr (under test) and b_ptr (the yardstick) are host pointers, or device pointers with
        EV_FLAG_DEVICE_INPUTS -- of this engine or of another one on the same device; lens is a host array.  The returned struct's arrays
        are host memory and stay valid until the next compare call on this engine."""
        ln = np.ascontiguousarray(lens, np.int64)
        if ln.size != B:
            raise ValueError("lens must have B = %d entries" % B)
        res = _ffi.ev_compare_result()
        res.struct_size = C.sizeof(_ffi.ev_compare_result)
        self._check(self._lib.ev_compare(self._h, B, C.c_void_p(a_ptr), C.c_void_p(b_ptr), ln.ctypes.data_as(C.c_void_p), flags, C.byref(res)))
        self.last_compare = res
        return res

    def compare_to_numpy(self, res: _ffi.ev_compare_result) -> Dict[str, object]:
        """Copies of the result's host arrays (they outlive the next compare call)."""
        B = res.batch
        out: Dict[str, object] = dict(batch=B, total=int(res.total))
        for k, dt in (("sum_d", np.float64), ("sum_d2", np.float64), ("sum_y", np.float64), ("sum_y2", np.float64), ("rel_l2", np.float64),
                      ("rel_l2_ac", np.float64), ("max_abs_d", np.float32), ("argmax_d", np.int64), ("peak_y", np.float32), ("nonfinite", np.int64)):
            out[k] = np.ctypeslib.as_array(getattr(res, k), (B,)).astype(dt, copy=True)
        offs = np.ctypeslib.as_array(res.chunk_offsets, (B + 1,)).astype(np.int64, copy=True)
        out["chunk_offsets"] = offs
        out["chunk_d2"] = np.ctypeslib.as_array(res.chunk_d2, (int(offs[-1]),)).astype(np.float64, copy=True)
        out["chunk_y2"] = np.ctypeslib.as_array(res.chunk_y2, (int(offs[-1]),)).astype(np.float64, copy=True)
        return out

    def compare(self, a_list: Sequence[np.ndarray], b_list: Sequence[np.ndarray]) -> Dict[str, object]:
        """Host signals: a_list (under test) against b_list (the yardstick), one array per segment, equal sizes pairwise (any shape: a mel is
        compared flattened).  Returns per-segment numpy arrays: sum_d, sum_d2, sum_y, sum_y2, rel_l2, rel_l2_ac (the mean of the yardstick
        removed), max_abs_d, argmax_d, peak_y, nonfinite, and chunk_d2 / chunk_y2 / chunk_offsets (the sums of every 4096-element chunk).
        Needs no weights."""
        if len(a_list) != len(b_list) or not len(a_list):
            raise ValueError("a_list and b_list must hold the same number (>= 1) of segments")
        lens = np.array([np.asarray(x).size for x in a_list], np.int64)
        for s, y in enumerate(b_list):
            if np.asarray(y).size != lens[s]:
                raise ValueError("segment %d: a has %d elements, b has %d" % (s, lens[s], np.asarray(y).size))
        fa = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in a_list]))
        fb = np.ascontiguousarray(np.concatenate([np.asarray(y, np.float32).reshape(-1) for y in b_list]))
        return self.compare_to_numpy(self.compare_raw(len(a_list), fa.ctypes.data, fb.ctypes.data, lens))

    # -- FLAC encoding (ev_flac): packed PCM -> one FLAC stream per segment, on the device
    def flac_raw(self, B: int, pcm_ptr: int, pcm_is_i16: bool, lens: np.ndarray, config=None, flags: int = 0) -> _ffi.ev_flac_result:
        """ev_flac (include/evhip.h).  pcm_ptr is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS; lens is a host array.  config:
        an emotivoice_amd.flac.FlacConfig, an _ffi.ev_flac_config or None (the library's default).  The returned struct's device bytes and host
        arrays stay valid until the next flac call on this engine."""
        ln = np.ascontiguousarray(lens, np.int64)
        if ln.size != B:
            raise ValueError("lens must have B = %d entries" % B)
        c = config.validate().to_struct() if hasattr(config, "to_struct") else config
        res = _ffi.ev_flac_result()
        res.struct_size = C.sizeof(_ffi.ev_flac_result)
        self._check(self._lib.ev_flac(self._h, B, C.c_void_p(pcm_ptr), 1 if pcm_is_i16 else 0, ln.ctypes.data_as(C.c_void_p),
                                      C.byref(c) if c is not None else None, flags, C.byref(res)))
        self.last_flac = res
        return res

    def flac_to_numpy(self, res: _ffi.ev_flac_result) -> Dict[str, object]:
        """One D2H copy of total_bytes and copies of the result's host arrays.  streams: one ``bytes`` per segment; frame_kind / frame_porder:
        one uint8 array per segment (0 constant, 1 verbatim, 8 + o fixed; the partition order)."""
        B, NF = res.batch, int(res.total_frames)
        raw = self.d2h(res.bytes, (int(res.total_bytes),), np.uint8)
        offs = np.ctypeslib.as_array(res.stream_offsets, (B + 1,)).astype(np.int64, copy=True)
        nfr = np.ctypeslib.as_array(res.stream_frames, (B,)).astype(np.int64, copy=True)
        kind = np.ctypeslib.as_array(res.frame_kind, (NF,)).astype(np.uint8, copy=True)
        porder = np.ctypeslib.as_array(res.frame_porder, (NF,)).astype(np.uint8, copy=True)
        f0 = np.concatenate([[0], np.cumsum(nfr)]).astype(np.int64)
        return dict(streams=[raw[offs[b]:offs[b + 1]].tobytes() for b in range(B)], stream_offsets=offs, stream_frames=nfr,
                    frame_offsets=np.ctypeslib.as_array(res.frame_offsets, (NF + 1,)).astype(np.int64, copy=True),
                    frame_kind=[kind[f0[b]:f0[b + 1]] for b in range(B)], frame_porder=[porder[f0[b]:f0[b + 1]] for b in range(B)],
                    total_bytes=int(res.total_bytes))

    def flac(self, pcm_list: Sequence[np.ndarray], **config) -> Dict[str, object]:
        """Host signals -> FLAC streams.  pcm_list: one 1-D array per segment, all int16 or all floating (converted on the device with
        config's ``convert`` rule); further keywords: the fields of emotivoice_amd.flac.FlacConfig.  Needs no weights."""
        from .flac import FlacConfig
        fc = FlacConfig(**config).validate()
        if not len(pcm_list):
            raise ValueError("pcm_list must hold at least one segment")
        arrs = [np.asarray(x) for x in pcm_list]
        is16 = arrs[0].dtype == np.int16
        for s, a in enumerate(arrs):
            if a.ndim != 1 or (a.dtype == np.int16) != is16 or not (is16 or np.issubdtype(a.dtype, np.floating)):
                raise ValueError("segment %d: 1-D arrays, all int16 or all floating" % s)
        flat = np.ascontiguousarray(np.concatenate([a.astype(np.int16 if is16 else np.float32, copy=False) for a in arrs]))
        lens = np.array([a.size for a in arrs], np.int64)
        return self.flac_to_numpy(self.flac_raw(len(arrs), flat.ctypes.data, is16, lens, fc))

    def _flac_of_result(self, res: _ffi.ev_result, mask, pcm_i16: Optional[int] = None) -> List[Optional[bytes]]:
        """The utterances of an ev_result that ``mask`` selects, encoded from the fp32 device waveform with the wrapping conversion: one ev_flac
        call per run of consecutive selected utterances (ev_flac takes its segments back to back).  ``pcm_i16``: a device int16 waveform in
        the same packing (ev_loudness's) to encode instead."""
        from .flac import FlacConfig
        B, up = res.batch, self.shapes.upsample_factor
        sel = np.ones(B, bool) if mask is True else np.asarray(mask, bool)
        if sel.shape != (B,):
            raise ValueError("flac: True or one entry per utterance (%d), got shape %s" % (B, sel.shape))
        if sel.any() and not (res.wav or pcm_i16):
            raise ValueError("flac needs the vocoder's waveform")
        fc = FlacConfig(sample_rate=int(self.shapes.sr), convert="wrap")
        mel_offs = np.array([res.mel_offsets[b] for b in range(B + 1)], np.int64)
        out: List[Optional[bytes]] = [None] * B
        b = 0
        while b < B:
            if not sel[b]:
                b += 1
                continue
            e = b
            while e < B and sel[e]:
                e += 1
            src = pcm_i16 + 2 * int(mel_offs[b]) * up if pcm_i16 else res.wav + 4 * int(mel_offs[b]) * up
            fr = self.flac_raw(e - b, src, bool(pcm_i16), np.diff(mel_offs[b:e + 1]) * up, fc, _ffi.EV_FLAG_DEVICE_INPUTS)
            out[b:e] = self.flac_to_numpy(fr)["streams"]
            b = e
        return out

    # -- loudness normalisation (ev_loudness): BS.1770 programme loudness, one gain per segment and the scaled waveform, on the device
    def loudness_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, lens: np.ndarray, config=None, flags: int = 0) -> _ffi.ev_loudness_result:
        """ev_loudness (include/evhip.h).  wav_ptr is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS; lens is a host array.
        config: an emotivoice_amd.loudness.LoudnessConfig, an _ffi.ev_loudness_config or None (the library's default: 16 kHz, measure only).
        The returned struct's device waveforms and host arrays stay valid until the next loudness call on this engine."""
        ln = np.ascontiguousarray(lens, np.int64)
        if ln.size != B:
            raise ValueError("lens must have B = %d entries" % B)
        c = config.validate().to_struct() if hasattr(config, "to_struct") else config
        res = _ffi.ev_loudness_result()
        res.struct_size = C.sizeof(_ffi.ev_loudness_result)
        self._check(self._lib.ev_loudness(self._h, B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, ln.ctypes.data_as(C.c_void_p),
                                          C.byref(c) if c is not None else None, flags, C.byref(res)))
        res._lens = ln.copy()      # the packing of res.wav / res.wav_i16, for loudness_to_numpy
        self.last_loudness = res
        return res

    def loudness_to_numpy(self, res: _ffi.ev_loudness_result, int16_only: bool = False, lens=None) -> Dict[str, object]:
        """Copies of the result's host arrays and, unless the call only measured, one D2H copy of the fp32 output (with ``int16_only`` and a
        result that has it, of the int16 output only; without it both).  block_ms / block_state: one array per segment.  lens: the call's
        lens, which cut the output into wav_list / wav_i16_list (None: the ones loudness_raw kept with the struct)."""
        B = res.batch
        arr = lambda p, n, dt: np.ctypeslib.as_array(p, (n,)).astype(dt, copy=True)      # noqa: E731
        boffs = arr(res.block_offsets, B + 1, np.int64)
        nb = int(boffs[-1])
        ms, state = arr(res.block_ms, nb, np.float64), arr(res.block_state, nb, np.uint8)
        out: Dict[str, object] = dict(loudness=arr(res.loudness, B, np.float64), rel_threshold=arr(res.rel_threshold, B, np.float64),
                                      gain=arr(res.gain, B, np.float32), peak=arr(res.peak, B, np.float32), flags=arr(res.flags, B, np.uint8),
                                      nonfinite=arr(res.nonfinite, B, np.int64), block_offsets=boffs,
                                      block_ms=[ms[boffs[b]:boffs[b + 1]] for b in range(B)], block_state=[state[boffs[b]:boffs[b + 1]] for b in range(B)])
        if not res.wav:
            return out
        lens = np.asarray(res._lens if lens is None else lens, np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        if not (int16_only and res.wav_i16):
            out["wav"] = self.d2h(res.wav, (int(res.total),), np.float32)
            out["wav_list"] = [out["wav"][offs[b]:offs[b + 1]] for b in range(B)]
        if res.wav_i16:
            out["wav_i16"] = self.d2h(res.wav_i16, (int(res.total),), np.int16)
            out["wav_i16_list"] = [out["wav_i16"][offs[b]:offs[b + 1]] for b in range(B)]
        return out

    def loudness(self, wavs: Sequence[np.ndarray], **config) -> Dict[str, object]:
        """Host signals -> their loudness and, with a target, the normalised signals.  wavs: one 1-D array per segment, all int16 or all
        floating, at any rate of the table (recordings as well as synthesis); further keywords: the fields of
        emotivoice_amd.loudness.LoudnessConfig (no target_lufs: measure only).  Needs no weights."""
        from .loudness import LoudnessConfig
        lc = LoudnessConfig(**config).validate()
        if not len(wavs):
            raise ValueError("wavs must hold at least one segment")
        arrs = [np.asarray(x) for x in wavs]
        is16 = arrs[0].dtype == np.int16
        for s, a in enumerate(arrs):
            if a.ndim != 1 or a.size < 1 or (a.dtype == np.int16) != is16 or not (is16 or np.issubdtype(a.dtype, np.floating)):
                raise ValueError("segment %d: non-empty 1-D arrays, all int16 or all floating" % s)
        flat = np.ascontiguousarray(np.concatenate([a.astype(np.int16 if is16 else np.float32, copy=False) for a in arrs]))
        lens = np.array([a.size for a in arrs], np.int64)
        return self.loudness_to_numpy(self.loudness_raw(len(arrs), flat.ctypes.data, is16, lens, lc))

    # -- true-peak metering and limiting (ev_limit): a 4x true-peak meter, a gain per sample that holds the ceiling and the limited waveform, on the device
    def limit_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, lens: np.ndarray, gains=None, config=None, flags: int = 0) -> _ffi.ev_limit_result:
        """ev_limit (include/evhip.h).  wav_ptr is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS; lens and gains (None: all 1) are
        host arrays.  config: an emotivoice_amd.limiter.LimiterConfig, an _ffi.ev_limit_config or None (the library's default: 16 kHz, -1 dBTP, 80
        and 800 samples).  The returned struct's device waveforms and host arrays stay valid until the next limit call on this engine."""
        ln = np.ascontiguousarray(lens, np.int64)
        if ln.size != B:
            raise ValueError("lens must have B = %d entries" % B)
        gn = None
        if gains is not None:
            gn = np.ascontiguousarray(gains, np.float32)
            if gn.shape != (B,):
                raise ValueError("gains must have B = %d entries" % B)
        c = config.validate().to_struct() if hasattr(config, "to_struct") else config
        res = _ffi.ev_limit_result()
        res.struct_size = C.sizeof(_ffi.ev_limit_result)
        self._check(self._lib.ev_limit(self._h, B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, ln.ctypes.data_as(C.c_void_p),
                                       gn.ctypes.data_as(C.c_void_p) if gn is not None else None, C.byref(c) if c is not None else None, flags,
                                       C.byref(res)))
        res._lens = ln.copy()      # the packing of res.wav / res.wav_i16, for limit_to_numpy
        self.last_limit = res
        return res

    def limit_to_numpy(self, res: _ffi.ev_limit_result, int16_only: bool = False, lens=None) -> Dict[str, object]:
        """Copies of the result's host arrays and one D2H copy of the fp32 output (with ``int16_only`` and a result that has it, of the int16
        output only; without it both).  lens: the call's lens, which cut the output into wav_list / wav_i16_list (None: the ones limit_raw kept
        with the struct)."""
        B = res.batch
        arr = lambda p, dt: np.ctypeslib.as_array(p, (B,)).astype(dt, copy=True)      # noqa: E731
        out: Dict[str, object] = dict(true_peak_in=arr(res.true_peak_in, np.float32), sample_peak_in=arr(res.sample_peak_in, np.float32),
                                      true_peak_out=arr(res.true_peak_out, np.float32), sample_peak_out=arr(res.sample_peak_out, np.float32),
                                      min_gain=arr(res.min_gain, np.float32), limited=arr(res.limited, np.int64), nonfinite=arr(res.nonfinite, np.int64))
        lens = np.asarray(res._lens if lens is None else lens, np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        if not (int16_only and res.wav_i16):
            out["wav"] = self.d2h(res.wav, (int(res.total),), np.float32)
            out["wav_list"] = [out["wav"][offs[b]:offs[b + 1]] for b in range(B)]
        if res.wav_i16:
            out["wav_i16"] = self.d2h(res.wav_i16, (int(res.total),), np.int16)
            out["wav_i16_list"] = [out["wav_i16"][offs[b]:offs[b + 1]] for b in range(B)]
        return out

    def limit(self, wavs: Sequence[np.ndarray], gains=None, **config) -> Dict[str, object]:
        """Host signals -> their peaks and the limited signals.  wavs: one 1-D array per segment, all int16 or all floating, at any rate of the
        table; gains: one pre-gain per segment (None: 1); further keywords: the fields of emotivoice_amd.limiter.LimiterConfig.  Needs no weights."""
        from .limiter import LimiterConfig
        lc = LimiterConfig(**config).validate()
        if not len(wavs):
            raise ValueError("wavs must hold at least one segment")
        arrs = [np.asarray(x) for x in wavs]
        is16 = arrs[0].dtype == np.int16
        for s, a in enumerate(arrs):
            if a.ndim != 1 or a.size < 1 or (a.dtype == np.int16) != is16 or not (is16 or np.issubdtype(a.dtype, np.floating)):
                raise ValueError("segment %d: non-empty 1-D arrays, all int16 or all floating" % s)
        flat = np.ascontiguousarray(np.concatenate([a.astype(np.int16 if is16 else np.float32, copy=False) for a in arrs]))
        lens = np.array([a.size for a in arrs], np.int64)
        return self.limit_to_numpy(self.limit_raw(len(arrs), flat.ctypes.data, is16, lens, gains, lc))

    def _measure_and_limit(self, B: int, wav_ptr: int, lens: np.ndarray, loudness, limiter, sample_rate: int, want_int16: bool, int16_only: bool = False):
        """``loudness=`` with ``limiter=`` on a device waveform: ev_loudness measure only, the pre-gain on the host (the gain rule without its
        sample-peak step), then ev_limit, which scales and limits in its one pass.  With ``limiter=`` alone the gains are 1.
        -> (ev_limit_result, the limiter's dict, the loudness dict or None)."""
        import dataclasses
        from .limiter import as_config as limiter_config, pre_gain
        mc = limiter_config(limiter, sample_rate, want_int16)
        gains, meas = None, None
        if loudness is not None:
            from .loudness import as_config as loudness_config
            lc = loudness_config(loudness, sample_rate)
            only = dataclasses.replace(lc, target_lufs=float("nan"), want_int16=False)
            meas = self.loudness_to_numpy(self.loudness_raw(B, wav_ptr, False, lens, only, _ffi.EV_FLAG_DEVICE_INPUTS))
            pairs = [pre_gain(float(l), lc) for l in meas["loudness"]]
            gains = np.array([g for g, _ in pairs], np.float32)
            meas["gain"], meas["flags"] = gains.copy(), np.array([f for _, f in pairs], np.uint8)
        lm = self.limit_raw(B, wav_ptr, False, lens, gains, mc, _ffi.EV_FLAG_DEVICE_INPUTS)
        return lm, self.limit_to_numpy(lm, int16_only=int16_only), meas

    def set_forced_durations(self, durations: np.ndarray):
        d = np.ascontiguousarray(durations, np.int64)
        self._check(self._lib.ev_set_forced_durations(self._h, d.ctypes.data_as(C.c_void_p), d.size))

    # -- helpers
    def d2h(self, dev_ptr: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        if out.nbytes:
            self._check(self._lib.ev_memcpy_d2h(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(dev_ptr), out.nbytes))
        return out

    def result_to_numpy(self, res: _ffi.ev_result, want_int16: bool = False, skip_wav: bool = False) -> Dict[str, object]:
        B = res.batch
        mel_lens = np.array([res.mel_lens[b] for b in range(B)], np.int32)
        mel_offs = np.array([res.mel_offsets[b] for b in range(B + 1)], np.int64)
        up = self.shapes.upsample_factor
        out: Dict[str, object] = dict(mel_lens=mel_lens, mel_offsets=mel_offs)
        if res.wav and not skip_wav:
            out["wav"] = self.d2h(res.wav, (res.total_samples,), np.float32)
            out["wav_list"] = [out["wav"][mel_offs[b] * up:mel_offs[b + 1] * up] for b in range(B)]
        if want_int16 and res.wav_i16 and not skip_wav:
            out["wav_i16"] = self.d2h(res.wav_i16, (res.total_samples,), np.int16)
        if res.mel:
            out["mel"] = self.d2h(res.mel, (res.total_frames, self.shapes.n_mels), np.float32)
            out["mel_list"] = [out["mel"][mel_offs[b]:mel_offs[b + 1]] for b in range(B)]
        if res.durations:
            out["durations"] = self.d2h(res.durations, (res.total_tokens,), np.int64)
            out["log_durations"] = self.d2h(res.log_durations, (res.total_tokens,), np.float32)
            out["pitch"] = self.d2h(res.pitch, (res.total_tokens,), np.float32)
            out["energy"] = self.d2h(res.energy, (res.total_tokens,), np.float32)
        return out

    # -- numpy convenience API
    def _synthesize_call(self, utts: Sequence[dict], alpha: float, flags: int, forced_durations, prosody):
        """The packing and the one ev_synthesize[_prosody] call of ``synthesize``: (ev_result, cu_seqlens)."""
        B = len(utts)
        packed = None
        if prosody is not None:
            from .prosody import pack_prosody
            packed = pack_prosody(prosody, [len(u["ling"]) for u in utts], alpha, forced=forced_durations is not None)
        ling = np.ascontiguousarray(np.concatenate([np.asarray(u["ling"], np.int64) for u in utts]))
        cu = np.zeros(B + 1, np.int32)
        cu[1:] = np.cumsum([len(u["ling"]) for u in utts])
        spk = np.ascontiguousarray([int(u["speaker"]) for u in utts], np.int64)
        style = np.ascontiguousarray(np.stack([np.asarray(u["style"], np.float32) for u in utts]))
        content = np.ascontiguousarray(np.stack([np.asarray(u["content"], np.float32) for u in utts]))
        if forced_durations is not None:
            self.set_forced_durations(forced_durations)
            flags |= _ffi.EV_FLAG_FORCED_DURATIONS
        if packed is None:
            res = self.synthesize_raw(B, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data, alpha, flags)
        else:
            res = self.synthesize_prosody_raw(B, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data, alpha,
                                              packed, flags)
        return res, cu

    def synthesize(self, utts: Sequence[dict], alpha: float = 1.0, want_int16: bool = False, vocoder: bool = True,
                   forced_durations: Optional[np.ndarray] = None, prosody=None, flac=None, loudness=None, limiter=None) -> Dict[str, object]:
        """utts: dicts with ling (N,) int64, speaker int, style (768,), content (768,) -- the four fields the
        reference builds per input line (inference_am_vocoder_joint.py:113-119).
        prosody: None (ev_synthesize), or one emotivoice_amd.prosody.Prosody per utterance (None entries = identity) or a single one
        for every utterance: ev_synthesize_prosody.  The returned pitch / energy / durations are the predictions either way.
        flac: None, True or one boolean per utterance: adds flac_list, the FLAC stream (``bytes``) of every selected utterance and None
        for the others, encoded on the device from the fp32 waveform with the wrapping conversion -- a stream decodes to
        wav_float_to_int16(wav_list[b]).
        loudness: None, a target in LUFS or an emotivoice_amd.loudness.LoudnessConfig: every utterance is normalised on the device
        (ev_loudness on the vocoder's waveform).  wav / wav_list then hold the normalised audio, want_int16 adds wav_i16 / wav_int16_list
        by the clamping rule (not EV_FLAG_WANT_INT16's wrapping cast), ``loudness`` holds the per-utterance figures, and flac encodes the
        normalised int16: a stream decodes to wav_int16_list[b].
        limiter: None, True, a true-peak ceiling in dBTP or an emotivoice_amd.limiter.LimiterConfig: every utterance goes through ev_limit
        on the device.  With ``loudness`` the gain to the target is no longer cut by the utterance's largest sample: ev_loudness only measures,
        the pre-gain (emotivoice_amd.limiter.pre_gain) goes into ev_limit, and the limiter holds the peaks sample by sample; ``loudness`` then
        holds the measurement and the pre-gain, ``limiter`` the limiter's per-utterance figures, and the audio, the int16 (clamping rule) and
        the FLAC streams are the limiter's.  The loudness is not measured again after the limiter: it sits at or slightly below the target."""
        if flac is not None and flac is not False and not vocoder:
            raise ValueError("flac needs the vocoder's waveform")
        if limiter is not None:
            if not vocoder:
                raise ValueError("limiter needs the vocoder's waveform")
            return self._synthesize_limited(utts, alpha, want_int16, forced_durations, prosody, flac, loudness, limiter)
        if loudness is not None:
            if not vocoder:
                raise ValueError("loudness needs the vocoder's waveform")
            return self._synthesize_normalised(utts, alpha, want_int16, forced_durations, prosody, flac, loudness)
        flags = 0
        if want_int16:
            flags |= _ffi.EV_FLAG_WANT_INT16
        if not vocoder:
            flags |= _ffi.EV_FLAG_NO_VOCODER
        res, cu = self._synthesize_call(utts, alpha, flags, forced_durations, prosody)
        out = self.result_to_numpy(res, want_int16)
        out["cu_seqlens"] = cu
        if flac is not None and flac is not False:
            out["flac_list"] = self._flac_of_result(res, flac)
        return out

    def _synthesize_normalised(self, utts, alpha, want_int16, forced_durations, prosody, flac, loudness) -> Dict[str, object]:
        """``synthesize`` with ``loudness=``: the synthesis call, ev_loudness on its device waveform, D2H copies of the normalised audio only."""
        from .loudness import as_config
        want_flac = flac is not None and flac is not False
        lc = as_config(loudness, int(self.shapes.sr), want_int16 or want_flac)
        res, cu = self._synthesize_call(utts, alpha, 0, forced_durations, prosody)
        out = self.result_to_numpy(res, skip_wav=True)
        out["cu_seqlens"] = cu
        B, up = res.batch, self.shapes.upsample_factor
        ld = self.loudness_raw(B, res.wav, False, np.diff(out["mel_offsets"]) * up, lc, _ffi.EV_FLAG_DEVICE_INPUTS)
        norm = self.loudness_to_numpy(ld)
        out["wav"], out["wav_list"] = norm.pop("wav"), norm.pop("wav_list")
        i16, i16_list = norm.pop("wav_i16", None), norm.pop("wav_i16_list", None)
        if want_int16 or want_flac:
            out["wav_i16"], out["wav_int16_list"] = i16, i16_list
        out["loudness"] = norm
        if want_flac:
            out["flac_list"] = self._flac_of_result(res, flac, pcm_i16=ld.wav_i16)
        return out

    def _synthesize_limited(self, utts, alpha, want_int16, forced_durations, prosody, flac, loudness, limiter) -> Dict[str, object]:
        """``synthesize`` with ``limiter=``: the synthesis call, ev_loudness (measure only) when a target is given, ev_limit on the device
        waveform, D2H copies of the limited audio only."""
        want_flac = flac is not None and flac is not False
        res, cu = self._synthesize_call(utts, alpha, 0, forced_durations, prosody)
        out = self.result_to_numpy(res, skip_wav=True)
        out["cu_seqlens"] = cu
        B, up = res.batch, self.shapes.upsample_factor
        lm, lim, meas = self._measure_and_limit(B, res.wav, np.diff(out["mel_offsets"]) * up, loudness, limiter, int(self.shapes.sr), want_int16 or want_flac)
        out["wav"], out["wav_list"] = lim.pop("wav"), lim.pop("wav_list")
        i16, i16_list = lim.pop("wav_i16", None), lim.pop("wav_i16_list", None)
        if want_int16 or want_flac:
            out["wav_i16"], out["wav_int16_list"] = i16, i16_list
        if meas is not None:
            out["loudness"] = meas
        out["limiter"] = lim
        if want_flac:
            out["flac_list"] = self._flac_of_result(res, flac, pcm_i16=lm.wav_i16)
        return out

    def vocoder(self, mels: Sequence[np.ndarray], want_int16: bool = False) -> Dict[str, object]:
        """mels: list of (n_mels, T_b) arrays (the reference's (B,80,T) layout per utterance), fp32 or fp16."""
        is16 = mels[0].dtype == np.float16
        flat = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(m, mels[0].dtype).ravel() for m in mels]))
        lens = np.array([m.shape[1] for m in mels], np.int32)
        flags = _ffi.EV_FLAG_WANT_INT16 if want_int16 else 0
        res = self.vocoder_raw(len(mels), flat.ctypes.data, is16, lens, flags)
        return self.result_to_numpy(res, want_int16)

    # receptive field of the generator in mel frames per side: conv_post 3 samples -> 60-sample ResBlock halos per stage through the
    # four transposed convs -> 11 frames, + conv_pre 3 = 14 (derivation in DESIGN.md section 4); 16 is used
    VOCODER_CONTEXT_FRAMES = 16

    def vocoder_chunked(self, mel: np.ndarray, chunk_frames: int = 256, context: Optional[int] = None):
        """Streaming vocoding of one long mel (n_mels, T): yields the waveform of consecutive chunks of ``chunk_frames`` frames.
        Every chunk is vocoded with ``context`` extra frames on each side and the centre is kept; because every output sample
        only depends on +-14 mel frames and the kernels are position-independent, the concatenation is BIT-IDENTICAL to vocoding
        the whole mel at once (tests/test_gpu_parity.py).  Bounds the vocoder workspace for arbitrarily long utterances and gives
        first audio after one chunk (ROADMAP "Support longer text")."""
        ctx = self.VOCODER_CONTEXT_FRAMES if context is None else context
        up = self.shapes.upsample_factor
        T = mel.shape[1]
        for a in range(0, T, chunk_frames):
            b = min(T, a + chunk_frames)
            lo, hi = max(0, a - ctx), min(T, b + ctx)
            wav = self.vocoder([np.ascontiguousarray(mel[:, lo:hi])])["wav"]
            yield wav[(a - lo) * up:(b - lo) * up]

    def get_stage(self, name: str) -> np.ndarray:
        """Stage tap of the last call (SURVEY.md Appendix C names; needs keep_stages=True): (rows, C) fp32."""
        need = self._lib.ev_get_stage(self._h, name.encode(), None, 0)
        if need < 0:
            raise EVError(self._lib.ev_last_error(self._h).decode())
        if name in ("dur", "dur_eff", "mel_len"):      # "log_p_attn" (after align): the (T_b, N_b) fp32 blocks, concatenated
            out = np.empty(need // 8, np.int64)
        else:
            out = np.empty(need // 4, np.float32)
        got = self._lib.ev_get_stage(self._h, name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes)
        if got < 0:
            raise EVError(self._lib.ev_last_error(self._h).decode())
        return out

    def timings(self) -> Dict[str, float]:
        out = {}
        ms = C.c_float()
        for name in ("total", "am", "encoder", "variance", "decoder", "vocoder"):
            if self._lib.ev_get_timing(self._h, name.encode(), C.byref(ms)) == 0:
                out[name] = float(ms.value)
        return out

    def launch_records(self) -> List[dict]:
        """Per-launch records of the last profiled call (set_profiling(True)), in launch order."""
        out = []
        r = _ffi.ev_launch_record()
        for i in range(self._lib.ev_launch_record_count(self._h)):
            self._lib.ev_get_launch_record(self._h, i, C.byref(r))
            out.append(dict(name=r.name.decode(), M=r.M, N=r.N, K=r.K, taps=r.taps, dil=r.dil, ms=float(r.ms), flops=float(r.flops), bytes=float(r.bytes)))
        return out

    def kernel_stats(self) -> List[dict]:
        out = []
        st = _ffi.ev_kernel_stat()
        for i in range(self._lib.ev_kernel_stat_count(self._h)):
            self._lib.ev_get_kernel_stat(self._h, i, C.byref(st))
            out.append(dict(name=st.name.decode(), launches=st.launches, ms=float(st.ms), flops=float(st.flops), bytes=float(st.bytes)))
        return out
