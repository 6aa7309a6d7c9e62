"""Object wrapper over the libevhip.so handle: numpy / raw-pointer in, numpy out.  No torch needed."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _ffi
from .config import EVShapes
from .engine_audio import EVAudio, cut, host_array
from .output_chain import resolve as resolve_chain, run as run_chain
from .packing import pack_utts


class EVError(RuntimeError):
    pass


# the chain's audio keys (output_chain.AUDIO_KEYS) under the names each entry point returns them
SYNTHESIZE_NAMES = (("wav", "wav"), ("wav_list", "wav_list"), ("wav_i16", "wav_i16"), ("wav_i16_list", "wav_int16_list"))
SYNTHESIZE_LONG_NAMES = (("wav", "wav"), ("wav_list", "docs"), ("wav_i16", "wav_i16"), ("wav_i16_list", "docs_i16"))

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


class EVEngine(EVAudio):
    """One handle = one GPU + one stream + one workspace (include/evhip.h).  Not thread-safe.  The audio utilities (features, pitch, resample,
    stitch, compare, flac, loudness, limit, deliver, score, denoise) are EVAudio's (engine_audio.py)."""

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
        EVAudio.__init__(self)      # the utilities' setups, their keys and ``last_<utility>``

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
        self._weights_changed()

    def load_blob_device(self, dptr: int, nbytes: int, keepalive=None):
        """Borrow a blob that already lives in device memory (e.g. after an RCCL broadcast)."""
        self._blob_keepalive = keepalive
        self._check(self._lib.ev_load_weights_device(self._h, C.c_void_p(dptr), nbytes, None))
        self._weights_changed()

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
        return self._call("align", B, C.c_void_p(ling_ptr), cu.ctypes.data_as(C.c_void_p), C.c_void_p(speaker_ptr), C.c_void_p(style_ptr),
                          C.c_void_p(content_ptr), C.c_void_p(mel_ptr), 1 if mel_is_f16 else 0, ml.ctypes.data_as(C.c_void_p),
                          C.c_void_p(pitch_ptr) if pitch_ptr else None, C.c_void_p(energy_ptr) if energy_ptr else None, flags)

    def align_to_numpy(self, res: _ffi.ev_align_result) -> Dict[str, object]:
        B, NT = res.batch, res.total_tokens
        out: Dict[str, object] = dict(mel_lens=host_array(res.mel_lens, B, np.int32), mel_offsets=host_array(res.mel_offsets, B + 1, np.int64),
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
        ling, cu, spk, style, content = pack_utts(utts)
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
        out["durations_list"] = cut(out["durations"], cu)
        return out

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
        ling, cu, spk, style, content = pack_utts(utts)
        if forced_durations is not None:
            self.set_forced_durations(forced_durations)
            flags |= _ffi.EV_FLAG_FORCED_DURATIONS
        if packed is None:
            res = self.synthesize_raw(B, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data, alpha, flags)
        else:
            res = self.synthesize_prosody_raw(B, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data, alpha,
                                              packed, flags)
        return res, cu

    def _denoise_ready(self, denoise):
        """Before a synthesis whose waveform ev_denoise will read: measure the vocoder's own bias now if the config asks for it and none is
        kept, because measuring runs the vocoder and would replace that waveform."""
        if denoise is not None and denoise.bias is None and denoise.tables_key() not in self._denoise_own_bias:
            self.denoise_setup(denoise)

    def synthesize(self, utts: Sequence[dict], alpha: float = 1.0, want_int16: bool = False, vocoder: bool = True,
                   forced_durations: Optional[np.ndarray] = None, prosody=None, flac=None, loudness=None, limiter=None, delivery=None,
                   denoise=None, stretch=None, watermark=None) -> Dict[str, object]:
        """utts: dicts with ling (N,) int64, speaker int, style (768,), content (768,) -- the four fields the
        reference builds per input line (inference_am_vocoder_joint.py:113-119).
        prosody: None (ev_synthesize), or one emotivoice_amd.prosody.Prosody per utterance (None entries = identity) or a single one
        for every utterance: ev_synthesize_prosody.  The returned pitch / energy / durations are the predictions either way.
        The seven arguments below are the output chain on the device, denoise -> stretch -> watermark -> loudness -> limiter -> delivery -> flac; emotivoice_amd/output_chain.py
        states once, for every combination, the order, which stage makes the int16, what is copied to the host and what a FLAC stream decodes to.
        flac: None, True, one boolean per utterance or an emotivoice_amd.flac.FlacConfig (every utterance, with its LPC / MD5 / block settings;
        the sample rate is the engine's and the conversion stays the wrapping one): adds flac_list, the FLAC stream (``bytes``) of every selected
        utterance and None for the others.  Without another stage a stream decodes to wav_float_to_int16(wav_list[b]).
        loudness: None, a target in LUFS or an emotivoice_amd.loudness.LoudnessConfig: every utterance is normalised on the device (ev_loudness).
        wav / wav_list then hold the normalised audio, want_int16 adds wav_i16 / wav_int16_list by the clamping rule (not EV_FLAG_WANT_INT16's
        wrapping cast) and ``loudness`` holds the per-utterance figures.
        limiter: None, True, a true-peak ceiling in dBTP or an emotivoice_amd.limiter.LimiterConfig: every utterance goes through ev_limit
        on the device; ``limiter`` holds its per-utterance figures.  With ``loudness`` the gain to the target is no longer cut by the utterance's
        largest sample: ev_loudness only measures and ``loudness`` holds the measurement and the pre-gain.  The loudness is not measured again
        after the limiter: it sits at or slightly below the target.
        delivery: None, a sample rate in Hz (int16 at that rate) or an emotivoice_amd.delivery.DeliveryConfig: ev_deliver runs on the device
        after the last of the stages above and the response is what it writes: delivered_list (one float32 / int16 / uint8 array per utterance,
        at delivered_rate), ``delivery`` (peak, clipped, n_samples per utterance).  wav / wav_list / wav_i16 are then not returned -- the 16 kHz
        waveform stays on the device -- and want_int16 is ignored.  With ``flac`` the encoding must be "s16".
        denoise: None, True, a strength, a dict of DenoiseConfig's fields or an emotivoice_amd.denoise.DenoiseConfig: ev_denoise runs FIRST, on the
        vocoder's waveform -- strength times the magnitude spectrum of the vocoder's answer to an all-zero mel (measured once per engine, or
        config.bias) is subtracted from every STFT cell; the lengths do not change (a waveform of whole frames).  ``denoise`` in the result holds
        lens_out and, with report=True, removed_db.  The default strength 0.01 is an unmeasured starting value (emotivoice_amd.denoise).
        stretch: None, a speed, one speed per utterance or an emotivoice_amd.stretch.StretchConfig (speed, seconds or samples per utterance):
        ev_stretch runs SECOND, after ev_denoise, and changes the length of every waveform at the same pitch (WSOLA; not the reference's Rubber
        Band, see emotivoice_amd.stretch for what is not verified).  wav_list (and wav_int16_list, delivered_list) have the new lengths and
        ``stretch`` holds lens_in, lens_out, speed and the search's figures.  durations, mel_lens and mel_offsets stay on the MODEL's clock: they
        describe the mel the vocoder read, not the stretched waveform.  The packed ``wav`` is cut by stretch["offsets"], not by mel_offsets.
        watermark: None, a key, 'KEY[:PAYLOAD:NBITS]', a dict or an emotivoice_amd.watermark.WatermarkConfig (payload, nbits and strength_db may
        have one entry per utterance): ev_watermark runs THIRD, after ev_stretch and before ev_loudness, and marks every waveform with the keyed
        pattern that EVEngine.watermark_detect finds again (see emotivoice_amd.watermark for what is not verified: nobody has listened to it, no
        security claim).  Its output has whole hops, as ev_denoise's; ``watermark`` in the result holds lens_out, offsets, key, payload, nbits
        and strength_db."""
        plan = resolve_chain(self.shapes.sr, len(utts), denoise, loudness, limiter, delivery, flac, vocoder, flac_convert="wrap", stretch=stretch,
                             watermark=watermark)
        flags = (_ffi.EV_FLAG_WANT_INT16 if want_int16 and not plan.staged else 0) | (0 if vocoder else _ffi.EV_FLAG_NO_VOCODER)
        self._denoise_ready(plan.denoise)
        res, cu = self._synthesize_call(utts, alpha, flags, forced_durations, prosody)
        out = self.result_to_numpy(res, want_int16, skip_wav=plan.staged)
        out["cu_seqlens"] = cu
        lens = np.diff(out["mel_offsets"] * self.shapes.upsample_factor)
        want_i16 = want_int16 or plan.flac is not None
        chain = run_chain(self, plan, res.wav, lens, want_i16)
        if plan.denoise is not None:      # whole frames in, whole frames out: every offset above still holds
            assert np.array_equal(chain.figures["denoise"]["lens_out"], lens), "ev_denoise changed a length of whole frames"
        return chain.into(out, SYNTHESIZE_NAMES if want_i16 else SYNTHESIZE_NAMES[:2])

    def synthesize_long(self, documents: Sequence, alpha: float = 1.0, prosody=None, config=None, flac=None, loudness=None, limiter=None,
                        delivery=None, denoise=None, stretch=None, watermark=None) -> Dict[str, object]:
        """Documents of several sentences each -> one waveform per document and the time of every sentence in it.  documents: each a
        dict(utts=[utt dicts as ``synthesize`` takes], pauses=[one per joint: a class of emotivoice_amd.longform.pauses_ms, milliseconds, or
        None]) or a pair (utts, pauses); pauses None = "sentence" everywhere.  prosody: as ``synthesize`` takes it, over the sentences of all
        documents in order.  config: an emotivoice_amd.longform.StitchConfig (None: its defaults, which have not been measured on a released
        checkpoint).  One ev_synthesize[_prosody] call, one ev_stitch call on its device waveform and one D2H copy (int16 with
        config.want_int16, else fp32).  All sentences go into one synthesize call: more than it takes raises; splitting is the caller's.
        The seven arguments below are the output chain, per document, after ev_stitch; emotivoice_amd/output_chain.py states its rules.
        flac=True or an emotivoice_amd.flac.FlacConfig (its LPC / MD5 / block settings; the sample rate is the engine's; ``md5`` costs one serial
        chain per document) adds flac_list, one FLAC stream (``bytes``) per document (it turns config.want_int16 on, so
        ``documents`` are the int16 ones a stream decodes to).
        loudness: None, a target in LUFS or an emotivoice_amd.loudness.LoudnessConfig: every document is normalised on the device (ev_loudness:
        one gain per document, so the balance between its sentences stays); ``documents`` (int16 by the clamping rule with config.want_int16)
        then hold the normalised audio and ``loudness`` the per-document figures.
        limiter: as ``synthesize`` takes it, per document; ``documents`` hold the limited audio and ``limiter`` the per-document figures.
        delivery: as ``synthesize`` takes it, per document: ``documents`` is then delivered_list (at delivered_rate, in the delivery's encoding),
        ``delivery`` holds peak / clipped / n_samples, no 16 kHz audio is copied to the host, config.want_int16 is ignored and flac needs the
        encoding "s16".  sentence_times are in SECONDS and hold at any delivered rate; seg_pos / seg_start / seg_end / doc_lens and
        ``sample_rate`` stay on the engine's 16 kHz clock (delivered_rate is returned next to them).
        denoise: as ``synthesize`` takes it, per document, right after ev_stitch.  Its output has whole hops: a document whose length is no
        multiple of the hop (256) loses the up to 255 samples after its last whole hop, doc_lens then holds the new lengths and ``denoise``
        lens_out (and removed_db with report=True).
        stretch: as ``synthesize`` takes it, per DOCUMENT (a sequence has one entry per document), after ev_stitch and ev_denoise.  doc_lens and
        doc_offsets become the stretched ones and ``stretch`` holds lens_in, lens_out, speed and the search's figures.  sentence_times are
        scaled by L_out / L_in of their document: WSOLA follows that line only to within its lag range, so a time is off by up to 128 samples
        (8 ms at 16 kHz) plus the rounding of the frame positions.  seg_pos, seg_start and seg_end stay on the clock BEFORE the stretch.
        watermark: as ``synthesize`` takes it, per DOCUMENT (a sequence has one entry per document), after ev_stretch.  Its output has whole
        hops, so a document loses the up to 255 samples after its last whole hop, as under denoise; doc_lens and doc_offsets are the marked
        ones."""
        import dataclasses
        from .longform import StitchConfig, flatten_documents, plan_document
        sc = (config or StitchConfig()).validate()
        if int(sc.sample_rate) != int(self.shapes.sr):
            raise ValueError("config.sample_rate %d is not the engine's %d" % (sc.sample_rate, self.shapes.sr))
        plan = resolve_chain(sc.sample_rate, None, denoise, loudness, limiter, delivery, flac, stretch=stretch, watermark=watermark)
        stitch_i16 = bool(sc.want_int16 or plan.flac is not None) and plan.delivery is None      # a delivered response has no 16 kHz int16
        if stitch_i16 != sc.want_int16:
            sc = dataclasses.replace(sc, want_int16=stitch_i16).validate()
        utts, seg_doc, pauses = flatten_documents(documents)
        if plan.stretch is not None:
            plan.stretch.per_segment(len(documents), sc.sample_rate)      # one entry per document, before any library call
        if plan.watermark is not None:
            plan.watermark.per_segment(len(documents))
        S = len(utts)
        if S > 65535:
            raise ValueError("%d sentences exceed the 65535 segments of one ev_stitch call; split the documents over several calls" % S)
        seg_doc, pause_after = plan_document(seg_doc, pauses, sc.sample_rate)
        self._denoise_ready(plan.denoise)
        res, _ = self._synthesize_call(utts, alpha, 0, None, prosody)
        mel_offs = host_array(res.mel_offsets, S + 1, np.int64) * self.shapes.upsample_factor
        st = self.stitch_raw(S, res.wav, mel_offs[:-1], np.diff(mel_offs), seg_doc, pause_after, sc, _ffi.EV_FLAG_DEVICE_INPUTS)
        out = self.stitch_to_numpy(st, int16_only=sc.want_int16, skip_wav=plan.staged)
        reader = ("denoise" if plan.denoise is not None else "stretch" if plan.stretch is not None else "watermark" if plan.watermark is not None else "limiter" if plan.limiter is not None else "loudness" if plan.loudness is not None else
                  "delivery" if plan.delivery is not None else "flac" if plan.flac is not None else None)
        empty = [d for d in range(st.batch_docs) if out["doc_lens"][d] < 1]
        if empty and reader:
            raise ValueError("%s: document %d is empty after the cut" % (reader, empty[0]))
        chain = run_chain(self, plan, st.wav, out["doc_lens"], sc.want_int16, sc.want_int16, st.wav_i16)
        chain.into(out, SYNTHESIZE_LONG_NAMES)
        if plan.denoise is not None:
            out["doc_lens"], out["doc_offsets"] = out["denoise"]["lens_out"], out["denoise"]["offsets"]
        scale = np.ones(st.batch_docs, np.float64)      # a sentence's time in its stretched document: its time before, times L_out / L_in
        if plan.stretch is not None:
            out["doc_lens"], out["doc_offsets"] = out["stretch"]["lens_out"], out["stretch"]["offsets"]
            scale = out["stretch"]["lens_out"] / out["stretch"]["lens_in"]
        if plan.watermark is not None:
            out["doc_lens"], out["doc_offsets"] = out["watermark"]["lens_out"], out["watermark"]["offsets"]
        sr = float(sc.sample_rate)
        start = out["seg_pos"] / sr * scale[seg_doc]
        end = (out["seg_pos"] + (out["seg_end"] - out["seg_start"])) / sr * scale[seg_doc]
        out["documents"] = out["delivered_list"] if plan.delivery is not None else out["docs_i16"] if sc.want_int16 else out["docs"]
        out["seg_doc"] = seg_doc
        out["sentence_times"] = [[(float(start[s]), float(end[s])) for s in np.nonzero(seg_doc == d)[0]] for d in range(st.batch_docs)]
        out["sample_rate"] = int(sc.sample_rate)
        return out

    def synthesize_fit(self, utts: Sequence[dict], seconds, prosody=None, **chain) -> Dict[str, object]:
        """Every utterance in exactly its time slot: ``seconds`` (a scalar or one value per utterance) -> len(wav_list[b]) ==
        round(seconds[b] * sample rate).  Three steps: an acoustic pass without the vocoder gives the natural mel_lens; a second synthesis runs
        with alpha = target / natural per utterance, clamped to [0.5, 2] (the model's durations are whole frames and its own predictions, so
        this only comes close); ``stretch=StretchConfig(samples=target)`` closes the rest on the waveform -- a few per cent, where a
        time-domain stretch is cleanest.  prosody: as ``synthesize`` takes it, but without a speed or alpha of its own (ValueError): the
        duration scale is this call's.  **chain: the other output-chain arguments and want_int16 of ``synthesize``.  Returns what ``synthesize``
        returns and ``fit``: natural_samples, model_samples, target_samples and residual_speed (model / target, what the stretch closed) per
        utterance.  A target outside [0.5, 2] of what the model reaches is refused by ev_stretch's ratio rule."""
        import dataclasses
        from .prosody import Prosody
        from .stretch import StretchConfig, fit_alpha
        B, sr, up = len(utts), int(self.shapes.sr), int(self.shapes.upsample_factor)
        for k in ("stretch", "alpha", "vocoder", "forced_durations"):
            if k in chain:
                raise ValueError("synthesize_fit sets %s itself" % k)
        plist = list(prosody) if isinstance(prosody, (list, tuple)) else [prosody] * B
        if len(plist) != B:
            raise ValueError("prosody: one entry per utterance (%d), got %d" % (B, len(plist)))
        for b, p in enumerate(plist):
            if p is not None and (p.speed is not None or p.alpha is not None):
                raise ValueError("prosody[%d] has a speed or alpha of its own: synthesize_fit sets the duration scale" % b)
        sc = StretchConfig(seconds=seconds if np.ndim(seconds) == 0 else list(seconds)).validate()
        _, targets = sc.per_segment(B, sr)
        natural = self.synthesize(utts, vocoder=False, prosody=prosody)["mel_lens"].astype(np.int64) * up
        alphas = [fit_alpha(int(n), int(t)) for n, t in zip(natural, targets)]
        fitted = [dataclasses.replace(p, alpha=a) if p is not None else Prosody(alpha=a) for p, a in zip(plist, alphas)]
        out = self.synthesize(utts, prosody=fitted, stretch=StretchConfig(samples=[int(t) for t in targets]), **chain)
        model = out["mel_lens"].astype(np.int64) * up
        out["fit"] = dict(natural_samples=natural, model_samples=model, target_samples=np.array(targets, np.int64), alpha=np.array(alphas, np.float64),
                          residual_speed=model / np.array(targets, np.float64))
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
