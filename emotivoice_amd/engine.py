"""Object wrapper over the libevhip.so handle: numpy / raw-pointer in, numpy out.  No torch needed."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _ffi
from .config import EVShapes
from .delivery import delivery_config
from .denoise import denoise_config, removed_db
from .engine_audio import EVAudio, cut, host_array
from .limiter import as_config as limiter_config, pre_gain
from .loudness import as_config as loudness_config
from .packing import pack_utts


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
        self.feature_config = self.resample_config = self.delivery_config = self._delivery_key = None      # set by features_setup() / resample_setup() / deliver_setup()
        self.denoise_config = self._denoise_key = None      # set by denoise_setup()
        self._denoise_own_bias: Dict[tuple, np.ndarray] = {}      # the vocoder's own bias per (n_fft, hop), measured by denoise_setup on the loaded weights
        for name in ("align", "features", "pitch", "resample", "stitch", "compare", "flac", "loudness", "limit", "deliver", "denoise"):
            setattr(self, "last_" + name, None)                # the ev_<name>_result of the last call (_call)

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
        self._denoise_own_bias.clear()
        self._denoise_key = None

    def load_blob_device(self, dptr: int, nbytes: int, keepalive=None):
        """Borrow a blob that already lives in device memory (e.g. after an RCCL broadcast)."""
        self._blob_keepalive = keepalive
        self._check(self._lib.ev_load_weights_device(self._h, C.c_void_p(dptr), nbytes, None))
        self._denoise_own_bias.clear()
        self._denoise_key = None

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
        if denoise is not None and denoise.bias is None and (int(denoise.n_fft), int(denoise.hop)) not in self._denoise_own_bias:
            self.denoise_setup(denoise)

    def _denoise_stage(self, wav_ptr: int, lens: np.ndarray, denoise, want_int16: bool, int16_only: bool, last_stage: bool):
        """ev_denoise as the first output stage, on a packed device fp32 waveform: (ev_denoise_result, its host figures -- lens_out, offsets, with
        ``denoise.report`` removed_db from ev_compare on the two device waveforms, and the audio when it is the last stage)."""
        import dataclasses
        dev = _ffi.EV_FLAG_DEVICE_INPUTS
        dc = dataclasses.replace(denoise, want_int16=bool(last_stage and (denoise.want_int16 or want_int16))).validate()
        if self._denoise_key != dc.key():
            self.denoise_setup(dc)
        B = len(lens)
        res = self.denoise_raw(B, wav_ptr, False, lens, None, dev)
        got = self.denoise_to_numpy(res, int16_only=int16_only, skip_wav=not last_stage)
        if dc.report:
            if np.array_equal(got["lens_out"], np.asarray(lens, np.int64)):      # the same packing on both sides: one call
                cmp = self.compare_to_numpy(self.compare_raw(B, res.wav, wav_ptr, lens, dev))
                got["removed_db"] = removed_db(cmp["sum_d2"], cmp["sum_y2"])
            else:                                                                 # a length was cut to whole hops: utterance by utterance
                offs_in, rd = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]), []
                for b in range(B):
                    cmp = self.compare_to_numpy(self.compare_raw(1, res.wav + 4 * int(got["offsets"][b]), wav_ptr + 4 * int(offs_in[b]),
                                                                 got["lens_out"][b:b + 1], dev))
                    rd.append(removed_db(cmp["sum_d2"], cmp["sum_y2"])[0])
                got["removed_db"] = np.array(rd, np.float64)
        return res, got

    def _finish(self, wav_ptr: int, lens: np.ndarray, loudness, limiter, want_int16: bool, int16_only: bool, delivery=None, denoise=None):
        """The output stages between the synthesis (or ev_stitch) and ev_flac, on a packed device fp32 waveform.  loudness / limiter: a
        LoudnessConfig / LimiterConfig or None.  loudness alone: ev_loudness scales; limiter alone: ev_limit; both: ev_loudness measures only,
        the pre-gain is worked out on the host (the gain rule without its sample-peak step) and ev_limit scales and limits in its one pass.
        The last stage also writes the clamped int16 with ``want_int16``.  -> (the audio copied from the last stage: wav / wav_list and,
        where the stage made it, wav_i16 / wav_i16_list, by ``int16_only`` as ``*_to_numpy`` reads it; the loudness figures or None; the
        limiter's figures or None; the last stage's device int16 waveform or None; ev_deliver's result or None).
        delivery: a DeliveryConfig or None.  With it ev_deliver runs last, on the fp32 device waveform of the stage before it (``wav_ptr`` when
        there is none); the earlier stages then make no int16 and none of their audio is copied to the host: the delivered bytes are the audio
        (delivered_list, delivered_rate and ``delivery`` = peak / clipped / n_samples in the returned audio)."""
        import dataclasses
        B, dev = len(lens), _ffi.EV_FLAG_DEVICE_INPUTS
        last = figures = limited = gains = denoised = None
        if delivery is not None:
            want_int16 = False
        if denoise is not None:      # first: the later stages measure and shape the audio that is delivered
            last, denoised = self._denoise_stage(wav_ptr, lens, denoise, want_int16, int16_only, loudness is None and limiter is None and delivery is None)
            wav_ptr, lens = last.wav, denoised["lens_out"]
        if loudness is not None:
            lc = (dataclasses.replace(loudness, want_int16=loudness.want_int16 or want_int16) if limiter is None else
                  dataclasses.replace(loudness, target_lufs=float("nan"), want_int16=False))
            last = self.loudness_raw(B, wav_ptr, False, lens, lc, dev)
            figures = self.loudness_to_numpy(last, int16_only=int16_only, skip_wav=delivery is not None)
        if limiter is not None:
            if loudness is not None:
                pairs = [pre_gain(float(l), loudness) for l in figures["loudness"]]
                gains = np.array([g for g, _ in pairs], np.float32)
                figures["gain"], figures["flags"] = gains.copy(), np.array([f for _, f in pairs], np.uint8)
            last = self.limit_raw(B, wav_ptr, False, lens, gains, dataclasses.replace(limiter, want_int16=limiter.want_int16 or want_int16), dev)
            limited = self.limit_to_numpy(last, int16_only=int16_only, skip_wav=delivery is not None)
        src = limited if limited is not None else figures if figures is not None else denoised if denoised is not None else {}
        audio = {k: src.pop(k) for k in ("wav", "wav_list", "wav_i16", "wav_i16_list") if k in src}
        if denoised is not None:
            audio["denoise"] = denoised
        if delivery is None:
            return audio, figures, limited, last.wav_i16 if last is not None else None, None
        sr = int(self.shapes.sr)
        if self._delivery_key != delivery.key(sr):
            self.deliver_setup(delivery, sr)
        dres = self.deliver_raw(B, last.wav if last is not None else wav_ptr, False, lens, None, dev)
        got = self.deliver_to_numpy(dres, delivery)
        audio = dict(delivered_list=got["delivered_list"], delivered_rate=int(delivery.sample_rate),
                     delivery=dict(peak=got["peak"], clipped=got["clipped"], n_samples=got["n_samples"], encoding=delivery.encoding))
        if denoised is not None:
            audio["denoise"] = denoised
        return audio, figures, limited, None, dres

    def _flac_delivered(self, sel, dres, given, sample_rate: int, **kw) -> List[Optional[bytes]]:
        """The selected utterances of an ev_deliver result (int16) as FLAC at the delivered rate: one ev_flac call per utterance, since every
        utterance of the result starts on its own 16-byte boundary and ev_flac takes its segments back to back."""
        fc = self._flac_config(given, int(sample_rate), **kw)
        out: List[Optional[bytes]] = [None] * dres.batch
        for b in range(dres.batch):
            if sel[b]:
                fr = self.flac_raw(1, dres.data + int(dres.byte_offsets[b]), True, [int(dres.n_samples[b])], fc, _ffi.EV_FLAG_DEVICE_INPUTS)
                out[b] = self.flac_to_numpy(fr)["streams"][0]
        return out

    def _flac_config(self, given, sample_rate: int, **kw):
        """The FlacConfig of a ``flac=`` argument: a given one with the engine's sample rate (and ``kw``), else the defaults."""
        import dataclasses
        from .flac import FlacConfig
        if isinstance(given, FlacConfig):
            return dataclasses.replace(given, sample_rate=int(sample_rate), **kw).validate()
        return FlacConfig(sample_rate=int(sample_rate), **kw)

    def _flac_runs(self, sel: np.ndarray, offsets: np.ndarray, wav_ptr: int, pcm_i16: Optional[int], given=None) -> List[Optional[bytes]]:
        """The segments that ``sel`` selects of a packed device waveform, as FLAC: one ev_flac call per run of consecutive selected segments
        (ev_flac takes its segments back to back), from the int16 waveform ``pcm_i16`` when there is one, else from the fp32 ``wav_ptr`` with
        the wrapping conversion."""
        fc = self._flac_config(given, int(self.shapes.sr), convert="wrap")
        out: List[Optional[bytes]] = [None] * len(sel)
        edges = np.flatnonzero(np.diff(np.concatenate([[0], sel, [0]]).astype(np.int8)))      # where a run begins, where it ends, ...
        for b, e in zip(edges[::2].tolist(), edges[1::2].tolist()):
            src = pcm_i16 + 2 * int(offsets[b]) if pcm_i16 else wav_ptr + 4 * int(offsets[b])
            fr = self.flac_raw(e - b, src, bool(pcm_i16), np.diff(offsets[b:e + 1]), fc, _ffi.EV_FLAG_DEVICE_INPUTS)
            out[b:e] = self.flac_to_numpy(fr)["streams"]
        return out

    def synthesize(self, utts: Sequence[dict], alpha: float = 1.0, want_int16: bool = False, vocoder: bool = True,
                   forced_durations: Optional[np.ndarray] = None, prosody=None, flac=None, loudness=None, limiter=None, delivery=None,
                   denoise=None) -> Dict[str, object]:
        """utts: dicts with ling (N,) int64, speaker int, style (768,), content (768,) -- the four fields the
        reference builds per input line (inference_am_vocoder_joint.py:113-119).
        prosody: None (ev_synthesize), or one emotivoice_amd.prosody.Prosody per utterance (None entries = identity) or a single one
        for every utterance: ev_synthesize_prosody.  The returned pitch / energy / durations are the predictions either way.
        flac: None, True, one boolean per utterance or an emotivoice_amd.flac.FlacConfig (every utterance, with its LPC / MD5 / block settings;
        the sample rate is the engine's and the conversion stays the wrapping one): adds flac_list, the FLAC stream (``bytes``) of every selected utterance and None
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
        the FLAC streams are the limiter's.  The loudness is not measured again after the limiter: it sits at or slightly below the target.
        delivery: None, a sample rate in Hz (int16 at that rate) or an emotivoice_amd.delivery.DeliveryConfig: ev_deliver runs on the device
        after the last of the stages above (on the vocoder's waveform when there is none) and the response is what it writes: delivered_list
        (one float32 / int16 / uint8 array per utterance, at delivered_rate), ``delivery`` (peak, clipped, n_samples per utterance).  wav /
        wav_list / wav_i16 are then not returned -- the 16 kHz waveform stays on the device -- and want_int16 is ignored.  With ``flac`` the
        encoding must be "s16": ev_flac reads ev_deliver's int16 on the device at the delivered rate, a stream decodes to delivered_list[b].
        denoise: None, True, a strength, a dict of DenoiseConfig's fields or an emotivoice_amd.denoise.DenoiseConfig: ev_denoise runs FIRST, on the
        vocoder's waveform -- strength times the magnitude spectrum of the vocoder's answer to an all-zero mel (measured once per engine, or
        config.bias) is subtracted from every STFT cell -- so that loudness is measured on the audio that is delivered; the lengths do not change
        (a waveform of whole frames).  Alone it is the last stage: wav / wav_list hold its output, want_int16 and flac its clamped int16.
        ``denoise`` in the result holds lens_out and, with report=True, removed_db: per utterance the removed energy relative to the input
        (ev_compare on the two device waveforms).  The default strength 0.01 is an unmeasured starting value (emotivoice_amd.denoise)."""
        from .flac import FlacConfig
        sel = None
        if flac is not None and flac is not False:
            sel = np.ones(len(utts), bool) if flac is True or isinstance(flac, FlacConfig) else np.asarray(flac, bool)
            if sel.shape != (len(utts),):
                raise ValueError("flac: True or one entry per utterance (%d), got shape %s" % (len(utts), sel.shape))
        for name, given in (("flac", sel), ("limiter", limiter), ("loudness", loudness), ("delivery", delivery), ("denoise", denoise)):
            if given is not None and not vocoder:
                raise ValueError("%s needs the vocoder's waveform" % name)
        lc = None if loudness is None else loudness_config(loudness, int(self.shapes.sr))
        mc = None if limiter is None else limiter_config(limiter, int(self.shapes.sr))
        dc = delivery_config(delivery, int(self.shapes.sr))
        nc = denoise_config(denoise, int(self.shapes.sr))
        if dc is not None and sel is not None and dc.encoding != "s16":
            raise ValueError("flac needs delivery's encoding 's16', not %r" % dc.encoding)
        staged = lc is not None or mc is not None or dc is not None or nc is not None       # the audio is the last stage's: the synthesis makes no int16 and its waveform stays on the device
        flags = (_ffi.EV_FLAG_WANT_INT16 if want_int16 and not staged else 0) | (0 if vocoder else _ffi.EV_FLAG_NO_VOCODER)
        self._denoise_ready(nc)
        res, cu = self._synthesize_call(utts, alpha, flags, forced_durations, prosody)
        out = self.result_to_numpy(res, want_int16, skip_wav=staged)
        out["cu_seqlens"] = cu
        offs = out["mel_offsets"] * self.shapes.upsample_factor
        pcm_i16 = None
        if staged:
            audio, figures, limited, pcm_i16, dres = self._finish(res.wav, np.diff(offs), lc, mc, want_int16 or sel is not None, False, dc, nc)
            if nc is not None:      # whole frames in, whole frames out: every offset above still holds
                assert np.array_equal(audio["denoise"]["lens_out"], np.diff(offs)), "ev_denoise changed a length of whole frames"
                out["denoise"] = audio.pop("denoise")
            if dc is not None:
                out.update(audio)
            else:
                out["wav"], out["wav_list"] = audio["wav"], audio["wav_list"]
                if want_int16 or sel is not None:
                    out["wav_i16"], out["wav_int16_list"] = audio.get("wav_i16"), audio.get("wav_i16_list")
            if figures is not None:
                out["loudness"] = figures
            if limited is not None:
                out["limiter"] = limited
        if sel is not None and dc is not None:
            out["flac_list"] = self._flac_delivered(sel, dres, flac, dc.sample_rate, convert="wrap")
        elif sel is not None:
            out["flac_list"] = self._flac_runs(sel, offs, res.wav, pcm_i16, flac)
        return out

    def synthesize_long(self, documents: Sequence, alpha: float = 1.0, prosody=None, config=None, flac=None, loudness=None, limiter=None,
                        delivery=None, denoise=None) -> Dict[str, object]:
        """Documents of several sentences each -> one waveform per document and the time of every sentence in it.  documents: each a
        dict(utts=[utt dicts as ``synthesize`` takes], pauses=[one per joint: a class of emotivoice_amd.longform.pauses_ms, milliseconds, or
        None]) or a pair (utts, pauses); pauses None = "sentence" everywhere.  prosody: as ``synthesize`` takes it, over the sentences of all
        documents in order.  config: an emotivoice_amd.longform.StitchConfig (None: its defaults, which have not been measured on a released
        checkpoint).  One ev_synthesize[_prosody] call, one ev_stitch call on its device waveform and one D2H copy (int16 with
        config.want_int16, else fp32).  All sentences go into one synthesize call: more than it takes raises; splitting is the caller's.
        flac=True or an emotivoice_amd.flac.FlacConfig (its LPC / MD5 / block settings; the sample rate is the engine's; ``md5`` costs one serial
        chain per document) adds flac_list, one FLAC stream (``bytes``) per document, encoded on the device from ev_stitch's int16 documents (it turns
        config.want_int16 on, so ``documents`` are the int16 ones a stream decodes to).
        loudness: None, a target in LUFS or an emotivoice_amd.loudness.LoudnessConfig: every document is normalised on the device after ev_stitch
        (ev_loudness: one gain per document, so the balance between its sentences stays) and before ev_flac; ``documents`` (int16 by the
        clamping rule with config.want_int16) then hold the normalised audio and ``loudness`` the per-document figures.
        limiter: as ``synthesize`` takes it, per document: ev_limit after ev_stitch (and after ev_loudness's measurement when ``loudness`` is
        given, whose pre-gain it applies) and before ev_flac; ``documents`` hold the limited audio and ``limiter`` the per-document figures.
        delivery: as ``synthesize`` takes it, per document, after the last of those stages: ``documents`` is then delivered_list (at
        delivered_rate, in the delivery's encoding), ``delivery`` holds peak / clipped / n_samples, no 16 kHz audio is copied to the host,
        config.want_int16 is ignored and flac (encoding "s16" only) reads ev_deliver's int16 at the delivered rate.  sentence_times are in
        SECONDS and hold at any delivered rate; seg_pos / seg_start / seg_end / doc_lens and ``sample_rate`` stay on the engine's 16 kHz clock
        (delivered_rate is returned next to them).
        denoise: as ``synthesize`` takes it, per document: ev_denoise right after ev_stitch and before the other stages.  Its output has whole
        hops: a document whose length is no multiple of the hop (256) loses the up to 255 samples after its last whole hop, doc_lens then holds
        the new lengths and ``denoise`` lens_out (and removed_db with report=True)."""
        import dataclasses
        from .longform import StitchConfig, flatten_documents, plan_document
        sc = (config or StitchConfig()).validate()
        dc = delivery_config(delivery, int(self.shapes.sr))
        nc = denoise_config(denoise, int(self.shapes.sr))
        if dc is not None and flac and dc.encoding != "s16":
            raise ValueError("flac needs delivery's encoding 's16', not %r" % dc.encoding)
        if dc is not None and sc.want_int16:
            sc = dataclasses.replace(sc, want_int16=False).validate()
        if flac and not sc.want_int16 and dc is None:
            sc = dataclasses.replace(sc, want_int16=True).validate()
        if int(sc.sample_rate) != int(self.shapes.sr):
            raise ValueError("config.sample_rate %d is not the engine's %d" % (sc.sample_rate, self.shapes.sr))
        lc = None if loudness is None else loudness_config(loudness, int(sc.sample_rate))
        mc = None if limiter is None else limiter_config(limiter, int(sc.sample_rate))
        utts, seg_doc, pauses = flatten_documents(documents)
        S = len(utts)
        if S > 65535:
            raise ValueError("%d sentences exceed the 65535 segments of one ev_stitch call; split the documents over several calls" % S)
        seg_doc, pause_after = plan_document(seg_doc, pauses, sc.sample_rate)
        self._denoise_ready(nc)
        res, _ = self._synthesize_call(utts, alpha, 0, None, prosody)
        mel_offs = host_array(res.mel_offsets, S + 1, np.int64) * self.shapes.upsample_factor
        st = self.stitch_raw(S, res.wav, mel_offs[:-1], np.diff(mel_offs), seg_doc, pause_after, sc, _ffi.EV_FLAG_DEVICE_INPUTS)
        out = self.stitch_to_numpy(st, int16_only=sc.want_int16, skip_wav=lc is not None or mc is not None or dc is not None or nc is not None)
        stage = ("denoise" if nc is not None else "limiter" if mc is not None else "loudness" if lc is not None else "delivery" if dc is not None else
                 "flac" if flac else None)
        empty = [d for d in range(st.batch_docs) if out["doc_lens"][d] < 1]
        if empty and stage:
            raise ValueError("%s: document %d is empty after the cut" % (stage, empty[0]))
        audio, figures, limited, pcm_i16, dres = self._finish(st.wav, out["doc_lens"], lc, mc, sc.want_int16, sc.want_int16, dc, nc)
        if nc is not None:
            out["denoise"] = audio.pop("denoise")
            out["doc_lens"], out["doc_offsets"] = out["denoise"]["lens_out"], out["denoise"]["offsets"]
        if dc is not None:
            out.update(audio)
        for k, name in (("wav", "wav"), ("wav_list", "docs"), ("wav_i16", "wav_i16"), ("wav_i16_list", "docs_i16")):
            if k in audio:
                out[name] = audio[k]
        if figures is not None:
            out["loudness"] = figures
        if limited is not None:
            out["limiter"] = limited
        if flac and dc is not None:
            out["flac_list"] = self._flac_delivered([True] * st.batch_docs, dres, flac, dc.sample_rate)
        elif flac:
            fr = self.flac_raw(st.batch_docs, pcm_i16 or st.wav_i16, True, out["doc_lens"], self._flac_config(flac, int(sc.sample_rate)),
                               _ffi.EV_FLAG_DEVICE_INPUTS)
            out["flac_list"] = self.flac_to_numpy(fr)["streams"]
        sr = float(sc.sample_rate)
        start = out["seg_pos"] / sr
        end = (out["seg_pos"] + (out["seg_end"] - out["seg_start"])) / sr
        out["documents"] = out["delivered_list"] if dc is not None else out["docs_i16"] if sc.want_int16 else out["docs"]
        out["seg_doc"] = seg_doc
        out["sentence_times"] = [[(float(start[s]), float(end[s])) for s in np.nonzero(seg_doc == d)[0]] for d in range(st.batch_docs)]
        out["sample_rate"] = int(sc.sample_rate)
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
