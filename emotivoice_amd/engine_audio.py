"""The audio utilities of the libevhip.so handle (csrc/ev_audio.cpp): ev_features, ev_pitch, ev_resample, ev_stitch, ev_compare, ev_flac,
ev_loudness, ev_limit, ev_deliver, ev_score, ev_denoise, ev_stretch and ev_watermark as ``*_setup`` / ``*_raw`` / ``*_to_numpy`` and a host-array call each.  EVEngine (engine.py) inherits them; the
handle, ``_check`` and ``d2h`` are its own."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _ffi
from .packing import pack_segments


def host_array(ptr, n: int, dtype) -> np.ndarray:
    """A copy of the ``n`` elements of a result struct's host array (it outlives the next call on the engine)."""
    n = int(n)
    return np.ctypeslib.as_array(ptr, (n,)).astype(dtype, copy=True) if n else np.empty(0, dtype)


def cut(flat: np.ndarray, offsets) -> List[np.ndarray]:
    """The segments of a packed array as views: flat[offsets[i]:offsets[i + 1]]."""
    return [flat[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


def offsets_of(lens) -> np.ndarray:
    """lens (B,) -> the (B + 1,) int64 offsets of their back-to-back packing."""
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)


def host_lens(lens, B: int, name: str = "lens") -> np.ndarray:
    """A per-segment host array as the library reads it: contiguous int64 with B entries."""
    ln = np.ascontiguousarray(lens, np.int64)
    if ln.size != B:
        raise ValueError("%s must have B = %d entries" % (name, B))
    return ln


def config_ref(config):
    """``config`` of a ``*_raw`` call -> what the library takes: a config object (validated, ``to_struct``), a struct or None -> byref or None."""
    c = config.validate().to_struct() if hasattr(config, "to_struct") else config
    return C.byref(c) if c is not None else None


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class EVAudio:
    """The utilities' methods of EVEngine.  Every call leaves its result struct in ``last_<utility>``; the struct's arrays stay valid until the
    next call of the same utility on this engine."""

    def __init__(self):
        self.feature_config = self.resample_config = self.delivery_config = self.denoise_config = None      # set by the ``*_setup`` calls
        self._setup_keys: Dict[str, tuple] = {}                   # "deliver" / "denoise" -> the key of the config the library is set up with
        self._denoise_own_bias: Dict[tuple, np.ndarray] = {}      # the vocoder's own bias per (n_fft, hop), measured by denoise_setup on the loaded weights
        for name in ("align", "features", "pitch", "resample", "stitch", "compare", "flac", "loudness", "limit", "deliver", "denoise", "stretch", "watermark", "watermark_detect"):
            setattr(self, "last_" + name, None)                # the ev_<name>_result of the last call (_call)

    def _setup_for(self, name: str, key: tuple, *args):
        """``<name>_setup(*args)`` unless the library is set up with ``key`` already: the output chain and the host-array calls of one engine share
        a setup, and set up again only when the key changed."""
        if self._setup_keys.get(name) != key:
            getattr(self, name + "_setup")(*args)

    def _weights_changed(self):
        """Other weights: the measured bias is the old vocoder's, and so is a denoise setup that may hold it."""
        self._denoise_own_bias.clear()
        self._setup_keys.pop("denoise", None)

    def _call(self, name: str, *args):
        """ev_<name>(handle, *args, &result): a fresh ev_<name>_result with its struct_size, the call, the error check, ``last_<name>``."""
        rt = getattr(_ffi, "ev_%s_result" % name)
        res = rt()
        res.struct_size = C.sizeof(rt)
        self._check(getattr(self._lib, "ev_" + name)(self._h, *args, C.byref(res)))
        setattr(self, "last_" + name, res)
        return res

    def _wav_pair(self, res, total: int, offsets, int16_only: bool, names=("wav_list", "wav_i16_list")) -> Dict[str, object]:
        """The D2H copies of a result's ``wav`` / ``wav_i16``: fp32 unless ``int16_only`` and the result has int16, int16 when it has it, each also
        cut by ``offsets`` under ``names``."""
        out: Dict[str, object] = {}
        if not (int16_only and res.wav_i16):
            out["wav"] = self.d2h(res.wav, (int(total),), np.float32)
            out[names[0]] = cut(out["wav"], offsets)
        if res.wav_i16:
            out["wav_i16"] = self.d2h(res.wav_i16, (int(total),), np.int16)
            out[names[1]] = cut(out["wav_i16"], offsets)
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
        return self._call("features", B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, _ptr(host_lens(wav_lens, B, "wav_lens")),
                          C.c_float(energy_mean), C.c_float(energy_std), flags)

    def features_to_numpy(self, res: _ffi.ev_features_result) -> Dict[str, object]:
        B, n_mels = res.batch, self.feature_config.n_mels
        mel_lens, offs = host_array(res.mel_lens, B, np.int32), host_array(res.mel_offsets, B + 1, np.int64)
        mel = self.d2h(res.mel, (res.total_frames * n_mels,), np.float32)
        energy = self.d2h(res.energy, (res.total_frames,), np.float32)
        return dict(mel_lens=mel_lens, mel_offsets=offs, energy=energy,
                    mel_list=[m.reshape(n_mels, t) for m, t in zip(cut(mel, offs * n_mels), mel_lens)], energy_list=cut(energy, offs))

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
        wl = host_lens(wav_lens, B, "wav_lens")
        c = None
        if config is not None:
            c = _ffi.ev_pitch_config()
            self._lib.ev_default_pitch_config(C.byref(c))
            c.sample_rate, c.hop, c.win = int(config.sample_rate), int(config.hop), int(config.win)
            c.f_min, c.f_max, c.threshold, c.silence_rms = config.f_min, config.f_max, config.threshold, config.silence_rms
        return self._call("pitch", B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, _ptr(wl), config_ref(c), C.c_float(pitch_mean),
                          C.c_float(pitch_std), flags)

    def pitch_to_numpy(self, res: _ffi.ev_pitch_result) -> Dict[str, object]:
        B, n = res.batch, res.total_frames
        mel_lens, offs = host_array(res.mel_lens, B, np.int32), host_array(res.mel_offsets, B + 1, np.int64)
        pitch, f0, ap = (self.d2h(ptr, (n,), np.float32) for ptr in (res.pitch, res.f0_hz, res.aperiodicity))
        return dict(mel_lens=mel_lens, mel_offsets=offs, pitch=pitch, pitch_list=cut(pitch, offs), f0_list=cut(f0, offs),
                    aperiodicity_list=cut(ap, offs))

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
        return self._call("resample", B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, _ptr(host_lens(wav_lens, B, "wav_lens")), flags)

    def resample_to_numpy(self, res: _ffi.ev_resample_result) -> Dict[str, object]:
        B = res.batch
        offs = host_array(res.wav_offsets, B + 1, np.int64)
        wav = self.d2h(res.wav, (res.total_samples,), np.float32)
        return dict(wav=wav, wav_list=cut(wav, offs), wav_lens=host_array(res.wav_lens, B, np.int64), wav_offsets=offs,
                    trim_start=host_array(res.trim_start, B, np.int64), trim_end=host_array(res.trim_end, B, np.int64))

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
        return self._call("stitch", S, C.c_void_p(wav_ptr), _ptr(so), _ptr(sl), _ptr(sd), _ptr(pa), config_ref(config), flags)

    def stitch_to_numpy(self, res: _ffi.ev_stitch_result, int16_only: bool = False, skip_wav: bool = False) -> Dict[str, object]:
        """One D2H copy of the fp32 documents (or, with ``int16_only`` and a result that has them, of the int16 ones only; without it both) and
        the host arrays of the result.  ``skip_wav``: the host arrays only."""
        D, S = res.batch_docs, res.batch_segs
        out: Dict[str, object] = dict(doc_lens=host_array(res.doc_lens, D, np.int64), doc_offsets=host_array(res.doc_offsets, D + 1, np.int64),
                                      seg_pos=host_array(res.seg_pos, S, np.int64), seg_start=host_array(res.seg_start, S, np.int64),
                                      seg_end=host_array(res.seg_end, S, np.int64), seg_peak=host_array(res.seg_peak, S, np.float32))
        if not skip_wav:
            out.update(self._wav_pair(res, res.total_samples, out["doc_offsets"], int16_only, ("docs", "docs_i16")))
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

    # -- signal comparison (ev_compare): how far a signal lies from a yardstick, per segment, on the device
    def compare_raw(self, B: int, a_ptr: int, b_ptr: int, lens: np.ndarray, flags: int = 0) -> _ffi.ev_compare_result:
        """ev_compare (include/evhip.h).  a_ptr (under test) and b_ptr (the yardstick) are host pointers, or device pointers with
        EV_FLAG_DEVICE_INPUTS -- of this engine or of another one on the same device; lens is a host array.  The returned struct's arrays
        are host memory and stay valid until the next compare call on this engine."""
        return self._call("compare", B, C.c_void_p(a_ptr), C.c_void_p(b_ptr), _ptr(host_lens(lens, B)), flags)

    def compare_to_numpy(self, res: _ffi.ev_compare_result) -> Dict[str, object]:
        """Copies of the result's host arrays (they outlive the next compare call)."""
        B = res.batch
        out: Dict[str, object] = dict(batch=B, total=int(res.total))
        for k, dt in (("sum_d", np.float64), ("sum_d2", np.float64), ("sum_y", np.float64), ("sum_y2", np.float64), ("rel_l2", np.float64),
                      ("rel_l2_ac", np.float64), ("max_abs_d", np.float32), ("argmax_d", np.int64), ("peak_y", np.float32), ("nonfinite", np.int64)):
            out[k] = host_array(getattr(res, k), B, dt)
        offs = out["chunk_offsets"] = host_array(res.chunk_offsets, B + 1, np.int64)
        out["chunk_d2"], out["chunk_y2"] = host_array(res.chunk_d2, offs[-1], np.float64), host_array(res.chunk_y2, offs[-1], np.float64)
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
        arrays stay valid until the next flac call on this engine.  A FlacConfig with LPC or MD5 (``to_ext()`` not None) goes to ev_flac_lpc."""
        ext = config.validate().to_ext() if hasattr(config, "to_ext") else None
        if ext is None:
            return self._call("flac", B, C.c_void_p(pcm_ptr), 1 if pcm_is_i16 else 0, _ptr(host_lens(lens, B)), config_ref(config), flags)
        res = _ffi.ev_flac_result()
        res.struct_size = C.sizeof(_ffi.ev_flac_result)
        self._check(self._lib.ev_flac_lpc(self._h, B, C.c_void_p(pcm_ptr), 1 if pcm_is_i16 else 0, _ptr(host_lens(lens, B)), config_ref(config), C.byref(ext),
                                          flags, C.byref(res)))
        self.last_flac = res
        return res

    def flac_to_numpy(self, res: _ffi.ev_flac_result) -> Dict[str, object]:
        """One D2H copy of total_bytes and copies of the result's host arrays.  streams: one ``bytes`` per segment; frame_kind / frame_porder:
        one uint8 array per segment (0 constant, 1 verbatim, 8 + o fixed, 32 + (o - 1) LPC; the partition order)."""
        B, NF = res.batch, int(res.total_frames)
        raw = self.d2h(res.bytes, (int(res.total_bytes),), np.uint8)
        offs, nfr = host_array(res.stream_offsets, B + 1, np.int64), host_array(res.stream_frames, B, np.int64)
        f0 = offsets_of(nfr)
        return dict(streams=[s.tobytes() for s in cut(raw, offs)], stream_offsets=offs, stream_frames=nfr,
                    frame_offsets=host_array(res.frame_offsets, NF + 1, np.int64), frame_kind=cut(host_array(res.frame_kind, NF, np.uint8), f0),
                    frame_porder=cut(host_array(res.frame_porder, NF, np.uint8), f0), total_bytes=int(res.total_bytes))

    def flac(self, pcm_list: Sequence[np.ndarray], **config) -> Dict[str, object]:
        """Host signals -> FLAC streams.  pcm_list: one 1-D array per segment, all int16 or all floating (converted on the device with
        config's ``convert`` rule); further keywords: the fields of emotivoice_amd.flac.FlacConfig.  Needs no weights."""
        from .flac import FlacConfig
        fc = FlacConfig(**config).validate()
        flat, is16, lens = pack_segments(pcm_list, "pcm_list", min_samples=0)
        return self.flac_to_numpy(self.flac_raw(len(lens), flat.ctypes.data, is16, lens, fc))

    # -- loudness normalisation (ev_loudness): BS.1770 programme loudness, one gain per segment and the scaled waveform, on the device
    def loudness_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, lens: np.ndarray, config=None, flags: int = 0) -> _ffi.ev_loudness_result:
        """ev_loudness (include/evhip.h).  wav_ptr is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS; lens is a host array.
        config: an emotivoice_amd.loudness.LoudnessConfig, an _ffi.ev_loudness_config or None (the library's default: 16 kHz, measure only).
        The returned struct's device waveforms and host arrays stay valid until the next loudness call on this engine."""
        ln = host_lens(lens, B)
        res = self._call("loudness", B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, _ptr(ln), config_ref(config), flags)
        res._lens = ln.copy()      # the packing of res.wav / res.wav_i16, for loudness_to_numpy
        return res

    def loudness_to_numpy(self, res: _ffi.ev_loudness_result, int16_only: bool = False, lens=None, skip_wav: bool = False) -> Dict[str, object]:
        """Copies of the result's host arrays and, unless the call only measured, one D2H copy of the fp32 output (with ``int16_only`` and a
        result that has it, of the int16 output only; without it both).  block_ms / block_state: one array per segment.  lens: the call's
        lens, which cut the output into wav_list / wav_i16_list (None: the ones loudness_raw kept with the struct).  ``skip_wav``: the host
        arrays only."""
        B = res.batch
        boffs = host_array(res.block_offsets, B + 1, np.int64)
        out: Dict[str, object] = dict(loudness=host_array(res.loudness, B, np.float64), rel_threshold=host_array(res.rel_threshold, B, np.float64),
                                      gain=host_array(res.gain, B, np.float32), peak=host_array(res.peak, B, np.float32),
                                      flags=host_array(res.flags, B, np.uint8), nonfinite=host_array(res.nonfinite, B, np.int64), block_offsets=boffs,
                                      block_ms=cut(host_array(res.block_ms, boffs[-1], np.float64), boffs),
                                      block_state=cut(host_array(res.block_state, boffs[-1], np.uint8), boffs))
        if res.wav and not skip_wav:
            out.update(self._wav_pair(res, res.total, offsets_of(res._lens if lens is None else lens), int16_only))
        return out

    def loudness(self, wavs: Sequence[np.ndarray], **config) -> Dict[str, object]:
        """Host signals -> their loudness and, with a target, the normalised signals.  wavs: one 1-D array per segment, all int16 or all
        floating, at any rate of the table (recordings as well as synthesis); further keywords: the fields of
        emotivoice_amd.loudness.LoudnessConfig (no target_lufs: measure only).  Needs no weights."""
        from .loudness import LoudnessConfig
        lc = LoudnessConfig(**config).validate()
        flat, is16, lens = pack_segments(wavs)
        return self.loudness_to_numpy(self.loudness_raw(len(lens), flat.ctypes.data, is16, lens, lc))

    # -- true-peak metering and limiting (ev_limit): a 4x true-peak meter, a gain per sample that holds the ceiling and the limited waveform, on the device
    def limit_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, lens: np.ndarray, gains=None, config=None, flags: int = 0) -> _ffi.ev_limit_result:
        """ev_limit (include/evhip.h).  wav_ptr is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS; lens and gains (None: all 1) are
        host arrays.  config: an emotivoice_amd.limiter.LimiterConfig, an _ffi.ev_limit_config or None (the library's default: 16 kHz, -1 dBTP, 80
        and 800 samples).  The returned struct's device waveforms and host arrays stay valid until the next limit call on this engine."""
        ln = host_lens(lens, B)
        gn = None
        if gains is not None:
            gn = np.ascontiguousarray(gains, np.float32)
            if gn.shape != (B,):
                raise ValueError("gains must have B = %d entries" % B)
        res = self._call("limit", B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, _ptr(ln), _ptr(gn) if gn is not None else None,
                         config_ref(config), flags)
        res._lens = ln.copy()      # the packing of res.wav / res.wav_i16, for limit_to_numpy
        return res

    def limit_to_numpy(self, res: _ffi.ev_limit_result, int16_only: bool = False, lens=None, skip_wav: bool = False) -> Dict[str, object]:
        """Copies of the result's host arrays and one D2H copy of the fp32 output (with ``int16_only`` and a result that has it, of the int16
        output only; without it both).  lens: the call's lens, which cut the output into wav_list / wav_i16_list (None: the ones limit_raw kept
        with the struct).  ``skip_wav``: the host arrays only."""
        out: Dict[str, object] = {k: host_array(getattr(res, k), res.batch, np.float32)
                                  for k in ("true_peak_in", "sample_peak_in", "true_peak_out", "sample_peak_out", "min_gain")}
        out["limited"], out["nonfinite"] = host_array(res.limited, res.batch, np.int64), host_array(res.nonfinite, res.batch, np.int64)
        if not skip_wav:
            out.update(self._wav_pair(res, res.total, offsets_of(res._lens if lens is None else lens), int16_only))
        return out

    def limit(self, wavs: Sequence[np.ndarray], gains=None, **config) -> Dict[str, object]:
        """Host signals -> their peaks and the limited signals.  wavs: one 1-D array per segment, all int16 or all floating, at any rate of the
        table; gains: one pre-gain per segment (None: 1); further keywords: the fields of emotivoice_amd.limiter.LimiterConfig.  Needs no weights."""
        from .limiter import LimiterConfig
        lc = LimiterConfig(**config).validate()
        flat, is16, lens = pack_segments(wavs)
        return self.limit_to_numpy(self.limit_raw(len(lens), flat.ctypes.data, is16, lens, gains, lc))

    # -- response delivery (ev_deliver): the waveform at the client's rate as fp32, int16 (optionally dithered), mu-law or A-law bytes, on the device
    def deliver_setup(self, config, sr_in: int = 16000):
        """ev_deliver_setup.  config: an emotivoice_amd.delivery.DeliveryConfig or a sample rate in Hz (int16 at that rate); sr_in: the rate of
        the waveforms that will go in.  The setup is ev_deliver's own: it leaves resample_setup's alone.  Needs no weights."""
        from .delivery import ENCODINGS, delivery_config
        dc = delivery_config(config, int(sr_in))
        if dc is None:
            raise ValueError("deliver_setup needs a DeliveryConfig or a sample rate")
        c = _ffi.ev_deliver_config()
        c.struct_size = C.sizeof(_ffi.ev_deliver_config)
        c.sr_in, c.sr_out, c.encoding, c.dither, c.seed = int(sr_in), int(dc.sample_rate), ENCODINGS[dc.encoding], 1 if dc.dither else 0, int(dc.seed)
        taps = None
        if dc.taps is not None:
            taps = np.ascontiguousarray(dc.taps, np.float32).reshape(-1)
            c.taps, c.half_len = taps.ctypes.data, (taps.size - 1) // 2
        self._check(self._lib.ev_deliver_setup(self._h, C.byref(c)))
        self.delivery_config, self._setup_keys["deliver"] = dc, dc.key(sr_in)

    def deliver_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, lens: np.ndarray, seeds=None, flags: int = 0) -> _ffi.ev_deliver_result:
        """ev_deliver (include/evhip.h).  wav_ptr is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS; lens and seeds (None: the
        config's seed for every utterance) are host arrays.  The returned struct's device bytes and host arrays stay valid until the next deliver
        call on this engine."""
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray(seeds, np.uint32)
            if sd.shape != (B,):
                raise ValueError("seeds must have B = %d entries" % B)
        return self._call("deliver", B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, _ptr(host_lens(lens, B)), _ptr(sd) if sd is not None else None, flags)

    def deliver_to_numpy(self, res: _ffi.ev_deliver_result, config=None) -> Dict[str, object]:
        """One D2H copy of total_bytes and copies of the result's host arrays.  delivered_list: one typed array per utterance (float32 / int16 /
        uint8 by the encoding of ``config``, default the last deliver_setup's); peak, clipped, n_samples, byte_offsets: per utterance."""
        dc = config or self.delivery_config
        B = res.batch
        raw = self.d2h(res.data, (int(res.total_bytes),), np.uint8)
        offs, n = host_array(res.byte_offsets, B + 1, np.int64), host_array(res.n_samples, B, np.int64)
        es = dc.sample_bytes
        return dict(delivered_list=[raw[int(o):int(o) + int(k) * es].view(dc.dtype) for o, k in zip(offs[:-1], n)], n_samples=n, byte_offsets=offs,
                    peak=host_array(res.peak, B, np.float32), clipped=host_array(res.clipped, B, np.int64), sample_rate=int(dc.sample_rate),
                    encoding=dc.encoding)

    def deliver(self, wavs: Sequence[np.ndarray], config, sample_rate: int = 16000, seeds=None) -> Dict[str, object]:
        """Host signals at ``sample_rate`` -> what a client asked for.  wavs: one 1-D array per utterance, all int16 or all floating; config: an
        emotivoice_amd.delivery.DeliveryConfig or a sample rate in Hz (int16 at that rate); seeds: one dither seed per utterance (None: the
        config's).  The filter is this project's polyphase windowed sinc (ev_resample's), not soxr.  Needs no weights."""
        from .delivery import delivery_config
        dc = delivery_config(config, int(sample_rate))
        if dc is None:
            raise ValueError("deliver needs a DeliveryConfig or a sample rate")
        self._setup_for("deliver", dc.key(sample_rate), dc, sample_rate)
        flat, is16, lens = pack_segments(wavs)
        return self.deliver_to_numpy(self.deliver_raw(len(lens), flat.ctypes.data, is16, lens, seeds), dc)

    # -- vocoder bias removal (ev_denoise): STFT, a gain per cell from the vocoder's zero-mel spectrum, inverse STFT, on the device
    def denoise_setup(self, config=None):
        """ev_denoise_setup.  config: an emotivoice_amd.denoise.DenoiseConfig (default: strength 0.01, 1024 / 256).  With config.bias None the
        engine measures its own vocoder's bias, which needs the weights and runs the vocoder once -- it replaces ``last`` and the waveform of the
        last synthesis, so it must not happen between a synthesis and the stages that read its device waveform; the measured bias is kept and
        passed back on later setups until other weights are loaded.  ``denoise_bias()`` reads it.  The setup is ev_denoise's own: it leaves
        features_setup's alone."""
        from .denoise import DenoiseConfig
        dc = (config or DenoiseConfig()).validate()
        c = _ffi.ev_denoise_config()
        self._lib.ev_default_denoise_config(C.byref(c))
        c.n_fft, c.hop, c.strength, c.want_i16 = int(dc.n_fft), int(dc.hop), float(dc.strength), 1 if dc.want_int16 else 0
        win = None if dc.window is None else np.ascontiguousarray(dc.window, np.float32)      # copied by the library; kept alive across the call
        c.window = win.ctypes.data if win is not None else None
        own, shape = self._denoise_own_bias, dc.tables_key()      # the bias measured on the loaded weights: measured once, then passed back
        bias = own.get(shape) if dc.bias is None else np.ascontiguousarray(dc.bias, np.float32)
        self._check(self._lib.ev_denoise_setup(self._h, C.byref(c), _ptr(bias) if bias is not None else None))
        self.denoise_config, self._setup_keys["denoise"] = dc, dc.key()
        if dc.bias is None and bias is None:
            own[shape] = self.denoise_bias()

    def denoise_bias(self) -> np.ndarray:
        """ev_denoise_bias: the (n_fft / 2 + 1,) float32 bias in use -- what to keep beside a checkpoint and pass back as DenoiseConfig.bias."""
        if self.denoise_config is None:
            raise ValueError("denoise_setup has not been called")
        out = np.empty(int(self.denoise_config.n_fft) // 2 + 1, np.float32)
        self._check(self._lib.ev_denoise_bias(self._h, _ptr(out)))
        return out

    def denoise_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, lens: np.ndarray, strengths=None, flags: int = 0) -> _ffi.ev_denoise_result:
        """ev_denoise (include/evhip.h).  wav_ptr is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS; lens and strengths (None: the
        config's strength for every utterance) are host arrays.  The returned struct's device waveforms and host arrays stay valid until the next
        denoise call on this engine."""
        st = None
        if strengths is not None:
            st = np.ascontiguousarray(strengths, np.float32)
            if st.shape != (B,):
                raise ValueError("strengths must have B = %d entries" % B)
        return self._call("denoise", B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, _ptr(host_lens(lens, B)), _ptr(st) if st is not None else None, flags)

    def denoise_to_numpy(self, res: _ffi.ev_denoise_result, int16_only: bool = False, skip_wav: bool = False) -> Dict[str, object]:
        """Copies of the result's host arrays and one D2H copy of the fp32 output (with ``int16_only`` and a result that has it, of the int16
        output only; without it both).  ``skip_wav``: the host arrays only."""
        B = res.batch
        out: Dict[str, object] = dict(lens_out=host_array(res.lens_out, B, np.int64), offsets=host_array(res.offsets, B + 1, np.int64))
        if not skip_wav:
            out.update(self._wav_pair(res, res.total, out["offsets"], int16_only))
        return out

    def denoise(self, wavs: Sequence[np.ndarray], config=None, strengths=None) -> Dict[str, object]:
        """Host signals -> the signals with the vocoder's bias removed.  wavs: one 1-D array per utterance, all int16 or all floating, each of
        n_fft / 2 + 1 samples or more; config: None, a strength or an emotivoice_amd.denoise.DenoiseConfig; strengths: one per utterance (None:
        the config's).  Every output has hop * (len // hop) samples."""
        from .denoise import DenoiseConfig, denoise_config
        dc = denoise_config(config) or DenoiseConfig().validate()
        self._setup_for("denoise", dc.key(), dc)
        flat, is16, lens = pack_segments(wavs, min_samples=int(dc.n_fft) // 2 + 1)
        return self.denoise_to_numpy(self.denoise_raw(len(lens), flat.ctypes.data, is16, lens, strengths))

    # -- time-scale modification (ev_stretch): WSOLA per segment, another length at the same pitch, on the device
    def stretch_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, lens: np.ndarray, lens_out: np.ndarray, config=None, flags: int = 0) -> _ffi.ev_stretch_result:
        """ev_stretch (include/evhip.h).  wav_ptr is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS; lens and lens_out (what
        emotivoice_amd.stretch.plan_lengths or ev_stretch_plan gives) are host arrays.  config: an emotivoice_amd.stretch.StretchConfig (only its
        want_int16 reaches the library), an _ffi.ev_stretch_config or None.  The returned struct's device arrays and host arrays stay valid until
        the next stretch call on this engine."""
        return self._call("stretch", B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, _ptr(host_lens(lens, B)), _ptr(host_lens(lens_out, B, "lens_out")),
                          config_ref(config), flags)

    def stretch_to_numpy(self, res: _ffi.ev_stretch_result, int16_only: bool = False, skip_wav: bool = False, want_track: bool = False) -> Dict[str, object]:
        """Copies of the result's host arrays and one D2H copy of the fp32 output (with ``int16_only`` and a result that has it, of the int16
        output only; without it both).  ``skip_wav``: the host arrays only.  ``want_track``: also deltas_list, one int16 array of lags per segment."""
        B = res.batch
        out: Dict[str, object] = dict(lens_out=host_array(res.lens_out, B, np.int64), offsets=host_array(res.offsets, B + 1, np.int64),
                                      frames=host_array(res.frames, B, np.int32), frame_offsets=host_array(res.frame_offsets, B + 1, np.int64),
                                      edge_frames=host_array(res.edge_frames, B, np.int32), sum_dist=host_array(res.sum_dist, B, np.uint64),
                                      nonfinite=host_array(res.nonfinite, B, np.int64))
        if want_track:
            out["deltas_list"] = cut(self.d2h(res.deltas, (int(out["frame_offsets"][-1]),), np.int16), out["frame_offsets"])
        if not skip_wav:
            out.update(self._wav_pair(res, res.total, out["offsets"], int16_only))
        return out

    def stretch(self, wavs: Sequence[np.ndarray], speed=None, seconds=None, samples=None, sample_rate: int = 16000, want_int16: bool = False,
                want_track: bool = False) -> Dict[str, object]:
        """Host signals -> the same signals at another length and the same pitch (WSOLA; not the reference's Rubber Band).  wavs: one 1-D array per
        segment, all int16 or all floating; speed, seconds, samples: the fields of emotivoice_amd.stretch.StretchConfig (a scalar or one entry
        per segment, at most one of the three per segment; none: speed 1); sample_rate turns seconds into samples and nothing else: the frame
        and the lag range are in samples.  Returns wav_list, lens_in, lens_out, speed (lens_in / lens_out) and the search's figures.  Needs no
        weights."""
        from .stretch import StretchConfig
        sc = StretchConfig(speed, seconds, samples, want_int16).validate()
        flat, is16, lens = pack_segments(wavs)
        out = self.stretch_to_numpy(self.stretch_raw(len(lens), flat.ctypes.data, is16, lens, sc.lengths(lens, sample_rate), sc), want_track=want_track)
        out["lens_in"] = np.asarray(lens, np.int64).copy()
        out["speed"] = out["lens_in"] / out["lens_out"]
        return out

    # -- audio watermark (ev_watermark, ev_watermark_detect): a keyed mark on the STFT magnitude and its detector, on the device
    def watermark_pattern(self, key: int, nbits: int = 0, payload: int = 0) -> np.ndarray:
        """ev_watermark_pattern: the 768 signs (int8, +1 / -1, payload flips applied) of the pattern, chip 48 u + v.  Host only."""
        signs = np.zeros(_ffi.EV_WATERMARK_CHIPS, np.int8)
        if self._lib.ev_watermark_pattern(C.c_uint32(int(key)), int(nbits), C.c_uint32(int(payload)), _ptr(signs)):
            raise ValueError("ev_watermark_pattern: nbits %r outside [0, %d] or payload %r does not fit" % (nbits, _ffi.EV_WATERMARK_MAX_BITS, payload))
        return signs

    def watermark_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, lens: np.ndarray, config, flags: int = 0) -> _ffi.ev_watermark_result:
        """ev_watermark (include/evhip.h).  wav_ptr is a host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS; lens is a host array.
        config: an emotivoice_amd.watermark.WatermarkConfig; its payload, nbits and strength_db go in per segment.  The returned struct's device
        waveforms and host arrays stay valid until the next watermark call on this engine."""
        payloads, nbits, strengths = config.validate().per_segment(B)
        return self._call("watermark", B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, _ptr(host_lens(lens, B)), config_ref(config), _ptr(payloads),
                          _ptr(nbits), _ptr(strengths), flags)

    watermark_to_numpy = denoise_to_numpy      # an ev_watermark_result has the fields of an ev_denoise_result

    def watermark(self, wavs: Sequence[np.ndarray], config) -> Dict[str, object]:
        """Host signals at 16 kHz -> the marked signals.  wavs: one 1-D array per segment, all int16 or all floating, each of 513 samples or more;
        config: a key, 'KEY[:PAYLOAD:NBITS]', a dict or an emotivoice_amd.watermark.WatermarkConfig.  Every output has 256 * (len // 256)
        samples.  Needs no weights."""
        from .watermark import N_FFT, watermark_config
        wc = watermark_config(config)
        if wc is None:
            raise ValueError("watermark needs a key or a WatermarkConfig")
        flat, is16, lens = pack_segments(wavs, min_samples=N_FFT // 2 + 1)
        return self.watermark_to_numpy(self.watermark_raw(len(lens), flat.ctypes.data, is16, lens, wc))

    def watermark_detect_raw(self, B: int, wav_ptr: int, wav_is_i16: bool, lens: np.ndarray, key: int, nbits: int = 0,
                             flags: int = 0) -> _ffi.ev_watermark_detect_result:
        """ev_watermark_detect (include/evhip.h).  The returned struct's host arrays and device q stay valid until the next detect call."""
        return self._call("watermark_detect", B, C.c_void_p(wav_ptr), 1 if wav_is_i16 else 0, _ptr(host_lens(lens, B)), C.c_uint32(int(key)), int(nbits), flags)

    def watermark_detect_to_numpy(self, res: _ffi.ev_watermark_detect_result, want_q: bool = False) -> Dict[str, object]:
        """The detector's integers per segment: offset, C, n (B,), bit_C, bit_n (B, 16), frames.  ``want_q``: also q_list, one (T_b, 48) int32
        array per segment (a D2H copy)."""
        B, nb = res.batch, _ffi.EV_WATERMARK_MAX_BITS
        out: Dict[str, object] = dict(offset=host_array(res.offset, B, np.int32), C=host_array(res.C, B, np.int32), n=host_array(res.n, B, np.int32),
                                      bit_C=host_array(res.bit_C, B * nb, np.int32).reshape(B, nb), bit_n=host_array(res.bit_n, B * nb, np.int32).reshape(B, nb),
                                      frames=host_array(res.frames, B, np.int32), frame_offsets=host_array(res.frame_offsets, B + 1, np.int64))
        if want_q:
            nbands = _ffi.EV_WATERMARK_BANDS
            q = self.d2h(res.q, (int(out["frame_offsets"][-1]) * nbands,), np.int32)
            out["q_list"] = [a.reshape(-1, nbands) for a in cut(q, out["frame_offsets"] * nbands)]
        return out

    def watermark_detect(self, wavs: Sequence[np.ndarray], key: int, nbits: int = 0, sample_rate: int = 16000, threshold: Optional[float] = None,
                         want_q: bool = False) -> Dict[str, object]:
        """Host signals -> is the mark of ``key`` in them?  wavs: one 1-D array per segment, all int16 or all floating; sample_rate: theirs -- at
        another rate than 16 kHz (one of ev_resample's) they are brought to 16 kHz by ev_resample on the device first.  Returns the detector's
        integers and ``report``: per segment dict(z, present, offset, bits, payload) (emotivoice_amd.watermark.detect_report; threshold None:
        6.25).  Needs no weights."""
        from .watermark import N_FFT, SAMPLE_RATE, THRESHOLD, detect_report
        if int(sample_rate) == SAMPLE_RATE:
            flat, is16, lens = pack_segments(wavs, min_samples=N_FFT // 2 + 1)
            res = self.watermark_detect_raw(len(lens), flat.ctypes.data, is16, lens, key, nbits)
        else:
            from .resample import ResampleConfig, pack_wavs
            rc = ResampleConfig(sr_in=int(sample_rate), sr_out=SAMPLE_RATE).validate()
            if self.resample_config is None or self.resample_config.key() != rc.key():
                self.resample_setup(rc)
            flat, is16, lens = pack_wavs(wavs, rc)
            rs = self.resample_raw(len(wavs), flat.ctypes.data, is16, lens)
            res = self.watermark_detect_raw(rs.batch, rs.wav, False, host_array(rs.wav_lens, rs.batch, np.int64), key, nbits, _ffi.EV_FLAG_DEVICE_INPUTS)
        out = self.watermark_detect_to_numpy(res, want_q)
        out["report"] = detect_report(out, int(nbits), THRESHOLD if threshold is None else float(threshold))
        return out

    # -- objective scoring (ev_score): MCD, F0 error and voiced / unvoiced error of a signal against a yardstick of another length, on the device
    def score_load_raw(self, side: int, B: int, n_mels: int, n_ceps: int, mel_ptr: int, lens: np.ndarray, f0_ptr: int = 0, flags: int = 0) -> None:
        """ev_score_load (include/evhip.h): side 0 = a (under test), 1 = b (the yardstick).  mel_ptr ((n_mels, T_b) per signal, back to back) and
        f0_ptr (Hz, 0 = none) are host pointers, or device pointers with EV_FLAG_DEVICE_INPUTS -- an ev_features_result.mel and an
        ev_pitch_result.f0_hz go straight in; lens is a host array of frames.  The side stays loaded until it is replaced."""
        ln = np.ascontiguousarray(lens, np.int32)
        if ln.size < B:          # the library reads B entries; it rejects B < 1 itself
            raise ValueError("lens must have B = %d entries" % B)
        self._check(self._lib.ev_score_load(self._h, int(side), B, int(n_mels), int(n_ceps), C.c_void_p(mel_ptr), _ptr(ln),
                                            C.c_void_p(f0_ptr) if f0_ptr else None, flags))

    def score_raw(self, linear: bool = False) -> _ffi.ev_score_result:
        """ev_score on the two loaded sides.  The returned struct's device arrays and host arrays stay valid until the next score call on this engine."""
        return self._call("score", _ffi.EV_SCORE_LINEAR if linear else 0)

    def score_to_numpy(self, res: _ffi.ev_score_result, with_paths: bool = True, with_cq: bool = False) -> Dict[str, object]:
        """Copies of the result's host arrays; with ``with_paths`` one D2H copy of each path array (path_list: one (K_b, 2) int32 array per pair, the
        frame of a and the frame of b); with ``with_cq`` the integer cepstra of both sides (cq_a_list / cq_b_list: (T_b, n_ceps) each)."""
        B, D = res.batch, res.n_ceps
        out: Dict[str, object] = dict(batch=B, n_ceps=D, linear=bool(res.linear), sum_dist=host_array(res.sum_dist, B, np.int64))
        for k in _ffi.SCORE_INT_FIELDS + ("lens_a", "lens_b", "nonfinite_a", "nonfinite_b"):
            out[k] = host_array(getattr(res, k), B, np.int32)
        for k in _ffi.SCORE_FLOAT_FIELDS:
            out[k] = host_array(getattr(res, k), B, np.float64)
        offs = out["path_offsets"] = host_array(res.path_offsets, B + 1, np.int64)
        if with_paths:
            pa, pb = self.d2h(res.path_a, (int(offs[-1]),), np.int32), self.d2h(res.path_b, (int(offs[-1]),), np.int32)
            out["path_list"] = [np.stack([x, y], 1) for x, y in zip(cut(pa, offs), cut(pb, offs))]
        if with_cq:
            for side, total, lens in (("a", res.total_frames_a, out["lens_a"]), ("b", res.total_frames_b, out["lens_b"])):
                cq = self.d2h(getattr(res, "cq_" + side), (int(total) * D,), np.int32)
                out["cq_%s_list" % side] = [c.reshape(-1, D) for c in cut(cq, offsets_of(lens) * D)]
        return out

    def score_load(self, side: int, feats: Sequence[np.ndarray], f0=None, n_ceps: int = 13) -> None:
        """Host arrays into one side: feats, one (n_mels, T_b) natural-log mel per signal (what features() returns); f0: one (T_b,) track in Hz per
        signal (0 or non-finite = unvoiced, what pitch() returns as f0_list) or None."""
        if not len(feats):
            raise ValueError("feats must hold at least one signal")
        mels = [np.asarray(m, np.float32) for m in feats]
        n_mels = mels[0].shape[0]
        if any(m.ndim != 2 or m.shape[0] != n_mels for m in mels):
            raise ValueError("every entry of feats must be (n_mels, T) with the same n_mels")
        lens = np.array([m.shape[1] for m in mels], np.int32)
        flat = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in mels]))
        f0_flat = None
        if f0 is not None:
            if len(f0) != len(mels) or any(np.asarray(t).shape != (n,) for t, n in zip(f0, lens)):
                raise ValueError("f0 must hold one (T_b,) track per signal")
            f0_flat = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float32) for t in f0]))
        self.score_load_raw(side, len(mels), n_mels, n_ceps, flat.ctypes.data, lens, f0_flat.ctypes.data if f0_flat is not None else 0)

    def score(self, feats_a: Sequence[np.ndarray], feats_b: Sequence[np.ndarray], f0_a=None, f0_b=None, linear: bool = False, n_ceps: int = 13,
              with_cq: bool = False) -> Dict[str, object]:
        """Host features of a (under test) against b (the yardstick), pair by pair: mel-cepstral distortion along the DTW path (``linear``: along
        (k, k)), and with both F0 tracks the F0 error in cents and the voiced / unvoiced error rate.  Returns per-pair numpy arrays (sum_dist,
        path_len, n_diag, n_a, n_b, n_vv, n_vu, n_uv, n_uu, sum_c, sum_c2, mcd_db, f0_rmse_cents, f0_bias_cents, vuv_error, warp, nonfinite_a,
        nonfinite_b) and path_list.  An MFCC-style MCD on the engine's own log-mel: the figures compare among themselves only.  Needs no weights."""
        self.score_load(0, feats_a, f0_a, n_ceps)
        self.score_load(1, feats_b, f0_b, n_ceps)
        return self.score_to_numpy(self.score_raw(linear), with_cq=with_cq)
