"""Forced alignment helpers on top of ``EVEngine.align`` (ev_align, include/evhip.h).

``timestamps`` turns durations into per-phoneme times, ``prosody_from_alignment`` turns an alignment into per-token overrides for
``ev_synthesize_prosody`` (the values the reference's teacher-forced branch feeds as ds / ps / es, model_open_source.py:113-139), and
``transfer`` re-voices recordings: align them with their own conditioning, then synthesise the same phonemes with another speaker /
prompt and the recording's timing (and, optionally, its intonation and energy).  ``align_recordings`` / ``transfer_from_recordings`` start from
the waveforms: the mel and the energy track (ev_features) and, with ``pitch_stats``, the pitch track (ev_pitch) are computed on the device and
never leave it on the way into ev_align; with ``sample_rate`` / ``trim`` the waveform is first resampled and trimmed there too (ev_resample).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .prosody import MAX_DURATION, Prosody


def timestamps(durations, hop: int = 256, sr: int = 16000) -> List[Tuple[float, float]]:
    """(start_s, end_s) of every token of one utterance from its durations in mel frames (hop samples per frame at ``sr``)."""
    d = np.asarray(durations, np.int64).reshape(-1)
    if (d < 0).any():
        raise ValueError("durations must be >= 0")
    ends = np.cumsum(d)
    starts = ends - d
    f = float(hop) / float(sr)
    return [(float(a) * f, float(b) * f) for a, b in zip(starts, ends)]


def _split(aligned: Dict[str, object], key: str):
    cu = np.asarray(aligned["cu_seqlens"])
    v = aligned.get(key)
    if v is None:
        return None
    v = np.asarray(v)
    return [v[cu[b]:cu[b + 1]] for b in range(len(cu) - 1)]


def prosody_from_alignment(aligned: Dict[str, object], pitch: bool = True, energy: bool = True) -> List[Prosody]:
    """One Prosody per utterance of an ``EVEngine.align`` result: the aligned durations, and the per-token pitch / energy means where
    ``pitch`` / ``energy`` ask for them (an alignment made without frame tracks has none: asking for them is an error).  A duration above
    EV_PROSODY_MAX_DURATION is an error that names the utterance and token."""
    durs = _split(aligned, "durations")
    ps = _split(aligned, "pitch") if pitch else None
    es = _split(aligned, "energy") if energy else None
    if pitch and ps is None:
        raise ValueError("the alignment has no pitch: align with per-frame pitch tracks, or pass pitch=False")
    if energy and es is None:
        raise ValueError("the alignment has no energy: align with per-frame energy tracks, or pass energy=False")
    out = []
    for b, d in enumerate(durs):
        big = np.nonzero(d > MAX_DURATION)[0]
        if big.size:
            j = int(big[0])
            raise ValueError("utterance %d, token %d: aligned duration %d frames > EV_PROSODY_MAX_DURATION %d" % (b, j, int(d[j]), MAX_DURATION))
        out.append(Prosody(durations=np.asarray(d, np.int64), pitch=None if ps is None else np.asarray(ps[b], np.float32),
                           energy=None if es is None else np.asarray(es[b], np.float32)))
    return out


def transfer(engine, src_utts: Sequence[dict], mels: Sequence[np.ndarray], dst_utts: Sequence[dict],
             pitch_frames: Optional[Sequence[np.ndarray]] = None, energy_frames: Optional[Sequence[np.ndarray]] = None,
             pitch: bool = True, energy: bool = True, vocoder: bool = True) -> Dict[str, object]:
    """Re-voice recordings: align ``mels`` (one (n_mels, T_b) array per utterance) with the SOURCE conditioning of ``src_utts``, then
    synthesise ``dst_utts`` -- the same phonemes with the target speaker / style / content -- with the recording's durations, and its
    per-token pitch / energy where frame tracks are given and ``pitch`` / ``energy`` ask for them.  Utterance b of both lists must carry the
    same ``ling``.  Returns the synthesis result with the alignment under "alignment"."""
    if len(src_utts) != len(dst_utts):
        raise ValueError("%d source and %d target utterances" % (len(src_utts), len(dst_utts)))
    for b, (s, d) in enumerate(zip(src_utts, dst_utts)):
        if not np.array_equal(np.asarray(s["ling"], np.int64), np.asarray(d["ling"], np.int64)):
            raise ValueError("utterance %d: source and target phonemes (ling) differ" % b)
    aligned = engine.align(src_utts, mels, pitch=pitch_frames, energy=energy_frames)
    pros = prosody_from_alignment(aligned, pitch=pitch and pitch_frames is not None, energy=energy and energy_frames is not None)
    out = engine.synthesize(dst_utts, prosody=pros, vocoder=vocoder)
    out["alignment"] = aligned
    return out


def align_recordings(engine, utts: Sequence[dict], wavs: Sequence[np.ndarray], energy_stats=None, pitch_stats=None,
                     pitch_config=None, sample_rate: Optional[int] = None, trim: bool = False) -> Dict[str, object]:
    """Forced alignment of recordings given as waveforms (one 1-D int16 or floating array per utterance, at the feature setup's rate unless
    ``sample_rate`` says otherwise): ev_features, then
    ev_align with EV_FLAG_DEVICE_MEL -- the mel (and the energy track) go from one call into the other on the device.  energy_stats:
    (mean, std) of the checkpoint's energy normalisation; with it the result carries the per-token energy means, without it none.
    pitch_stats: (mean, std) in Hz of the checkpoint's pitch normalisation; with it ev_pitch runs on the same packed waveforms and its device
    track goes into ev_align, so the result carries the per-token pitch means (``pitch_config``: an emotivoice_amd.pitch.PitchConfig on the
    feature setup's hop, default its defaults); without it there is no pitch.  The track is YIN's, not the dio + stonemask track the
    checkpoint was trained on.  sample_rate: the recordings' rate; with a rate other than the feature setup's, or with ``trim`` (the
    reference's get_mel trim: cut below 0.5 % of the peak, 50 ms of zeros on each side), ev_resample runs first and its device waveform goes into
    ev_pitch / ev_features without leaving the device; the result then also carries ``resampled_lens`` and, per utterance, ``time_offset_s`` =
    (trim_start - trim_pad) / sr_out: add it to ``timestamps()`` to get times on the original recording's clock.  The resampler is this
    project's windowed sinc, not librosa's soxr.  Returns what ``EVEngine.align`` returns."""
    from . import _ffi
    from .engine_audio import cut, host_array
    from .features import frames_for, pack_wavs
    from .packing import pack_utts
    B = len(utts)
    if len(wavs) != B:
        raise ValueError("%d wavs for %d utterances" % (len(wavs), B))
    if engine.feature_config is None:
        engine.features_setup()
    fc = engine.feature_config
    if fc.n_mels != engine.shapes.n_mels:
        raise ValueError("the feature setup has %d mels, the model %d" % (fc.n_mels, engine.shapes.n_mels))
    resampled = None
    if sample_rate in (None, fc.sr) and not trim:
        flat, is16, lens = pack_wavs(wavs, fc.n_fft, fc.hop)
        wav_ptr, wav_flags = flat.ctypes.data, 0
    else:
        from .resample import ResampleConfig, pack_wavs as pack_any_rate, time_offset_s
        rc = ResampleConfig(sr_in=fc.sr if sample_rate is None else int(sample_rate), sr_out=fc.sr, trim=trim).validate()
        if engine.resample_config is None or engine.resample_config.key() != rc.key():
            engine.resample_setup(rc)
        flat, is16_in, lens_in = pack_any_rate(wavs, rc)
        rs = engine.resample_raw(B, flat.ctypes.data, is16_in, lens_in)
        lens = host_array(rs.wav_lens, B, np.int64)
        for b, n in enumerate(lens):
            if n < fc.n_fft // 2 + 1:
                raise ValueError("wavs[%d]: %d samples after resampling%s < n_fft / 2 + 1 = %d (reflect padding needs that many)"
                                 % (b, n, " and trimming" if trim else "", fc.n_fft // 2 + 1))
            if frames_for(int(n), fc.hop) > _ffi.EV_ALIGN_MAX_FRAMES:
                raise ValueError("wavs[%d]: %d frames > EV_ALIGN_MAX_FRAMES %d" % (b, frames_for(int(n), fc.hop), _ffi.EV_ALIGN_MAX_FRAMES))
        resampled = dict(resampled_lens=lens, time_offset_s=[time_offset_s(rs.trim_start[b], rc.pad() if trim else 0, fc.sr) for b in range(B)])
        wav_ptr, is16, wav_flags = rs.wav, False, _ffi.EV_FLAG_DEVICE_INPUTS
    mean, std = (0.0, 1.0) if energy_stats is None else (float(energy_stats[0]), float(energy_stats[1]))
    pitch_ptr = None
    if pitch_stats is not None:
        from .pitch import PitchConfig, check_stats
        pc = (pitch_config or PitchConfig(hop=fc.hop)).validate()
        if pc.hop != fc.hop:
            raise ValueError("the pitch config has hop %d, the feature setup %d: the two tracks must share the frame grid" % (pc.hop, fc.hop))
        pm, ps = check_stats(pitch_stats)
        pitch_ptr = engine.pitch_raw(B, wav_ptr, is16, lens, pm, ps, pc, flags=wav_flags).pitch
    feats = engine.features_raw(B, wav_ptr, is16, lens, mean, std, flags=wav_flags)
    mel_lens = host_array(feats.mel_lens, B, np.int32)
    ling, cu, spk, style, content = pack_utts(utts)
    res = engine.align_raw(B, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data, feats.mel, False, mel_lens,
                           pitch_ptr, feats.energy if energy_stats is not None else None, flags=_ffi.EV_FLAG_DEVICE_MEL)
    out = engine.align_to_numpy(res)
    out["cu_seqlens"] = cu
    out["durations_list"] = cut(out["durations"], cu)
    if resampled is not None:
        out.update(resampled)
    return out


def transfer_from_recordings(engine, src_utts: Sequence[dict], wavs: Sequence[np.ndarray], dst_utts: Sequence[dict], energy_stats=None,
                             energy: bool = True, vocoder: bool = True, pitch_stats=None, pitch: bool = True,
                             sample_rate: Optional[int] = None, trim: bool = False) -> Dict[str, object]:
    """The wav-in counterpart of ``transfer``: align the recordings (``align_recordings``), then synthesise ``dst_utts`` with their durations
    and, where ``energy_stats`` / ``pitch_stats`` are given and ``energy`` / ``pitch`` ask for it, their per-token energy / pitch (the pitch
    from ev_pitch's track).  Without ``pitch_stats``, or with ``pitch=False``, the pitch is the predictor's.  ``sample_rate`` / ``trim``: as
    ``align_recordings`` (ev_resample first)."""
    if len(src_utts) != len(dst_utts):
        raise ValueError("%d source and %d target utterances" % (len(src_utts), len(dst_utts)))
    for b, (s, d) in enumerate(zip(src_utts, dst_utts)):
        if not np.array_equal(np.asarray(s["ling"], np.int64), np.asarray(d["ling"], np.int64)):
            raise ValueError("utterance %d: source and target phonemes (ling) differ" % b)
    aligned = align_recordings(engine, src_utts, wavs, energy_stats=energy_stats, pitch_stats=pitch_stats if pitch else None,
                               sample_rate=sample_rate, trim=trim)
    pros = prosody_from_alignment(aligned, pitch=pitch and pitch_stats is not None, energy=energy and energy_stats is not None)
    out = engine.synthesize(dst_utts, prosody=pros, vocoder=vocoder)
    out["alignment"] = aligned
    return out
