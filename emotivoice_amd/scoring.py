"""Objective scores of synthesised speech against a reference signal, on the device (ev_score, include/evhip.h): mel-cepstral distortion along
the dynamic-time-warping path, F0 RMSE and bias in cents and the voiced / unvoiced error rate.

``score_recordings`` answers "how close is this checkpoint's rendering to a recording of the same sentence": synthesis, ev_features and ev_pitch
of the synthesis, ev_resample / ev_features / ev_pitch of the recordings and ev_score, with no waveform, mel or F0 track crossing to the host.
``score_engines`` puts two precision modes side by side on the same scores (durations forced equal, no warp): the 1e-3 of relative L2 of the
precision contract next to a figure in dB on the mel-cepstrum.

The MCD is an MFCC-style one on the engine's own log-mel (orthonormal DCT-II rows 1 .. n_ceps of the natural-log mel), NOT SPTK's warped
mel-cepstrum, and the F0 tracks are ev_pitch's YIN, not DIO: the figures compare among themselves only."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _ffi
from .engine_audio import host_array

PER_UTTERANCE = ("sum_dist", "path_len", "n_diag", "n_a", "n_b", "n_vv", "n_vu", "n_uv", "n_uu", "sum_c", "sum_c2", "mcd_db", "f0_rmse_cents",
                 "f0_bias_cents", "vuv_error", "warp", "lens_a", "lens_b", "nonfinite_a", "nonfinite_b")


@dataclass(frozen=True)
class ScoreConfig:
    n_ceps: int = 13          # cepstral coefficients c1 .. c13 (c0, the level, is left out)
    linear: bool = False      # no warp: the path is (k, k)

    def validate(self, n_mels: int = 80) -> "ScoreConfig":
        top = min(n_mels - 1, _ffi.EV_SCORE_MAX_CEPS)
        if not 1 <= int(self.n_ceps) <= top:
            raise ValueError("n_ceps = %r outside [1, %d]" % (self.n_ceps, top))
        return self


def corpus_means(res: Dict[str, object]) -> Dict[str, float]:
    """The corpus figures of a scored batch, every pair weighted by its path length K: mcd_db, vuv_error and warp are sums over the corpus
    divided by sum K; the F0 figures pool the sums over every voiced-voiced cell."""
    K = int(np.sum(res["path_len"]))
    n_vv = int(np.sum(res["n_vv"]))
    sum_c, sum_c2 = float(np.sum(res["sum_c"])), float(np.sum(res["sum_c2"]))
    return dict(pairs=int(len(res["path_len"])), path_len=K,
                mcd_db=(10.0 / math.log(10.0)) * math.sqrt(2.0) * (float(np.sum(res["sum_dist"])) / 65536.0) / K,
                f0_rmse_cents=math.sqrt(sum_c2 / n_vv) if n_vv else math.nan, f0_bias_cents=sum_c / n_vv if n_vv else math.nan,
                vuv_error=float(np.sum(res["n_vu"]) + np.sum(res["n_uv"])) / K, warp=float(np.sum(res["n_a"]) + np.sum(res["n_b"])) / K, n_vv=n_vv)


def _report(res: Dict[str, object]) -> Dict[str, object]:
    B = int(res["batch"])
    utts = [{k: (res[k][b].item()) for k in PER_UTTERANCE} for b in range(B)]
    return dict(utterances=utts, corpus=corpus_means(res), linear=bool(res["linear"]), n_ceps=int(res["n_ceps"]))


def _load_side(scorer, side: int, wav_ptr: int, wav_lens: np.ndarray, B: int, n_ceps: int, pitch_config) -> None:
    """ev_features and ev_pitch of a packed device waveform on ``scorer``, then ev_score_load of the two device results."""
    DEV = _ffi.EV_FLAG_DEVICE_INPUTS
    if scorer.feature_config is None:
        scorer.features_setup()
    fr = scorer.features_raw(B, wav_ptr, False, wav_lens, flags=DEV)
    pr = scorer.pitch_raw(B, wav_ptr, False, wav_lens, config=pitch_config, flags=DEV)
    lens = host_array(fr.mel_lens, B, np.int32)
    if not np.array_equal(lens, host_array(pr.mel_lens, B, np.int32)):
        raise ValueError("ev_features and ev_pitch disagree on the frame grid: the pitch config's hop must be the feature config's")
    scorer.score_load_raw(side, B, scorer.feature_config.n_mels, n_ceps, fr.mel, lens, pr.f0_hz, DEV)


def _wav_lens(engine, res) -> np.ndarray:
    return np.array([res.mel_lens[b] for b in range(res.batch)], np.int64) * engine.shapes.upsample_factor


def score_recordings(engine, utts: Sequence[dict], wavs: Sequence[np.ndarray], sample_rate: int = 16000, trim: bool = False, pitch_config=None,
                     config: Optional[ScoreConfig] = None) -> Dict[str, object]:
    """Synthesises ``utts`` on ``engine`` (weights loaded) and scores every utterance against its recording.  wavs: one 1-D array per utterance,
    all int16 or all floating, at ``sample_rate``; trim: cut leading and trailing silence off the recordings as the reference's get_mel does;
    pitch_config: an emotivoice_amd.pitch.PitchConfig (None: the library's default).  Returns ``utterances`` (one dict per utterance: the
    quantities of ev_score_result), ``corpus`` (corpus_means) and the settings."""
    from .resample import ResampleConfig, pack_wavs
    B = len(utts)
    if len(wavs) != B or not B:
        raise ValueError("%d recordings for %d utterances" % (len(wavs), B))
    sc = (config or ScoreConfig()).validate(engine.shapes.n_mels)
    res, _ = engine._synthesize_call(utts, 1.0, 0, None, None)
    _load_side(engine, 0, res.wav, _wav_lens(engine, res), B, sc.n_ceps, pitch_config)
    rc = ResampleConfig(sr_in=int(sample_rate), sr_out=engine.shapes.sr, trim=bool(trim)).validate()
    if engine.resample_config is None or engine.resample_config.key() != rc.key():
        engine.resample_setup(rc)
    flat, is16, lens = pack_wavs(wavs, rc)
    rr = engine.resample_raw(B, flat.ctypes.data, is16, lens)
    _load_side(engine, 1, rr.wav, host_array(rr.wav_lens, B, np.int64), B, sc.n_ceps, pitch_config)
    return _report(engine.score_to_numpy(engine.score_raw(sc.linear), with_paths=False))


def score_engines(engine_a, engine_b, utts: Sequence[dict], config: Optional[ScoreConfig] = None, pitch_config=None) -> Dict[str, object]:
    """The scores of engine_a's rendering (under test, e.g. "mx") against engine_b's (the yardstick, e.g. "strict") of the same utterances, both on
    one device with the same weights loaded.  engine_b synthesises with engine_a's durations forced (EV_FLAG_FORCED_DURATIONS, as the precision
    guard does), so the renderings have equal lengths and are scored without a warp.  Both waveforms go through engine_a's ev_features / ev_pitch /
    ev_score as device pointers."""
    sc = config or ScoreConfig(linear=True)
    sc.validate(engine_a.shapes.n_mels)
    B = len(utts)
    res_a, _ = engine_a._synthesize_call(utts, 1.0, 0, None, None)
    durations = engine_a.d2h(res_a.durations, (res_a.total_tokens,), np.int64)      # token-rate integers: what ev_set_forced_durations takes
    res_b, _ = engine_b._synthesize_call(utts, 1.0, 0, durations, None)
    lens_a, lens_b = _wav_lens(engine_a, res_a), _wav_lens(engine_b, res_b)
    if not np.array_equal(lens_a, lens_b):
        raise ValueError("forced durations did not give equal lengths: %s against %s samples" % (lens_a.tolist(), lens_b.tolist()))
    _load_side(engine_a, 0, res_a.wav, lens_a, B, sc.n_ceps, pitch_config)
    _load_side(engine_a, 1, res_b.wav, lens_b, B, sc.n_ceps, pitch_config)
    return _report(engine_a.score_to_numpy(engine_a.score_raw(sc.linear), with_paths=False))
