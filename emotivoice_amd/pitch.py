"""Host side of the pitch extraction ``EVEngine.pitch`` runs on the device (ev_pitch, include/evhip.h): the estimator's parameters and their
limits.  The estimator is YIN (a cumulative-mean-normalised difference function), not the dio + stonemask of pyworld the reference's training
stack uses (feats.Pitch); only the frame grid, the continuous fill of unvoiced frames and the standardisation restate the reference.

The statistics the track is standardised with belong to the checkpoint and are passed by the caller.  The reference's config
(config/joint/config.py: pitch_stats) has mean 225.089 Hz and std 53.78 Hz; that pair is kept here as ``PITCH_STATS`` for
documentation and is never a default.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from ._ffi import EV_PITCH_MAX_LDS as MAX_LDS
from ._ffi import EV_PITCH_MAX_WIN as MAX_WIN
from ._ffi import EV_PITCH_TILE_FRAMES as TILE_FRAMES

PITCH_STATS = (225.089, 53.78)


@dataclass
class PitchConfig:
    """ev_pitch_config with the defaults of ev_default_pitch_config (16 kHz, hop 256: config/joint/config.py)."""
    sample_rate: int = 16000
    hop: int = 256
    win: int = 1024
    f_min: float = 80.0
    f_max: float = 400.0
    threshold: float = 0.15
    silence_rms: float = 1e-3

    def tau_range(self) -> Tuple[int, int]:
        """(tau_min, tau_max) = (floor(sr / f_max), ceil(sr / f_min)), on the float32 values the C struct holds."""
        return (int(math.floor(self.sample_rate / float(np.float32(self.f_max)))),
                int(math.ceil(self.sample_rate / float(np.float32(self.f_min)))))

    def lds_bytes(self) -> int:
        """LDS of one tile of the kernel: its run of samples and three numbers per (frame, lag)."""
        tau_max = self.tau_range()[1]
        lags = (tau_max + 2 + 1) & ~1
        return TILE_FRAMES * lags * 12 + TILE_FRAMES * 4 + 4 * ((TILE_FRAMES - 1) * self.hop + self.win + tau_max + 1)

    def validate(self) -> "PitchConfig":
        """The rejections of ev_pitch, with messages that name the field."""
        if self.sample_rate < 1:
            raise ValueError("sample_rate %d must be positive" % self.sample_rate)
        if not 1 <= self.win <= MAX_WIN:
            raise ValueError("win %d outside [1, EV_PITCH_MAX_WIN %d]" % (self.win, MAX_WIN))
        if not 1 <= self.hop <= self.win:
            raise ValueError("hop %d outside [1, win %d]" % (self.hop, self.win))
        lo, hi = float(np.float32(self.f_min)), float(np.float32(self.f_max))
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi <= self.sample_rate / 4.0):
            raise ValueError("f_min %g / f_max %g must be finite with 0 < f_min < f_max <= sample_rate / 4" % (self.f_min, self.f_max))
        tau_min, tau_max = self.tau_range()
        if tau_max + 1 > self.win:
            raise ValueError("tau_max + 1 = %d > win %d (f_min %g is too low for the window)" % (tau_max + 1, self.win, self.f_min))
        if not 0.0 < float(np.float32(self.threshold)) <= 1.0:
            raise ValueError("threshold %g outside (0, 1]" % self.threshold)
        if not (np.isfinite(self.silence_rms) and self.silence_rms >= 0.0):
            raise ValueError("silence_rms must be >= 0 and finite")
        if self.win < 8 or not tau_min < tau_max or self.lds_bytes() > MAX_LDS:
            raise ValueError("win %d, hop %d, tau %d .. %d: the kernel needs win >= 8, tau_min < tau_max and a tile of %d bytes within "
                             "EV_PITCH_MAX_LDS %d" % (self.win, self.hop, tau_min, tau_max, self.lds_bytes(), MAX_LDS))
        return self


def check_stats(pitch_stats) -> Tuple[float, float]:
    mean, std = float(pitch_stats[0]), float(pitch_stats[1])
    if not np.isfinite(mean):
        raise ValueError("pitch_stats: pitch_mean must be finite")
    if not (np.isfinite(std) and std > 0):
        raise ValueError("pitch_stats: pitch_std must be positive and finite")
    return mean, std


def pack_wavs(wavs, hop: int = 256):
    """``features.pack_wavs``' packing rules with ev_pitch's own minimum length (one sample: there is no reflect padding here)."""
    from .features import pack_wavs as pack
    return pack(wavs, hop=hop, min_samples=1)
