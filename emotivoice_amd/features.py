"""Host-side tables and shapes of the acoustic features ``EVEngine.features`` computes on the device (ev_features, include/evhip.h): the
mel spectrogram and frame energy the reference's training stack extracts (prompt_dataset.get_mel -> TacotronSTFT.mel_spectrogram with the
parameters of config/joint/config.py).  Nothing here runs per utterance: the filterbank and the window are built once and handed to
``ev_features_setup``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._ffi import EV_ALIGN_MAX_FRAMES as MAX_FRAMES
from ._ffi import EV_FEATURES_MAX_MELS as MAX_MELS
from ._ffi import EV_FEATURES_MAX_NFFT as MAX_NFFT
from ._ffi import EV_FEATURES_MAX_RUN as MAX_RUN


def _hz_to_mel(f):
    """Slaney's auditory-toolbox mel scale: linear (3 mels per 200 Hz) below 1 kHz, logarithmic above (27 mels per factor 6.4)."""
    f = np.asarray(f, np.float64)
    lin = f / (200.0 / 3.0)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * (200.0 / 3.0))


def mel_filterbank(sr: int = 16000, n_fft: int = 1024, n_mels: int = 80, fmin: float = 0.0, fmax: Optional[float] = 8000.0) -> np.ndarray:
    """(n_mels, n_fft // 2 + 1) float32 triangular filters on the Slaney mel scale with Slaney (area) normalisation: n_mels + 2 band edges
    equally spaced in mels between fmin and fmax, filter m rises from edge m to edge m + 1 and falls to edge m + 2 over the FFT bin
    frequencies, and is scaled by 2 / (edge[m + 2] - edge[m])."""
    if fmax is None:
        fmax = sr / 2.0
    if n_mels < 1 or n_fft < 2 or not (0.0 <= fmin < fmax <= sr / 2.0 + 1e-9):
        raise ValueError("mel_filterbank: need n_mels >= 1 and 0 <= fmin < fmax <= sr / 2")
    freqs = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    width = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    fb = np.zeros((n_mels, freqs.size), np.float64)
    for m in range(n_mels):
        lower = -ramps[m] / width[m]
        upper = ramps[m + 2] / width[m + 1]
        fb[m] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edges[m + 2] - edges[m]))
    return fb.astype(np.float32)


def hann_window(n: int) -> np.ndarray:
    """Periodic hann window (scipy.signal.get_window("hann", n, fftbins=True)) in float32: what ev_features_setup uses for window = NULL."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)).astype(np.float32)


def frames_for(n_samples: int, hop: int = 256) -> int:
    """Frames of an utterance of n_samples samples: the centred STFT's n_samples // hop + 1."""
    if n_samples < 0:
        raise ValueError("n_samples must be >= 0")
    return int(n_samples) // int(hop) + 1


@dataclass
class FeatureConfig:
    """The reference's values (config/joint/config.py).  ``window`` None = periodic hann; ``mel_basis`` None = mel_filterbank(...)."""
    sr: int = 16000
    n_fft: int = 1024
    hop: int = 256
    n_mels: int = 80
    fmin: float = 0.0
    fmax: Optional[float] = 8000.0
    mel_clip: float = 1e-5
    energy_floor: float = 1e-10
    window: Optional[np.ndarray] = None
    mel_basis: Optional[np.ndarray] = None

    @property
    def n_bins(self) -> int:
        return self.n_fft // 2 + 1

    def validate(self) -> "FeatureConfig":
        """The limits of the device kernel, with messages that name the field (ev_features_setup rejects the same)."""
        if self.n_fft < 128 or self.n_fft % 128 or self.n_fft > MAX_NFFT:
            raise ValueError("n_fft %d must be a multiple of 128 in [128, %d]" % (self.n_fft, MAX_NFFT))
        if not 1 <= self.n_mels <= MAX_MELS:
            raise ValueError("n_mels %d outside [1, %d]" % (self.n_mels, MAX_MELS))
        if self.hop < 8 or self.hop % 8 or self.hop > self.n_fft:
            raise ValueError("hop %d must be a multiple of 8 in [8, n_fft]" % self.hop)
        if 63 * self.hop + self.n_fft > MAX_RUN:
            raise ValueError("hop %d: the 63 hop + n_fft samples of a 64-frame tile exceed %d" % (self.hop, MAX_RUN))
        if not (self.mel_clip > 0 and np.isfinite(self.mel_clip)) or not (self.energy_floor >= 0 and np.isfinite(self.energy_floor)):
            raise ValueError("mel_clip must be positive and energy_floor >= 0, both finite")
        if self.window is not None and np.asarray(self.window).shape != (self.n_fft,):
            raise ValueError("window: expected (%d,), got %s" % (self.n_fft, np.asarray(self.window).shape))
        if self.mel_basis is not None and np.asarray(self.mel_basis).shape != (self.n_mels, self.n_bins):
            raise ValueError("mel_basis: expected (%d, %d), got %s" % (self.n_mels, self.n_bins, np.asarray(self.mel_basis).shape))
        return self

    def tables(self):
        """(mel_basis float32 (n_mels, n_bins), window float32 (n_fft,) or None), contiguous."""
        mb = self.mel_basis if self.mel_basis is not None else mel_filterbank(self.sr, self.n_fft, self.n_mels, self.fmin, self.fmax)
        win = None if self.window is None else np.ascontiguousarray(self.window, np.float32)
        return np.ascontiguousarray(mb, np.float32), win


def pack_wavs(wavs, n_fft: int = 1024, hop: int = 256, min_samples: Optional[int] = None):
    """Utterances back to back for ev_features: (flat array, is_int16, lens int64).  All int16 or all floating (converted to float32);
    too short (< n_fft // 2 + 1 samples) or too long (> MAX_FRAMES frames) utterances are errors that name the utterance.  ``min_samples``: another
    minimum length, for a call without reflect padding (ev_pitch: 1)."""
    from .packing import pack_segments

    def limit(n):
        if min_samples is None and n < n_fft // 2 + 1:
            return "%d samples < n_fft / 2 + 1 = %d (reflect padding needs that many)" % (n, n_fft // 2 + 1)
        if frames_for(n, hop) > MAX_FRAMES:
            return "%d frames > EV_ALIGN_MAX_FRAMES %d" % (frames_for(n, hop), MAX_FRAMES)

    return pack_segments(wavs, min_samples=min_samples or 0, flatten=True, limit=limit)
