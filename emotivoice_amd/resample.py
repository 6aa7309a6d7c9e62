"""Host side of the sample-rate conversion and trimming ``EVEngine.resample`` runs on the device (ev_resample, include/evhip.h): the filter
design, the limits, and the packing of the recordings.

The reference resamples a corpus with ``librosa.resample(y, orig_sr=sr, target_sr=16000)`` (data/*/src/step1_clean_raw_data.py) and trims in
``prompt_dataset.get_mel`` (cut what lies below 0.5 % of the peak, pad 50 ms of zeros on each side; ``trim = True`` in config/joint/config.py).
The resampler here is NOT librosa's (soxr): it is a polyphase Kaiser-windowed sinc, specified in include/evhip.h and restated by ``design``.
The trim restates the reference.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from ._ffi import EV_ALIGN_MAX_FRAMES as MAX_FRAMES
from ._ffi import EV_RESAMPLE_MAX_RATIO as MAX_RATIO
from ._ffi import EV_RESAMPLE_MAX_TAPS as MAX_TAPS

MAX_OUT = MAX_FRAMES * 256           # output samples per utterance, padding included


@dataclass
class ResampleConfig:
    """ev_resample_config.  ``taps`` (2 half + 1 values, h[-half .. half]) replaces the design; ``trim`` switches the reference's trim on with
    ``trim_frac`` and ``trim_pad`` zeros on each side (None: sr_out // 20, the reference's 50 ms)."""
    sr_in: int = 16000
    sr_out: int = 16000
    zeros: int = 16
    rolloff: float = 0.945
    beta: float = 9.0
    taps: Optional[np.ndarray] = None
    trim: bool = False
    trim_frac: float = 0.005
    trim_pad: Optional[int] = None

    def ratio(self) -> Tuple[int, int]:
        """(up, down) = (sr_out / g, sr_in / g), g = gcd(sr_in, sr_out)."""
        g = math.gcd(int(self.sr_in), int(self.sr_out))
        return int(self.sr_out) // g, int(self.sr_in) // g

    def pad(self) -> int:
        return int(self.sr_out) // 20 if self.trim_pad is None else int(self.trim_pad)

    def key(self) -> tuple:
        """What two configs must share to share a setup."""
        taps = None if self.taps is None else np.asarray(self.taps, np.float32).tobytes()
        return (int(self.sr_in), int(self.sr_out), int(self.zeros), float(self.rolloff), float(self.beta), taps, bool(self.trim),
                float(self.trim_frac), self.pad())

    def is_default_design(self) -> bool:
        return self.taps is None and (self.zeros, float(self.rolloff), float(self.beta)) == (16, 0.945, 9.0)

    def design(self) -> np.ndarray:
        """The taps in use, float32 (2 half + 1,): ``taps`` if given, else the prototype filter of include/evhip.h, designed in float64 and rounded
        once."""
        if self.taps is not None:
            return np.ascontiguousarray(self.taps, np.float32).reshape(-1)
        up, down = self.ratio()
        q = max(up, down)
        half = int(self.zeros) * q
        i = np.arange(-half, half + 1, dtype=np.float64)
        r = i / float(half)
        g = np.sinc(float(self.rolloff) * i / float(q)) * np.i0(float(self.beta) * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / np.i0(float(self.beta))
        return (float(up) * g / g.sum()).astype(np.float32)

    def half_len(self) -> int:
        if self.taps is not None:
            return (np.asarray(self.taps).size - 1) // 2
        return int(self.zeros) * max(self.ratio())

    def validate(self) -> "ResampleConfig":
        """The rejections of ev_resample_setup, with messages that name the field."""
        if self.sr_in < 1 or self.sr_out < 1:
            raise ValueError("sr_in %d / sr_out %d must be positive" % (self.sr_in, self.sr_out))
        up, down = self.ratio()
        if up > MAX_RATIO or down > MAX_RATIO:
            raise ValueError("sr_in %d -> sr_out %d is up %d / down %d; both must be <= EV_RESAMPLE_MAX_RATIO %d" % (self.sr_in, self.sr_out, up, down, MAX_RATIO))
        if self.taps is not None:
            t = np.asarray(self.taps)
            if t.ndim != 1 or t.size < 3 or t.size % 2 == 0:
                raise ValueError("taps: expected an odd number (2 half_len + 1, half_len >= 1) of values in one dimension, got shape %s" % (t.shape,))
            if t.size > MAX_TAPS:
                raise ValueError("taps: %d values > EV_RESAMPLE_MAX_TAPS %d" % (t.size, MAX_TAPS))
            if not np.isfinite(t.astype(np.float32)).all():
                raise ValueError("taps: every value must be finite")
        else:
            if not 1 <= int(self.zeros) <= 4096:
                raise ValueError("zeros %d outside [1, 4096]" % self.zeros)
            if 2 * self.half_len() + 1 > MAX_TAPS:
                raise ValueError("zeros %d gives %d taps > EV_RESAMPLE_MAX_TAPS %d" % (self.zeros, 2 * self.half_len() + 1, MAX_TAPS))
            if not (np.isfinite(self.rolloff) and 0.0 < self.rolloff <= 1.0):
                raise ValueError("rolloff %g outside (0, 1]" % self.rolloff)
            if not (np.isfinite(self.beta) and self.beta >= 0.0):
                raise ValueError("beta must be >= 0 and finite")
        if self.trim:
            f = float(np.float32(self.trim_frac))
            if not (np.isfinite(f) and 0.0 < f < 1.0):
                raise ValueError("trim_frac %g outside (0, 1)" % self.trim_frac)
            if self.pad() < 0:
                raise ValueError("trim_pad %d must be >= 0" % self.pad())
        return self

    def output_len(self, L: int) -> int:
        """n = ceil(L up / down): the samples an utterance of L gives before the trim."""
        up, down = self.ratio()
        return -((-int(L) * up) // down)


def phase_table(taps: np.ndarray, up: int) -> np.ndarray:
    """The kernel's phase-major table (up, R), R = (2 half / up + 1) | 1: row p = (m down) mod up holds h[i], i = p (mod up), from the largest
    i <= half downwards (the order k ascends in), zero-filled -- what ev_get_stage("resample_taps") returns."""
    h = np.asarray(taps, np.float32).reshape(-1)
    half = (h.size - 1) // 2
    R = ((2 * half) // up + 1) | 1
    out = np.zeros((up, R), np.float32)
    for p in range(up):
        i0 = half - (half - p) % up
        idx = np.arange(i0, -half - 1, -up)
        out[p, :idx.size] = h[half + idx]
    return out


def time_offset_s(trim_start: int, trim_pad: int, sr_out: int) -> float:
    """Seconds to add to a time on the trimmed waveform's clock to get the time in the original recording: output sample j is resampled sample
    trim_start - trim_pad + j."""
    return (int(trim_start) - int(trim_pad)) / float(sr_out)


def pack_wavs(wavs, config: Optional[ResampleConfig] = None):
    """Utterances back to back for ev_resample: (flat array, is_int16, lens int64).  All int16 or all floating (converted to float32); an empty
    utterance, or one whose output (with the trim's padding) exceeds EV_ALIGN_MAX_FRAMES * 256 samples, is an error that names the utterance."""
    from .packing import pack_segments
    if len(wavs) > 65535:
        raise ValueError("%d utterances > 65535 per call" % len(wavs))
    cfg = config or ResampleConfig()
    extra = 2 * cfg.pad() if cfg.trim else 0

    def limit(n):
        if cfg.output_len(n) + extra > MAX_OUT:
            return "%d output samples > EV_ALIGN_MAX_FRAMES * 256 = %d" % (cfg.output_len(n) + extra, MAX_OUT)

    return pack_segments(wavs, flatten=True, limit=limit)
