"""Loudness normalisation (ev_loudness): the configuration of the device stage, the K-weighting coefficients and the host's gain rule.

The measurement itself is HIP (csrc/ev_loudness.hip) behind the C entry ev_loudness; include/evhip.h states it: ITU-R BS.1770 / EBU R 128
programme loudness (K-weighted, 400 ms blocks at a 100 ms step, absolute gate at -70 LUFS, relative gate 10 LU below the ungated level), the sample
peak (not the true peak), and one gain per segment limited by a largest boost and a peak ceiling.  Nothing here touches the device.

EXAMPLE_TARGET_LUFS and the default limits (20 dB of boost, a ceiling of -1 dBFS) are starting values; none has been measured on a released
checkpoint.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np

SAMPLE_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
EXAMPLE_TARGET_LUFS = -16.0
FLAG_UNDEFINED, FLAG_BOOST_LIMITED, FLAG_PEAK_LIMITED = 1, 2, 4
BLOCK_DROPPED_ABSOLUTE, BLOCK_DROPPED_RELATIVE, BLOCK_COUNTED = 0, 1, 2
DEFAULT_PEAK_CEILING = float(np.float32(10.0 ** (-1.0 / 20.0)))      # -1 dBFS, as the library rounds it


@dataclass
class LoudnessConfig:
    sample_rate: int = 16000
    target_lufs: float = float("nan")      # NaN: measure only
    max_gain_db: float = 20.0
    peak_ceiling: float = DEFAULT_PEAK_CEILING      # linear, on the sample peak
    want_int16: bool = False               # also the int16 output, clamped (ev_stitch's rule), never wrapped

    def validate(self) -> "LoudnessConfig":
        if isinstance(self.sample_rate, bool) or int(self.sample_rate) != self.sample_rate or int(self.sample_rate) not in SAMPLE_RATES:
            raise ValueError("sample_rate %r is not one of %s" % (self.sample_rate, SAMPLE_RATES))
        t = float(self.target_lufs)
        if not (math.isnan(t) or -70.0 <= t <= 0.0):
            raise ValueError("target_lufs %r is neither NaN (measure only) nor in [-70, 0]" % (self.target_lufs,))
        g = float(self.max_gain_db)
        if not (math.isfinite(g) and g >= 0.0):
            raise ValueError("max_gain_db %r is not finite and >= 0" % (self.max_gain_db,))
        p = float(np.float32(self.peak_ceiling))
        if not (0.0 < p <= 1.0):
            raise ValueError("peak_ceiling %r outside (0, 1]" % (self.peak_ceiling,))
        return self

    @property
    def measure_only(self) -> bool:
        return math.isnan(float(self.target_lufs))

    def to_struct(self):
        from . import _ffi
        c = _ffi.ev_loudness_config()
        c.struct_size = C.sizeof(_ffi.ev_loudness_config)
        c.sample_rate, c.target_lufs, c.max_gain_db = int(self.sample_rate), float(self.target_lufs), float(self.max_gain_db)
        c.peak_ceiling, c.want_i16 = float(self.peak_ceiling), 1 if self.want_int16 else 0
        return c


def as_config(loudness, sample_rate: int, want_int16: bool = False) -> LoudnessConfig:
    """The ``loudness=`` argument of EVEngine.synthesize / synthesize_long: a target in LUFS or a LoudnessConfig -> a validated LoudnessConfig at
    the engine's sample rate, with want_int16 turned on when the caller needs the int16 output."""
    import dataclasses
    if isinstance(loudness, LoudnessConfig):
        lc = loudness
        if int(lc.sample_rate) != int(sample_rate):
            raise ValueError("loudness.sample_rate %d is not the engine's %d" % (lc.sample_rate, sample_rate))
    elif isinstance(loudness, bool) or not isinstance(loudness, (int, float, np.integer, np.floating)):
        raise ValueError("loudness: None, a target in LUFS or a LoudnessConfig, not %r" % (loudness,))
    else:
        lc = LoudnessConfig(sample_rate=int(sample_rate), target_lufs=float(loudness))
    if lc.measure_only:
        raise ValueError("loudness: a target is needed to normalise (NaN measures only: EVEngine.loudness)")
    if want_int16 and not lc.want_int16:
        lc = dataclasses.replace(lc, want_int16=True)
    return lc.validate()


def k_weighting(sample_rate: int) -> Tuple[np.ndarray, np.ndarray]:
    """ev_loudness_design (host only): ((b, a) of the shelf, (b, a) of the high-pass) as two (2, 3) float64 arrays, a[0] = 1."""
    from . import _ffi
    co = (C.c_double * 10)()
    if _ffi.lib().ev_loudness_design(int(sample_rate), co) != 0:
        raise ValueError("sample_rate %r is not one of %s" % (sample_rate, SAMPLE_RATES))
    c = np.array(list(co), np.float64)
    return np.array([c[0:3], [1.0, c[3], c[4]]]), np.array([c[5:8], [1.0, c[8], c[9]]])


def gain_for(loudness: float, peak: float, cfg: LoudnessConfig) -> Tuple[np.float32, int]:
    """The host's gain rule of ev_loudness restated: (gain as the library rounds it, flags)."""
    cfg.validate()
    flags = FLAG_UNDEFINED if loudness == -math.inf else 0
    if cfg.measure_only:
        return np.float32(1.0), flags
    g = 1.0 if loudness == -math.inf else 10.0 ** ((float(cfg.target_lufs) - float(loudness)) / 20.0)
    gmax = 10.0 ** (float(cfg.max_gain_db) / 20.0)
    if g > gmax:
        g, flags = gmax, flags | FLAG_BOOST_LIMITED
    pk = float(np.float32(peak))
    if pk > 0.0:
        gpk = float(np.float32(cfg.peak_ceiling)) / pk
        if g > gpk:
            g, flags = gpk, flags | FLAG_PEAK_LIMITED
    return np.float32(g), flags
