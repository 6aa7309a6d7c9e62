"""True-peak metering and look-ahead limiting (ev_limit): the configuration of the device stage, its two host tables and the pre-gain rule.

The meter and the limiter are HIP (csrc/ev_limit.hip) behind the C entry ev_limit; include/evhip.h states them: a 4x polyphase interpolation (the
windowed sinc of ev_resample) gives the true peak, every sample above the ceiling asks for a gain, the gains are eroded over look-ahead + hold and
smoothed by a raised-cosine window, and the waveform is scaled by the result.  Nothing here touches the device.

The defaults (-1 dBTP, 5 ms of look-ahead, 50 ms of hold) are starting values; none has been measured on a released checkpoint.  The meter is not the
filter printed in BS.1770 annex 2 and under-reads near Nyquist (INTEGRATION.md has the table).
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from .loudness import SAMPLE_RATES, LoudnessConfig, gain_for

MAX_LOOKAHEAD, MAX_HOLD = 1024, 8192      # samples: EV_LIMIT_MAX_LOOKAHEAD, EV_LIMIT_MAX_HOLD


@dataclass
class LimiterConfig:
    sample_rate: int = 16000
    ceiling_dbtp: float = -1.0             # the true-peak ceiling, dB relative to full scale; <= 0
    lookahead_ms: float = 5.0
    hold_ms: float = 50.0
    want_int16: bool = False               # also the int16 output, clamped (ev_stitch's rule), never wrapped

    @property
    def ceiling(self) -> float:
        """The linear ceiling as the library rounds it."""
        return float(np.float32(10.0 ** (float(self.ceiling_dbtp) / 20.0)))

    def samples(self) -> Tuple[int, int]:
        """(lookahead, hold) in samples."""
        sr = int(self.sample_rate)
        return int(round(float(self.lookahead_ms) * sr / 1000.0)), int(round(float(self.hold_ms) * sr / 1000.0))

    def validate(self) -> "LimiterConfig":
        if isinstance(self.sample_rate, bool) or int(self.sample_rate) != self.sample_rate or int(self.sample_rate) not in SAMPLE_RATES:
            raise ValueError("sample_rate %r is not one of %s" % (self.sample_rate, SAMPLE_RATES))
        d = float(self.ceiling_dbtp)
        if not (math.isfinite(d) and d <= 0.0 and self.ceiling > 0.0):
            raise ValueError("ceiling_dbtp %r is not finite and <= 0 (a linear ceiling in (0, 1])" % (self.ceiling_dbtp,))
        for name, ms, cap in (("lookahead_ms", self.lookahead_ms, MAX_LOOKAHEAD), ("hold_ms", self.hold_ms, MAX_HOLD)):
            if not (math.isfinite(float(ms)) and float(ms) >= 0.0 and int(round(float(ms) * int(self.sample_rate) / 1000.0)) <= cap):
                raise ValueError("%s %r is not in [0, %d samples] at %d Hz" % (name, ms, cap, self.sample_rate))
        return self

    def to_struct(self):
        from . import _ffi
        c = _ffi.ev_limit_config()
        c.struct_size = C.sizeof(_ffi.ev_limit_config)
        c.sample_rate, c.ceiling, c.want_i16 = int(self.sample_rate), self.ceiling, 1 if self.want_int16 else 0
        c.lookahead, c.hold = self.samples()
        return c


def as_config(limiter, sample_rate: int, want_int16: bool = False) -> LimiterConfig:
    """The ``limiter=`` argument of EVEngine.synthesize / synthesize_long: True (the defaults), a ceiling in dBTP or a LimiterConfig -> a validated
    LimiterConfig at the engine's sample rate, with want_int16 turned on when the caller needs the int16 output."""
    import dataclasses
    if isinstance(limiter, LimiterConfig):
        lc = limiter
        if int(lc.sample_rate) != int(sample_rate):
            raise ValueError("limiter.sample_rate %d is not the engine's %d" % (lc.sample_rate, sample_rate))
    elif limiter is True:
        lc = LimiterConfig(sample_rate=int(sample_rate))
    elif isinstance(limiter, bool) or not isinstance(limiter, (int, float, np.integer, np.floating)):
        raise ValueError("limiter: None, True, a ceiling in dBTP or a LimiterConfig, not %r" % (limiter,))
    else:
        lc = LimiterConfig(sample_rate=int(sample_rate), ceiling_dbtp=float(limiter))
    if want_int16 and not lc.want_int16:
        lc = dataclasses.replace(lc, want_int16=True)
    return lc.validate()


def window(lookahead: int) -> np.ndarray:
    """ev_limit_design (host only): the lookahead + 1 fp32 taps of the smoothing window; their fp64 sum in ascending order is at most 1."""
    from . import _ffi
    L = int(lookahead)
    w = np.zeros(max(L, 0) + 1, np.float32)
    if _ffi.lib().ev_limit_design(L, w.ctypes.data_as(C.c_void_p)) != L + 1:
        raise ValueError("lookahead %r outside [0, %d]" % (lookahead, MAX_LOOKAHEAD))
    return w


def interpolator() -> np.ndarray:
    """The meter's 129 fp32 taps h[-64 .. 64]: ev_resample_design(1, 4, 16, 0.945, 9.0) (host only)."""
    from . import _ffi
    h = np.zeros(129, np.float32)
    if _ffi.lib().ev_resample_design(1, 4, 16, 0.945, 9.0, h.ctypes.data_as(C.c_void_p), 129) != 64:
        raise RuntimeError("ev_resample_design refused the meter's design")
    return h


def pre_gain(loudness: float, cfg: LoudnessConfig) -> Tuple[np.float32, int]:
    """Steps 1-3 of ev_loudness's gain rule, WITHOUT step 4 (the sample-peak limit): the pre-gain that goes into ev_limit, which holds the peak
    sample by sample instead.  The same operations and flags as emotivoice_amd.loudness.gain_for with a peak of 0: (gain, flags)."""
    return gain_for(loudness, 0.0, cfg)
