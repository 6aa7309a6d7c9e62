"""Time-scale modification (ev_stretch): the configuration of the device stage and its host rule for the lengths.

The stage is HIP (csrc/ev_stretch.hip) behind the C entry ev_stretch; include/evhip.h states it: WSOLA (waveform-similarity overlap-add) with a
squared-difference search on 12-bit samples, frames of 512 samples, a hop of 256 and lags of -128 .. 127, whatever the sample rate.  It changes the
length of a finished waveform and keeps its pitch.  Nothing here touches the device.

Not verified: this is not Rubber Band (the reference's pyrb.time_stretch is a phase vocoder with transient handling); nobody has listened to it; it
was compared to no other stretcher; the frame, the hop and the lag range are unmeasured starting values chosen for 16 kHz speech.  A segment's last
896 / r + 256 output samples (r = L_in / L_out) read the zero extension, so the search there is against silence.  Ratios beyond [0.5, 2] are
refused.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

FRAME, HOP, LAGS = 512, 256, 256      # EV_STRETCH_FRAME, EV_STRETCH_HOP, EV_STRETCH_LAGS
MAX_SAMPLES = 1 << 30                 # EV_STRETCH_MAX_SAMPLES
MIN_ALPHA, MAX_ALPHA = 0.5, 2.0       # what synthesize_fit asks of the model's duration scale before the stretch closes the rest

_FIELDS = ("speed", "seconds", "samples")


def _is_number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


@dataclass
class StretchConfig:
    """How long every segment becomes.  speed (> 0: 2 halves the duration, as the reference's ``speed``), seconds or samples: each None, a scalar
    for every segment or a sequence with one entry per segment (entries may be None).  A segment may have at most one of the three; none means
    speed 1, the identity."""
    speed: object = None
    seconds: object = None
    samples: object = None
    want_int16: bool = False               # also the int16 output, clamped (ev_loudness' rule), never wrapped

    def validate(self) -> "StretchConfig":
        scalars = 0
        for name in _FIELDS:
            v = getattr(self, name)
            if v is None:
                continue
            entries = [v] if _is_number(v) else list(v) if isinstance(v, (list, tuple, np.ndarray)) else None
            if entries is None:
                raise ValueError("%s: None, a number or one entry per segment, not %r" % (name, v))
            scalars += _is_number(v)
            for b, e in enumerate(entries):
                if e is not None:
                    _check_entry(name, e, b if not _is_number(v) else None)
        if scalars > 1:
            raise ValueError("only one of speed, seconds and samples may be given for a segment")
        return self

    def per_segment(self, B: int, sample_rate: int) -> Tuple[List[Optional[float]], List[Optional[int]]]:
        """(speeds, targets) with B entries each: a segment has a speed, a target in samples (seconds: round(seconds * sample_rate), ties to
        even) or neither."""
        self.validate()
        cols = {}
        for name in _FIELDS:
            v = getattr(self, name)
            col = [None] * B if v is None else [v] * B if _is_number(v) else list(v)
            if len(col) != B:
                raise ValueError("%s: one entry per segment (%d), got %d" % (name, B, len(col)))
            cols[name] = col
        speeds: List[Optional[float]] = [None] * B
        targets: List[Optional[int]] = [None] * B
        for b in range(B):
            given = [n for n in _FIELDS if cols[n][b] is not None]
            if len(given) > 1:
                raise ValueError("segment %d: only one of %s may be given" % (b, ", ".join(given)))
            if given == ["speed"]:
                speeds[b] = float(cols["speed"][b])
            elif given == ["seconds"]:
                targets[b] = int(round(float(cols["seconds"][b]) * int(sample_rate)))
            elif given == ["samples"]:
                targets[b] = int(cols["samples"][b])
        return speeds, targets

    def lengths(self, lens, sample_rate: int = 16000) -> np.ndarray:
        """lens (B,) -> lens_out (B,) int64 by the host rule (plan_lengths); ValueError names the segment."""
        speeds, targets = self.per_segment(len(lens), sample_rate)
        return plan_lengths(lens, speeds, targets)

    def to_struct(self):
        from . import _ffi
        c = _ffi.ev_stretch_config()
        c.struct_size = C.sizeof(_ffi.ev_stretch_config)
        c.want_int16 = 1 if self.want_int16 else 0
        return c


def _check_entry(name: str, e, b: Optional[int]) -> None:
    where = name if b is None else "%s[%d]" % (name, b)
    if not _is_number(e):
        raise ValueError("%s = %r is not a number" % (where, e))
    if name == "samples":
        if int(e) != e or int(e) < 1:
            raise ValueError("%s = %r is not a whole number of samples >= 1" % (where, e))
    elif not (math.isfinite(float(e)) and float(e) > 0.0):
        raise ValueError("%s = %r is not finite and > 0" % (where, e))


def stretch_config(x, sr: int = 16000) -> Optional[StretchConfig]:
    """The ``stretch=`` argument of EVEngine.synthesize / synthesize_long: None, a speed, one speed per segment or a StretchConfig -> a validated
    StretchConfig or None.  ``sr`` is accepted for symmetry with the other stages: seconds become samples once the lengths are known."""
    if x is None or x is False:
        return None
    if isinstance(x, StretchConfig):
        return x.validate()
    if _is_number(x) or isinstance(x, (list, tuple, np.ndarray)):
        return StretchConfig(speed=x if _is_number(x) else list(x)).validate()
    raise ValueError("stretch: None, a speed, one speed per segment or a StretchConfig, not %r" % (x,))


def check_lengths(b: int, L_in: int, L_out: int) -> None:
    """The rules of ev_stretch's step 1 on one segment, in the library's order; ValueError names the segment."""
    if L_in < 1:
        raise ValueError("lens[%d] = %d < 1" % (b, L_in))
    if L_out < 1:
        raise ValueError("lens_out[%d] = %d < 1" % (b, L_out))
    if L_in > MAX_SAMPLES:
        raise ValueError("lens[%d] = %d > EV_STRETCH_MAX_SAMPLES = %d" % (b, L_in, MAX_SAMPLES))
    if L_out > MAX_SAMPLES:
        raise ValueError("lens_out[%d] = %d > EV_STRETCH_MAX_SAMPLES = %d" % (b, L_out, MAX_SAMPLES))
    if min(L_in, L_out) >= FRAME and (L_in > 2 * L_out or L_out > 2 * L_in):
        raise ValueError("segment %d: %d -> %d samples lies outside the ratios [0.5, 2]" % (b, L_in, L_out))


def plan_lengths(lens, speeds: Optional[Sequence] = None, targets: Optional[Sequence] = None) -> np.ndarray:
    """ev_stretch_plan restated on the host: lens (B,) -> lens_out (B,) int64.  Segment b takes targets[b] where that is given (not None), else
    max(1, rint(lens[b] / speeds[b])) in float64 with ties to even (speed None: 1.0).  ValueError where the library rejects."""
    ln = [int(v) for v in np.asarray(lens).reshape(-1)]
    B = len(ln)
    out = np.zeros(B, np.int64)
    for b in range(B):
        t = None if targets is None else targets[b]
        if t is not None:
            L_out = int(t)
        else:
            s = 1.0 if speeds is None or speeds[b] is None else float(speeds[b])
            if not (math.isfinite(s) and s > 0.0):
                raise ValueError("speeds[%d] = %r is not finite and > 0" % (b, s))
            v = float(np.rint(np.float64(ln[b]) / np.float64(s)))
            L_out = 2 ** 63 - 1 if v >= 4e18 else max(1, int(v))
        check_lengths(b, ln[b], L_out)
        out[b] = L_out
    return out


def fit_alpha(natural_samples: int, target_samples: int) -> float:
    """synthesize_fit's duration scale for one utterance: target / natural, clamped to [0.5, 2].  The model's durations are whole frames and its
    own predictions, so the result only comes close; the stretch closes the rest."""
    return float(min(MAX_ALPHA, max(MIN_ALPHA, float(target_samples) / float(natural_samples))))
