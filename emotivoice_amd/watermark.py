"""Audio watermark (ev_watermark, ev_watermark_detect): the configuration of the device stage and the host's reading of the detector's integers.

The stage is HIP (csrc/ev_watermark.hip) behind the C entries ev_watermark / ev_watermark_detect; include/evhip.h states the scheme: ev_denoise's
STFT -> gain -> inverse STFT with the gain of a keyed +-1 chip per (time tile, band) -- a or 1 / a, a = 10^(strength_db / 20) -- in 48 bands of 4
bins from 312.5 Hz to 3.3 kHz, tiles of 8 frames and a period of 16 tiles; the detector correlates the sign of the local contrast of the quantised
log band energies with the chips over all 128 frame offsets and returns integers.  Nothing here touches the device.

The threshold is derived, not measured: for fixed audio and independent +-1 chips Hoeffding gives P(z >= t) <= exp(-t^2 / 2); over 128 offsets
t = 6.25 bounds the false-alarm rate per segment and key at 128 exp(-19.5) < 5e-7.  The hash is not a proven source of independent bits.

Not verified: nobody has listened to it and no imperceptibility is claimed; it was compared with no other watermark (AudioSeal, WavMark: none is
installed); it was not tested against mp3, Opus or acoustic re-recording; there is no security claim -- this is no defence against someone who
wants the mark gone; strength, bands, tiles and period are unmeasured starting values for 16 kHz speech, and the capacity figures in
INTEGRATION.md are for synthetic signals, not speech.
"""
import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

N_FFT, HOP, BAND0, BAND_BINS, BANDS, TILE, PERIOD = 1024, 256, 20, 4, 48, 8, 16      # EV_WATERMARK_*
CHIPS, OFFSETS, MAX_BITS, MAX_DB = PERIOD * BANDS, TILE * PERIOD, 16, 6.0
DEFAULT_STRENGTH_DB, THRESHOLD = 1.0, 6.25
SAMPLE_RATE = 16000      # the rate the bands were chosen for; ev_watermark_detect resamples a recording at another rate to it first


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _is_number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


@dataclass
class WatermarkConfig:
    """key: a uint32, per call.  payload (None = 0), nbits and strength_db: a scalar for every segment or one entry per segment.  threshold: what
    ``present`` compares z with on the detecting side."""
    key: int = 0
    payload: object = None
    nbits: object = 0
    strength_db: object = DEFAULT_STRENGTH_DB
    threshold: float = THRESHOLD
    want_int16: bool = False               # also the int16 output, clamped (ev_loudness' rule), never wrapped

    def validate(self) -> "WatermarkConfig":
        if not _is_int(self.key) or not 0 <= int(self.key) < 2 ** 32:
            raise ValueError("key %r is not an integer in [0, 2^32)" % (self.key,))
        if not _is_number(self.threshold) or not math.isfinite(float(self.threshold)):
            raise ValueError("threshold %r is not finite" % (self.threshold,))
        for name in ("payload", "nbits", "strength_db"):
            v = getattr(self, name)
            if v is None and name == "payload":
                continue
            if not (_is_number(v) or isinstance(v, (list, tuple, np.ndarray))):
                raise ValueError("%s: a number or one entry per segment, not %r" % (name, v))
        self.per_segment(None)
        return self

    def per_segment(self, B: Optional[int]):
        """(payloads uint32, nbits int32, strengths float32) with B entries each (B None: as many as the longest sequence given, else 1), checked
        by the library's rules; ValueError names the segment."""
        cols = {}
        given = [len(v) for v in (self.payload, self.nbits, self.strength_db) if isinstance(v, (list, tuple, np.ndarray))]
        n = B if B is not None else (max(given) if given else 1)
        for name, v in (("payload", 0 if self.payload is None else self.payload), ("nbits", self.nbits), ("strength_db", self.strength_db)):
            col = [v] * n if _is_number(v) else list(v)
            if len(col) != n:
                raise ValueError("%s: one entry per segment (%d), got %d" % (name, n, len(col)))
            cols[name] = col
        for b in range(n):
            nb, pl, db = cols["nbits"][b], cols["payload"][b], cols["strength_db"][b]
            if not _is_int(nb) or not 0 <= int(nb) <= MAX_BITS:
                raise ValueError("nbits[%d] = %r is not an integer in [0, %d]" % (b, nb, MAX_BITS))
            if not _is_int(pl) or not 0 <= int(pl) < (1 << int(nb)):
                raise ValueError("payload[%d] = %r does not fit %d bits" % (b, pl, int(nb)))
            if not _is_number(db) or not (0.0 <= float(db) <= MAX_DB):
                raise ValueError("strength_db[%d] = %r outside [0, %g]" % (b, db, MAX_DB))
        return np.array(cols["payload"], np.uint32), np.array(cols["nbits"], np.int32), np.array(cols["strength_db"], np.float32)

    def to_struct(self):
        import ctypes as C
        from . import _ffi
        c = _ffi.ev_watermark_config()
        c.struct_size = C.sizeof(_ffi.ev_watermark_config)
        c.key, c.want_i16 = int(self.key), 1 if self.want_int16 else 0
        c.nbits, c.payload, c.strength_db = 0, 0, DEFAULT_STRENGTH_DB      # every call passes the three per-segment arrays
        return c


def parse_flag(text: str) -> WatermarkConfig:
    """``KEY`` or ``KEY:PAYLOAD:NBITS`` (integers, any base Python reads: 0x...) -> a WatermarkConfig: the --watermark flag of the CLIs."""
    parts = str(text).split(":")
    if len(parts) not in (1, 3):
        raise ValueError("--watermark takes KEY or KEY:PAYLOAD:NBITS, not %r" % (text,))
    try:
        vals = [int(p, 0) for p in parts]
    except ValueError:
        raise ValueError("--watermark takes integers, not %r" % (text,)) from None
    return (WatermarkConfig(key=vals[0]) if len(vals) == 1 else WatermarkConfig(key=vals[0], payload=vals[1], nbits=vals[2])).validate()


def watermark_config(x, sr: int = 16000) -> Optional[WatermarkConfig]:
    """The ``watermark=`` argument of EVEngine.synthesize / synthesize_long: None, a key, a ``KEY[:PAYLOAD:NBITS]`` string, a dict of
    WatermarkConfig's fields or a WatermarkConfig -> a validated WatermarkConfig or None.  ``sr`` is accepted for symmetry with the other
    stages: the scheme is stated in frames and bins and does not follow the rate."""
    if x is None or x is False:
        return None
    if isinstance(x, WatermarkConfig):
        return x.validate()
    if isinstance(x, str):
        return parse_flag(x)
    if isinstance(x, dict):
        return WatermarkConfig(**x).validate()
    if _is_int(x):
        return WatermarkConfig(key=int(x)).validate()
    raise ValueError("watermark: None, a key, 'KEY[:PAYLOAD:NBITS]', a dict or a WatermarkConfig, not %r" % (x,))


def out_len(n_samples: int) -> int:
    """Samples ev_watermark returns for a segment of n_samples: whole hops, as ev_denoise."""
    return HOP * (int(n_samples) // HOP)


def z_score(C, n) -> np.ndarray:
    """z = C / sqrt(n) in float64; 0 where n == 0."""
    C, n = np.asarray(C, np.float64), np.asarray(n, np.float64)
    return np.where(n > 0, C / np.sqrt(np.where(n > 0, n, 1.0)), 0.0)


def detect_report(det: Dict[str, object], nbits: int = 0, threshold: float = THRESHOLD) -> List[Dict[str, object]]:
    """The detector's integers (``offset``, ``C``, ``n``, ``bit_C``, ``bit_n`` per segment, as watermark_detect_to_numpy gives them) -> per
    segment dict(z, present, offset, bits, payload, bit_z): z = C / sqrt(n), present = z >= threshold, bit j = C_j < 0.  bits and payload are
    read whether or not the mark is present; they mean nothing when it is not."""
    z = z_score(det["C"], det["n"])
    out = []
    for b in range(len(z)):
        bc, bn = np.asarray(det["bit_C"][b][:nbits], np.int64), np.asarray(det["bit_n"][b][:nbits], np.int64)
        bits = [int(c < 0) for c in bc]
        out.append(dict(z=float(z[b]), present=bool(z[b] >= threshold), offset=int(det["offset"][b]), bits=bits,
                        payload=sum(bit << j for j, bit in enumerate(bits)), bit_z=z_score(np.abs(bc), bn).tolist()))
    return out
