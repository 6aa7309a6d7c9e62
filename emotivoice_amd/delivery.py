"""Response delivery (ev_deliver): the configuration of the device stage that turns the chain's 16 kHz fp32 waveform into what a client asked for
-- another sample rate, and fp32, int16 (optionally TPDF-dithered), G.711 mu-law or A-law bytes -- and the RIFF container those bytes travel in.

The conversion is HIP (csrc/ev_deliver.hip) behind the C entry ev_deliver; include/evhip.h states every output byte.  Nothing here touches the
device.  What is not verified: the filter is ev_resample's own windowed sinc, not soxr or ffmpeg; G.711 is held to CPython's audioop and to a
numpy restatement, no telephony endpoint was exercised; the dither generator is a specified integer hash, checked for mean and variance only;
upsampling after the limiter can overshoot its ceiling, which ``peak`` and ``clipped`` report -- the stage does not limit again.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._ffi import EV_RESAMPLE_MAX_RATIO as MAX_RATIO
from ._ffi import EV_RESAMPLE_MAX_TAPS as MAX_TAPS

ENCODINGS = {"f32": 0, "s16": 1, "ulaw": 2, "alaw": 3}                      # EV_DELIVER_*
DTYPES = {"f32": np.float32, "s16": np.int16, "ulaw": np.uint8, "alaw": np.uint8}
WAV_TAGS = {"s16": 1, "f32": 3, "alaw": 6, "ulaw": 7}                       # WAVE_FORMAT_PCM, _IEEE_FLOAT, _ALAW, _MULAW


@dataclass
class DeliveryConfig:
    """ev_deliver_config without its input rate (the engine's).  ``taps`` (2 half + 1 values, h[-half .. half]) replaces ev_resample's default
    design for the rate pair."""
    sample_rate: int = 16000
    encoding: str = "s16"
    dither: bool = False                   # TPDF, one LSB peak to peak on each side, before the rounding to int16 (also under mu-law / A-law)
    seed: int = 0                          # the dither's seed where the call gives no seed per utterance
    taps: Optional[np.ndarray] = None

    @property
    def dtype(self):
        return DTYPES[self.encoding]

    @property
    def sample_bytes(self) -> int:
        return int(np.dtype(DTYPES[self.encoding]).itemsize)

    def key(self, sr_in: int) -> tuple:
        """What two configs must share to share a setup."""
        taps = None if self.taps is None else np.asarray(self.taps, np.float32).tobytes()
        return (int(sr_in), int(self.sample_rate), self.encoding, bool(self.dither), int(self.seed), taps)

    def output_len(self, L: int, sr_in: int) -> int:
        g = math.gcd(int(sr_in), int(self.sample_rate))
        return -((-int(L) * (int(self.sample_rate) // g)) // (int(sr_in) // g))

    def validate(self, sr_in: int = 16000) -> "DeliveryConfig":
        """The rejections of ev_deliver_setup, with messages that name the field."""
        sr = self.sample_rate
        if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or int(sr) < 1:
            raise ValueError("sample_rate %r must be a positive integer" % (sr,))
        if int(sr_in) < 1:
            raise ValueError("sr_in %r must be positive" % (sr_in,))
        g = math.gcd(int(sr_in), int(sr))
        up, down = int(sr) // g, int(sr_in) // g
        if up > MAX_RATIO or down > MAX_RATIO:
            raise ValueError("sr_in %d -> sample_rate %d is up %d / down %d; both must be <= EV_RESAMPLE_MAX_RATIO %d" % (sr_in, sr, up, down, MAX_RATIO))
        if self.encoding not in ENCODINGS:
            raise ValueError("encoding %r is not one of %s" % (self.encoding, sorted(ENCODINGS)))
        if not isinstance(self.dither, (bool, np.bool_)):
            raise ValueError("dither %r must be a boolean" % (self.dither,))
        if self.dither and self.encoding == "f32":
            raise ValueError("dither with encoding 'f32': nothing is quantised")
        if isinstance(self.seed, bool) or not isinstance(self.seed, (int, np.integer)) or not 0 <= int(self.seed) <= 0xFFFFFFFF:
            raise ValueError("seed %r must be an integer in [0, 2^32)" % (self.seed,))
        if self.taps is not None:
            t = np.asarray(self.taps)
            if t.ndim != 1 or t.size < 3 or t.size % 2 == 0:
                raise ValueError("taps: expected an odd number (2 half_len + 1, half_len >= 1) of values in one dimension, got shape %s" % (t.shape,))
            if t.size > MAX_TAPS:
                raise ValueError("taps: %d values > EV_RESAMPLE_MAX_TAPS %d" % (t.size, MAX_TAPS))
            if not np.isfinite(t.astype(np.float32)).all():
                raise ValueError("taps: every value must be finite")
        return self


def delivery_config(x, sr: int = 16000) -> Optional[DeliveryConfig]:
    """The ``delivery=`` argument of EVEngine.synthesize / synthesize_long and of the serving shell: None, a sample rate in Hz (int16 at that
    rate) or a DeliveryConfig -> None or a DeliveryConfig validated against the engine's rate ``sr``."""
    if x is None:
        return None
    if isinstance(x, DeliveryConfig):
        return x.validate(sr)
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise ValueError("delivery: None, a sample rate in Hz or a DeliveryConfig, not %r" % (x,))
    return DeliveryConfig(sample_rate=int(x)).validate(sr)


def wav_container(data: bytes, sample_rate: int, encoding: str) -> bytes:
    """One mono RIFF/WAVE file around delivered bytes.  Python's ``wave`` writes PCM only; this writes format tag 1 (PCM16: the 16-byte ``fmt ``),
    and 3 (IEEE float), 6 (A-law), 7 (mu-law) with the 18-byte ``fmt `` (cbSize = 0) and the ``fact`` chunk the non-PCM tags require.  An odd
    ``data`` chunk is followed by its pad byte."""
    if encoding not in WAV_TAGS:
        raise ValueError("encoding %r is not one of %s" % (encoding, sorted(WAV_TAGS)))
    data = bytes(data)
    width = int(np.dtype(DTYPES[encoding]).itemsize)
    if len(data) % width:
        raise ValueError("%d bytes are no whole number of %d-byte samples" % (len(data), width))
    sr, tag = int(sample_rate), WAV_TAGS[encoding]
    if sr < 1:
        raise ValueError("sample_rate %r must be positive" % (sample_rate,))
    head = struct.pack("<HHIIHH", tag, 1, sr, sr * width, width, 8 * width)
    if tag == 1:
        chunks = b"fmt " + struct.pack("<I", 16) + head
    else:
        chunks = b"fmt " + struct.pack("<I", 18) + head + struct.pack("<H", 0) + b"fact" + struct.pack("<II", 4, len(data) // width)
    chunks += b"data" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks
