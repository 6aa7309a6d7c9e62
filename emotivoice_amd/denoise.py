"""Vocoder bias removal (ev_denoise): the configuration of the device stage.

The stage is HIP (csrc/ev_denoise.hip) behind the C entries ev_denoise_setup / ev_denoise; include/evhip.h states it: the STFT of the waveform,
``strength`` times the magnitude spectrum of the vocoder's answer to an all-zero mel subtracted from every cell's magnitude and floored at zero, the
phase kept, the inverse STFT with window-sum normalisation -- the Tacotron 2 / WaveGlow / FastPitch ``Denoiser`` on the reference's STFT class.
Nothing here touches the device.

The default strength 0.01 is FastPitch's published value for HiFi-GAN (WaveGlow recipes use 0.1), on vocoders and checkpoints that were not available
here: an unmeasured starting value.  Nobody has listened to a released checkpoint with it; no audible improvement is claimed.
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

DEFAULT_STRENGTH = 0.01
MAX_NFFT, MAX_R, MAX_RUN = 2048, 8, 24576      # EV_FEATURES_MAX_NFFT, EV_DENOISE_MAX_R, EV_FEATURES_MAX_RUN
BIAS_FRAMES = 88                               # EV_DENOISE_BIAS_FRAMES


@dataclass
class DenoiseConfig:
    strength: float = DEFAULT_STRENGTH
    n_fft: int = 1024
    hop: int = 256
    bias: Optional[np.ndarray] = None      # (n_fft / 2 + 1,) magnitudes >= 0, or None: the engine measures its own vocoder's
    want_int16: bool = False               # also the int16 output, clamped (ev_loudness' rule), never wrapped
    report: bool = False                   # adds, per utterance, the removed energy in dB relative to the input (ev_compare)
    window: Optional[np.ndarray] = None    # (n_fft,) float32 analysis / synthesis window, or None: periodic hann

    def validate(self) -> "DenoiseConfig":
        s = self.strength
        if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)) or not (math.isfinite(float(s)) and float(s) >= 0.0):
            raise ValueError("strength %r is not finite and >= 0" % (s,))
        for name, v in (("n_fft", self.n_fft), ("hop", self.hop)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("%s %r is not an integer" % (name, v))
        n_fft, hop = int(self.n_fft), int(self.hop)
        if n_fft < 128 or n_fft % 128 or n_fft > MAX_NFFT:
            raise ValueError("n_fft %d is not a multiple of 128 in [128, %d]" % (n_fft, MAX_NFFT))
        if hop < 8 or hop % 8 or n_fft % hop or n_fft // hop > MAX_R:
            raise ValueError("hop %d is not a multiple of 8 that divides n_fft %d with n_fft / hop <= %d" % (hop, n_fft, MAX_R))
        if 63 * hop + n_fft > MAX_RUN:
            raise ValueError("hop %d: the 63 hop + n_fft samples of a 64-frame tile exceed %d" % (hop, MAX_RUN))
        if self.bias is not None:
            b = np.asarray(self.bias)
            if b.shape != (n_fft // 2 + 1,) or not np.all(np.isfinite(b)) or np.any(b < 0):
                raise ValueError("bias must hold n_fft / 2 + 1 = %d finite magnitudes >= 0" % (n_fft // 2 + 1))
        if self.window is not None:
            w = np.asarray(self.window)
            if w.shape != (n_fft,) or not np.all(np.isfinite(w)):
                raise ValueError("window must hold n_fft = %d finite values" % n_fft)
        return self

    def tables_key(self):
        """What the vocoder's measured bias depends on besides the weights: the frame shape and the window."""
        return (int(self.n_fft), int(self.hop), None if self.window is None else np.ascontiguousarray(self.window, np.float32).tobytes())

    def key(self):
        """What a setup depends on: a changed key means ev_denoise_setup again."""
        b = None if self.bias is None else np.ascontiguousarray(self.bias, np.float32).tobytes()
        return self.tables_key() + (float(np.float32(self.strength)), bool(self.want_int16), b)


def denoise_config(x, sr: int = 16000) -> Optional[DenoiseConfig]:
    """The ``denoise=`` argument of EVEngine.synthesize / synthesize_long: None, True (the default strength), a strength, a dict of DenoiseConfig's
    fields or a DenoiseConfig -> a validated DenoiseConfig or None.  ``sr`` is accepted for symmetry with the other stages: the frame shape is
    given in samples and does not follow the rate."""
    if x is None or x is False:
        return None
    if isinstance(x, DenoiseConfig):
        return x.validate()
    if x is True:
        return DenoiseConfig().validate()
    if isinstance(x, dict):
        return DenoiseConfig(**x).validate()
    if isinstance(x, (int, float, np.integer, np.floating)):
        return DenoiseConfig(strength=float(x)).validate()
    raise ValueError("denoise: None, True, a strength, a dict or a DenoiseConfig, not %r" % (x,))


def out_len(n_samples: int, hop: int = 256) -> int:
    """Samples ev_denoise returns for an utterance of n_samples: the reference's inverse STFT rounds down to whole hops."""
    return int(hop) * (int(n_samples) // int(hop))


def removed_db(sum_d2, sum_y2) -> np.ndarray:
    """10 log10(sum (in - out)^2 / sum in^2) per utterance from ev_compare's sums (a = the output, b = the input); -inf where nothing was removed."""
    d2, y2 = np.asarray(sum_d2, np.float64), np.asarray(sum_y2, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(d2 / y2)
