"""Float64 statement of the acoustic features ev_features computes (include/evhip.h, steps 1-6), on the float32 tables the reference and the
device hold: the yardstick both the reference's float32 result and the device's are measured against (tests/test_features.py,
tests/test_gpu_features.py)."""
import numpy as np

from emotivoice_amd.features import hann_window, mel_filterbank

_BASIS = {}


def basis_f32(n_fft=1024, window=None):
    """(re, im) float32 (n_bins, n_fft): float32(cos / -sin(2 pi k n / n_fft)) * float32(window), a float32 product."""
    key = (n_fft, None if window is None else np.asarray(window, np.float32).tobytes())
    if key not in _BASIS:
        k = np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None]
        n = np.arange(n_fft, dtype=np.int64)[None, :]
        ang = 2.0 * np.pi * ((k * n) % n_fft).astype(np.float64) / n_fft
        win = hann_window(n_fft) if window is None else np.asarray(window, np.float32)
        _BASIS[key] = (np.cos(ang).astype(np.float32) * win[None, :], (-np.sin(ang)).astype(np.float32) * win[None, :])
    return _BASIS[key]


def to_float(wav):
    wav = np.asarray(wav).reshape(-1)
    if wav.dtype == np.int16:
        return wav.astype(np.float32) / np.float32(32768.0)
    return wav.astype(np.float32)


def features64(wav, mel_basis=None, n_fft=1024, hop=256, mel_clip=1e-5, energy_floor=1e-10, window=None):
    """dict(mag (T, n_bins), mel_lin (n_mels, T) before the clamp, mel (n_mels, T), energy (T,)) in float64 for one utterance (float or int16)."""
    x = to_float(wav).astype(np.float64)
    if x.size < n_fft // 2 + 1:
        raise ValueError("utterance shorter than n_fft / 2 + 1")
    mb = (mel_filterbank(n_fft=n_fft) if mel_basis is None else np.asarray(mel_basis, np.float32)).astype(np.float64)
    padded = np.pad(x, n_fft // 2, mode="reflect")
    T = x.size // hop + 1
    frames = np.lib.stride_tricks.sliding_window_view(padded, n_fft)[::hop][:T]
    re_b, im_b = basis_f32(n_fft, window)
    re = frames @ re_b.astype(np.float64).T
    im = frames @ im_b.astype(np.float64).T
    mag = np.sqrt(re * re + im * im)
    mel_lin = mb @ mag.T
    clip = float(np.float32(mel_clip))
    return dict(mag=mag, mel_lin=mel_lin, mel=np.log(np.maximum(mel_lin, clip)),
                energy=np.sqrt(np.maximum((mag * mag).sum(axis=1), float(np.float32(energy_floor)))))


def mel_error(mel, mel64):
    """E(x) = max over (t, m) of |exp(x) - exp(mel64)| / max_m exp(mel64[t]); mel, mel64 (n_mels, T)."""
    a, b = np.exp(np.asarray(mel, np.float64)), np.exp(np.asarray(mel64, np.float64))
    return float((np.abs(a - b) / b.max(axis=0, keepdims=True)).max())


def energy_error(e, e64):
    """max_t |e - e64| relative to the utterance's largest frame energy."""
    e, e64 = np.asarray(e, np.float64), np.asarray(e64, np.float64)
    return float(np.abs(e - e64).max() / e64.max())


def mag_error(mag, mag64):
    """max over (t, k) of |mag - mag64| relative to the frame's largest magnitude (frames of exact silence: relative to 1)."""
    mag, mag64 = np.asarray(mag, np.float64), np.asarray(mag64, np.float64)
    den = mag64.max(axis=1, keepdims=True)
    return float((np.abs(mag - mag64) / np.where(den > 0, den, 1.0)).max())
