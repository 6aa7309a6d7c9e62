"""Float64 statement of the vocoder bias removal ev_denoise computes (include/evhip.h, steps 1-7), on the float32 tables the reference and the
device hold: the yardstick both the reference's float32 STFT.transform -> clamp(mag - s bias, 0) -> STFT.inverse and the device's result are
measured against (tests/test_denoise.py, tests/test_gpu_denoise.py).  The forward half is features_oracle's."""
import numpy as np

import features_oracle as fo
from emotivoice_amd.features import hann_window

TINY = float(np.finfo(np.float32).tiny)
_IBASIS = {}


def window_f32(n_fft=1024, window=None):
    return hann_window(n_fft) if window is None else np.asarray(window, np.float32)


def k_pad(n_fft):
    return (2 * (n_fft // 2 + 1) + 31) // 32 * 32


def inverse_basis_f32(n_fft=1024, window=None, all_two=False):
    """(cos part, sin part) float32 (n_bins, n_fft): float32(c_k cos / -c_k sin(2 pi k m / n_fft)) * float32(window[m]), c_k = 1, 2, ..., 2, 1.
    ``all_two``: every c_k = 2 -- a WRONG basis, the negative control of the GPU test."""
    key = (n_fft, None if window is None else np.asarray(window, np.float32).tobytes(), all_two)
    if key not in _IBASIS:
        k = np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None]
        m = np.arange(n_fft, dtype=np.int64)[None, :]
        ang = 2.0 * np.pi * ((k * m) % n_fft).astype(np.float64) / n_fft
        ck = np.full((n_fft // 2 + 1, 1), 2.0)
        if not all_two:
            ck[0, 0] = ck[-1, 0] = 1.0
        win = window_f32(n_fft, window)
        _IBASIS[key] = ((ck * np.cos(ang)).astype(np.float32) * win[None, :], (-ck * np.sin(ang)).astype(np.float32) * win[None, :])
    return _IBASIS[key]


def window_sq64(n_fft=1024, window=None):
    """The squares the envelope adds, float64: of the float64 periodic hann for window None (the reference squares scipy's float64 window), else
    of the float32 window the caller gave."""
    if window is None:
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)) ** 2
    return np.asarray(window, np.float32).astype(np.float64) ** 2


def envelope_f32(T, n_fft=1024, hop=256, window=None):
    """The window-sum envelope over the untrimmed signal, n_fft + hop (T - 1) float32: a float32 accumulator, += the float64 squares of
    window_sq64, frames ascending -- how the reference's window_sumsquare sums it."""
    w2 = window_sq64(n_fft, window)
    x = np.zeros(n_fft + hop * (T - 1), np.float32)
    for t in range(T):
        x[t * hop:t * hop + n_fft] += w2
    return x


def envelope_table(n_fft=1024, hop=256, window=None):
    """istft_pack_envelope: (R, R, hop) float32, entry [qa][qb][n] = the envelope at phase n of a chunk reached by the frames q = qa .. qb of its R
    candidates (frame j - R + 1 + q at offset (R - 1 - q) hop + n), summed in ascending q; 0 for qa > qb."""
    R = n_fft // hop
    w2 = window_sq64(n_fft, window)
    tab = np.zeros((R, R, hop), np.float32)
    for qa in range(R):
        for qb in range(qa, R):
            x = np.zeros(hop, np.float32)
            for q in range(qa, qb + 1):
                x += w2[(R - 1 - q) * hop:(R - q) * hop]
            tab[qa, qb] = x
    return tab


def envelope_from_table(tab, T, n_fft=1024, hop=256):
    """The envelope over the untrimmed signal as the device reads it from the table: per chunk j, qa = max(0, R - 1 - j), qb = min(R - 1, T + R - 2 - j)."""
    R = n_fft // hop
    out = np.zeros(n_fft + hop * (T - 1), np.float32)
    for j in range(T + R - 1):
        qa, qb = max(0, R - 1 - j), min(R - 1, T + R - 2 - j)
        out[j * hop:(j + 1) * hop] = tab[qa, qb]
    return out


def stft64(wav, n_fft=1024, hop=256, window=None):
    """(re, im) float64 (T, n_bins) of one utterance (float or int16): steps 1-2."""
    x = fo.to_float(wav).astype(np.float64)
    if x.size < n_fft // 2 + 1:
        raise ValueError("utterance shorter than n_fft / 2 + 1")
    padded = np.pad(x, n_fft // 2, mode="reflect")
    T = x.size // hop + 1
    frames = np.lib.stride_tricks.sliding_window_view(padded, n_fft)[::hop][:T]
    re_b, im_b = fo.basis_f32(n_fft, window)
    return frames @ re_b.astype(np.float64).T, frames @ im_b.astype(np.float64).T


def gain64(re, im, bias, strength):
    """Step 3: (g re, g im, mag) float64; bias (n_bins,) and strength as the float32 values the device holds.  A cell whose mag is not greater
    than 0 -- zero, or a NaN -- is a zero cell: selected, not multiplied by 0 (0 * NaN is NaN)."""
    with np.errstate(invalid="ignore"):
        mag = np.sqrt(re * re + im * im)
        live = mag > 0
    sb = float(np.float32(strength)) * np.asarray(bias, np.float32).astype(np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(live, np.maximum(mag - sb, 0.0) / np.where(live, mag, 1.0), 0.0)
        return np.where(live, g * re, 0.0), np.where(live, g * im, 0.0), mag


def istft64(gre, gim, n_fft=1024, hop=256, window=None, all_two=False):
    """Steps 4-6: the spectrum (T, n_bins) -> hop (T - 1) float64 samples."""
    T = gre.shape[0]
    cb, sb = inverse_basis_f32(n_fft, window, all_two)
    fr = gre @ cb.astype(np.float64) + gim @ sb.astype(np.float64)      # (T, n_fft): every frame's windowed inverse DFT, unnormalised
    u = np.zeros(n_fft + hop * (T - 1), np.float64)
    for t in range(T):
        u[t * hop:t * hop + n_fft] += fr[t]
    y = u * (1.0 / n_fft)
    env = envelope_f32(T, n_fft, hop, window).astype(np.float64)
    ok = env > TINY
    y[ok] = y[ok] / env[ok]
    return y[n_fft // 2:n_fft // 2 + hop * (T - 1)]


def denoise64(wav, bias, strength, n_fft=1024, hop=256, window=None, all_two=False):
    """Steps 1-6 for one utterance: hop (len // hop) float64 samples."""
    re, im = stft64(wav, n_fft, hop, window)
    gre, gim, _ = gain64(re, im, bias, strength)
    return istft64(gre, gim, n_fft, hop, window, all_two)


def to_i16(y):
    """Step 7 on float32 samples: one float32 product, the clamp, truncation toward zero; NaN -> 0."""
    t = np.asarray(y, np.float32) * np.float32(32768.0)
    return np.where(np.isnan(t), 0, np.trunc(np.clip(t, -32768.0, 32767.0))).astype(np.int16)


def split_planes(x):
    """float values -> (hi, lo) float16 with x ~ hi + lo / 2048: the device's split, for feeding ev_op_istft a spectrum of the oracle's."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


def pack_spectrum(gre, gim, n_fft=1024):
    """(T, n_bins) re / im -> the scratch layout (T, k_pad) float32: column 2 k = re, 2 k + 1 = im, zero padding columns."""
    T, nb = gre.shape
    out = np.zeros((T, k_pad(n_fft)), np.float32)
    out[:, 0:2 * nb:2], out[:, 1:2 * nb:2] = gre, gim
    return out


def peak_error(y, y64):
    """E = max |y - y64| / max |y64| of one utterance."""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    den = np.abs(y64).max() if y64.size else 0.0
    return float(np.abs(y - y64).max() / (den if den > 0 else 1.0)) if y64.size else 0.0
