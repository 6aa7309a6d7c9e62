"""numpy oracle of ev_resample's specification (include/evhip.h): the prototype filter, the direct-sum polyphase resampler and the reference's trim
(prompt_dataset.get_mel), in float64, and the same in float32 with the specified summation order (four interleaved partial sums of fmaf over
(k - k_lo) mod 4, combined as (s0 + s1) + (s2 + s3))."""
import math

import numpy as np


def ratio(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def design(sr_in, sr_out, zeros=16, rolloff=0.945, beta=9.0):
    """(h float32 (2 half + 1,), up, down, half): designed in float64, rounded once."""
    up, down = ratio(sr_in, sr_out)
    q = max(up, down)
    half = zeros * q
    i = np.arange(-half, half + 1, dtype=np.float64)
    g = np.sinc(rolloff * i / q) * np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (i / half) ** 2))) / np.i0(beta)
    return (up * g / g.sum()).astype(np.float32), up, down, half


def output_len(L, up, down):
    return -((-L * up) // down)


def as_float(x):
    """What the kernel reads: int16 is x / 32768 (exact in float32)."""
    x = np.asarray(x)
    return x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x.astype(np.float32)


def _terms(L, n, h, up, down):
    """Per output m (rows): the input indices k_lo .. k_lo + K - 1, the tap of each, and which of them take part (k <= k_hi; x is zero outside
    [0, L), which the caller applies)."""
    half = (h.size - 1) // 2
    md = np.arange(n, dtype=np.int64) * down
    k_lo = -((-(md - half)) // up)
    k_hi = (md + half) // up
    K = int((k_hi - k_lo).max()) + 1
    k = k_lo[:, None] + np.arange(K, dtype=np.int64)[None, :]
    live = k <= k_hi[:, None]
    tap = np.where(live, md[:, None] - k * up + half, 0)
    return k, tap, live


def resample64(x, h, up, down):
    """y[m] = sum_k x[k] h[m down - k up] in float64 on the float32 taps and the float32 (or int16 / 32768) samples."""
    x = as_float(x).astype(np.float64)
    L = x.size
    n = output_len(L, up, down)
    if up == 1 and down == 1:
        return x.copy()
    k, tap, live = _terms(L, n, h, up, down)
    inside = live & (k >= 0) & (k < L)
    xs = np.where(inside, x[np.clip(k, 0, L - 1)], 0.0)
    hs = np.where(live, h.astype(np.float64)[tap], 0.0)
    return (xs * hs).sum(axis=1)


def _fmaf(a, b, c):
    """float32 fma through float64: the product of two float32 is exact there; the sum is rounded twice, which differs from a true fma only in
    rare ties."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def resample32(x, h, up, down):
    """The specified float32 evaluation: fmaf into four partial sums over (k - k_lo) mod 4, k ascending, (s0 + s1) + (s2 + s3)."""
    x = as_float(x)
    L = x.size
    n = output_len(L, up, down)
    if up == 1 and down == 1:
        return x.copy()
    k, tap, live = _terms(L, n, h, up, down)
    inside = live & (k >= 0) & (k < L)
    xs = np.where(inside, x[np.clip(k, 0, L - 1)], np.float32(0.0)).astype(np.float32)
    hs = h.astype(np.float32)[tap]
    s = [np.zeros(n, np.float32) for _ in range(4)]
    for j in range(k.shape[1]):
        upd = _fmaf(xs[:, j], hs[:, j], s[j & 3])
        s[j & 3] = np.where(live[:, j], upd, s[j & 3])
    return ((s[0] + s[1]) + (s[2] + s[3])).astype(np.float32)


def accumulation_bound(h, up, ntaps_per_output, max_abs_x):
    """(ntaps + 2) 2^-24 max_p sum_j |h_p[j]| max|x|: the float32 accumulation bound of the specified sum, per output sample."""
    half = (h.size - 1) // 2
    a = np.abs(h.astype(np.float64))
    worst = max(a[(half + p) % up::up].sum() for p in range(up))
    return (ntaps_per_output + 2) * 2.0 ** -24 * worst * float(max_abs_x)


def taps_per_output(h, up):
    return (h.size - 1) // up + 1


def trim(y, frac=0.005, pad=800):
    """prompt_dataset.get_mel:38-46 on a float32 waveform: (out, start, end).  thr is one float32 product; the slice excludes ``end``; no
    sample above the threshold gives the empty cut (the reference raises)."""
    y = np.asarray(y, np.float32)
    a = np.abs(y)
    thr = np.float32(a.max()) * np.float32(frac)
    idx = np.nonzero(a > thr)[0]
    start, end = (int(idx[0]), int(idx[-1])) if idx.size else (0, 0)
    z = np.zeros(pad, np.float32)
    return np.concatenate([z, y[start:end], z]), start, end


def trim64(y, frac=0.005):
    """(start, end, thr) of the same rule on a float64 waveform."""
    a = np.abs(np.asarray(y, np.float64))
    thr = a.max() * float(np.float32(frac))
    idx = np.nonzero(a > thr)[0]
    return (int(idx[0]), int(idx[-1]), thr) if idx.size else (0, 0, thr)


def cut_margin(y, thr, start, end, reach=64):
    """The least | |y| - thr | within ``reach`` samples of either cut: how far the float64 decision is from flipping."""
    a = np.abs(np.asarray(y, np.float64))
    near = np.zeros(a.size, bool)
    for c in (start, end):
        near[max(0, c - reach):c + reach + 1] = True
    return float(np.abs(a[near] - thr).min())


def tone(f, sr, seconds, amp=1.0):
    return (amp * np.sin(2.0 * np.pi * f * np.arange(int(round(sr * seconds))) / sr)).astype(np.float32)


def speechlike(seed, L, sr, i16=False):
    """Harmonics of a wandering 90-300 Hz fundamental up to 0.4 sr under a slow envelope, plus broadband noise: energy across the band."""
    rng = np.random.default_rng(seed)
    nk = L // (sr // 2) + 2
    f0 = np.interp(np.arange(L), np.linspace(0, L - 1, nk), rng.uniform(90.0, 300.0, nk))
    ph = 2.0 * np.pi * np.cumsum(f0) / sr
    x = np.zeros(L)
    for hh in range(1, 40):
        x += np.where(f0 * hh < 0.4 * sr, np.sin(hh * ph + rng.uniform(0, 6.28)) / hh, 0.0)
    env = 0.5 + 0.5 * np.sin(2.0 * np.pi * 3.0 * np.arange(L) / sr)
    x = 0.25 * x * env + 0.02 * rng.standard_normal(L)
    if i16:
        return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)
