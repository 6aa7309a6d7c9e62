"""numpy restatement of ev_limit (include/evhip.h), bit for bit: the pre-gain, the 4x true-peak meter (an fp64 sum of exact fp32 x fp32 products in
ascending order, rounded once), the required gain, the erosion on the extended index range, the smoothing window, the gain and the output rules.

It is written from the specification, not from the device code.  The interpolator's taps are an argument: the default is the Python design of
tests/resample_oracle.py, which the library's design matches to one fp32 ulp (tests/test_resample.py), not to the bit; the GPU tests pass the
library's own taps (emotivoice_amd.limiter.interpolator), so that every output bit can be compared.
"""
import math

import numpy as np

import loudness_oracle as lo
import resample_oracle as ro

HALO = 16
DEFAULT_CEILING = np.float32(10.0 ** (-1.0 / 20.0))
# The largest overshoot of the output's true peak above the ceiling that this oracle shows on the voiced signal of tests/test_limit.py (gains 1,
# 2.5, 6; (L, Hd) = (16, 0), (5, 37), (80, 800)): 2.21e-4, at gain 6 with (16, 0).  The meter is linear and the output is the input times a
# smooth gain, but the gain differs between the 32 samples one interpolated value reads, so the true peak is held only to the gain's variation
# over them.  MARGIN is twice that figure.  L = 0 is excluded: nothing smooths the gain there, and the true peak overshoots by 4 % at gain 2.5
# and 17 % at gain 6 while the sample peak holds.
WORST_OVERSHOOT = 2.21e-4
MARGIN = 2.0 * WORST_OVERSHOOT


def taps():
    """h[-64 .. 64] = design(1, 4, 16, 0.945, 9.0) as float32 (129,)."""
    h, up, down, half = ro.design(1, 4)
    assert (up, down, half, h.size) == (4, 1, 64, 129)
    return h


def pre(x, gain=1.0):
    """u = x * gain, one fp32 product; the source bits where gain == 1."""
    return lo.apply_gain(x, gain)


def meter(u, h=None):
    """u (float32) -> dict(p, sample_peak, true_peak, nonfinite, v): the specification's oversampled signal and peaks."""
    h64 = (taps() if h is None else np.asarray(h, np.float32)).astype(np.float64)
    u = np.asarray(u, np.float32)
    bad = ~np.isfinite(u)
    uz = np.where(bad, np.float32(0.0), u)
    n = uz.size
    pad = np.concatenate([np.zeros(HALO), uz.astype(np.float64), np.zeros(HALO)])
    v = np.empty((n, 4), np.float32)
    with np.errstate(over="ignore"):
        for q in range(4):
            acc = np.zeros(n, np.float64)
            for d in range(-HALO, HALO + 1):      # k = n + d ascending
                i = q - 4 * d
                if abs(i) <= 64:
                    acc = acc + pad[HALO + d:HALO + d + n] * h64[i + 64]
            v[:, q] = acc.astype(np.float32)
    p = np.maximum(np.abs(uz), np.abs(v).max(axis=1))
    return dict(p=p, v=v.reshape(-1), sample_peak=np.float32(np.abs(uz).max()), true_peak=np.float32(p.max()), nonfinite=int(bad.sum()))


def required(p, ceiling=DEFAULT_CEILING):
    c = np.float32(ceiling)
    with np.errstate(divide="ignore"):
        q = (np.float64(c) / p.astype(np.float64)).astype(np.float32)
    return np.where(p <= c, np.float32(1.0), q)


def sliding_min(a, W):
    """out[i] = min a[i .. i + W), len(a) - W + 1 values."""
    cur, span = a, 1
    while 2 * span <= W:
        cur = np.minimum(cur[:-span], cur[span:])
        span *= 2
    n = a.size - W + 1
    return np.minimum(cur[:n], cur[W - span:W - span + n])


def erode(r, L, Hd):
    """m[k] = min r[k - Hd .. k + L] for k = -L .. len - 1 (r = 1 outside [0, len)): len + L values, m[k] at index k + L."""
    one = np.float32(1.0)
    ext = np.concatenate([np.full(L + Hd, one), r, np.full(L, one)])
    return sliding_min(ext, L + Hd + 1)


def window(L):
    """The L + 1 fp32 taps: 1 - cos(2 pi (j + 1) / (L + 2)) over its ascending sum, then lowered until the fp64 sum of the fp32 taps is <= 1."""
    g = [1.0 - math.cos(2.0 * math.pi * (j + 1) / (L + 2)) for j in range(L + 1)]
    total = 0.0
    for x in g:
        total += x
    w = np.array([x / total for x in g], np.float64).astype(np.float32)
    while True:
        acc = 0.0
        for x in w:
            acc += float(x)
        if not acc > 1.0:
            return w
        top = int(np.argmax(w))      # the first largest
        w[top] = np.nextafter(w[top], np.float32(0.0))


def gain(m, w, L):
    """s[n] = 1 where m[n - L .. n] are all 1, else (float)(sum_j w[j] m[n - j]) in fp64, j ascending."""
    n = m.size - L
    m64, w64 = m.astype(np.float64), w.astype(np.float64)
    acc = np.zeros(n, np.float64)
    for j in range(L + 1):
        acc = acc + w64[j] * m64[L - j:L - j + n]
    return np.where(sliding_min(m, L + 1) == np.float32(1.0), np.float32(1.0), acc.astype(np.float32))


def limit(x, gain_in=1.0, ceiling=DEFAULT_CEILING, L=80, Hd=800, h=None):
    """Everything ev_limit reports for one segment, and the intermediate r, m and s."""
    u = pre(x, gain_in)
    mi = meter(u, h)
    r = required(mi["p"], ceiling)
    m = erode(r, L, Hd)
    s = gain(m, window(L), L)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.where(s == np.float32(1.0), u, (u * s).astype(np.float32))
    mo = meter(y, h)
    return dict(u=u, r=r, m=m, s=s, wav=y, wav_i16=lo.to_i16(y), true_peak_in=mi["true_peak"], sample_peak_in=mi["sample_peak"],
                true_peak_out=mo["true_peak"], sample_peak_out=mo["sample_peak"], min_gain=np.float32(s.min()), limited=int((s < 1).sum()),
                nonfinite=mi["nonfinite"])


def voiced_half(n=8000):
    """The tests' voiced signal scaled to a sample peak of 0.5, float32."""
    x = lo.voiced(n).astype(np.float64)
    return (x * (0.5 / np.abs(x).max())).astype(np.float32)
