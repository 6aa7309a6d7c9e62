"""float64 restatement of ev_loudness (include/evhip.h): the K-weighting design, the filter (scipy.signal.lfilter, sequential from a zero state),
the 400 ms blocks at a 100 ms step, the two gates, the gain rule and the output rules, plus the signals the tests use.

It is written from the specification, not from the device code: the device sums y^2 tile by tile and step by step, this file takes np.mean of a
block, so the two agree to fp64 rounding, not to the bit.
"""
import math

import numpy as np
from scipy.signal import lfilter

SAMPLE_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
UNDEFINED, BOOST_LIMITED, PEAK_LIMITED = 1, 2, 4
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): shelf b0 b1 b2 a1 a2, high-pass a1 a2 (its b is 1, -2, 1)
STANDARD_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, -1.99004745483398, 0.99007225036621)


def design(sample_rate):
    """The ten coefficients: shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2."""
    fs = float(sample_rate)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(shelf + hp, np.float64)


def to_f64(x):
    """The samples as the measurement sees them, and the mask of the non-finite ones: int16 is s / 32768, fp32 is widened, non-finite enters as 0."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float64) / 32768.0, np.zeros(x.shape, bool)
    v = x.astype(np.float32).astype(np.float64)
    bad = ~np.isfinite(v)
    return np.where(bad, 0.0, v), bad


def k_weight(x64, sample_rate):
    c = design(sample_rate)
    y = lfilter(c[0:3], [1.0, c[3], c[4]], x64)
    return lfilter(c[5:8], [1.0, c[8], c[9]], y)


def block_ms(y, sample_rate):
    step = sample_rate // 10
    block = 4 * step
    n = y.size
    if n < block:
        return np.array([np.mean(y * y)])
    nblk = (n - block) // step + 1
    return np.array([np.mean(y[j * step:j * step + block] ** 2) for j in range(nblk)])


def lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(np.asarray(z, np.float64))


def gate(z):
    """z -> (loudness, rel_threshold, block_state, the blocks' l_j)."""
    l = lufs(z)
    state = np.zeros(z.size, np.uint8)
    keep = l > -70.0
    if not keep.any():
        return -np.inf, -np.inf, state, l
    state[keep] = 1
    gamma = float(lufs(np.mean(z[keep]))) - 10.0
    keep2 = keep & (l > gamma)
    state[keep2] = 2
    return float(lufs(np.mean(z[keep2]))), gamma, state, l


def gain_for(loudness, peak, target_lufs, max_gain_db=20.0, peak_ceiling=np.float32(10.0 ** (-1.0 / 20.0))):
    """The host rule -> (gain as np.float32, flags)."""
    flags = UNDEFINED if loudness == -np.inf else 0
    if math.isnan(target_lufs):
        return np.float32(1.0), flags
    g = 1.0 if loudness == -np.inf else 10.0 ** ((target_lufs - loudness) / 20.0)
    gmax = 10.0 ** (max_gain_db / 20.0)
    if g > gmax:
        g, flags = gmax, flags | BOOST_LIMITED
    if peak > 0:
        gpk = float(np.float32(peak_ceiling)) / float(np.float32(peak))
        if g > gpk:
            g, flags = gpk, flags | PEAK_LIMITED
    return np.float32(g), flags


def source_f32(x):
    x = np.asarray(x)
    return x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x.astype(np.float32)


def apply_gain(x, gain):
    """out = x * gain, one fp32 product; the source bits where gain == 1."""
    xf = source_f32(x)
    g = np.float32(gain)
    with np.errstate(invalid="ignore", over="ignore"):
        return xf.copy() if g == np.float32(1.0) else (xf * g).astype(np.float32)


def to_i16(out):
    """ev_stitch's rule: (int)(out * 32768.0f) truncated toward zero, then clamped; NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(out, np.float32) * np.float32(32768.0)).astype(np.float64)
    t = np.where(np.isnan(t), 0.0, t)
    return np.clip(np.trunc(t), -32768, 32767).astype(np.int16)


def measure(x, sample_rate=16000, target_lufs=float("nan"), max_gain_db=20.0, peak_ceiling=np.float32(10.0 ** (-1.0 / 20.0))):
    """Everything ev_loudness reports for one segment."""
    x = np.asarray(x)
    x64, bad = to_f64(x)
    z = block_ms(k_weight(x64, sample_rate), sample_rate)
    loudness, gamma, state, l = gate(z)
    xf = source_f32(x)
    fin = np.abs(xf[~bad]) if not bad.all() else np.zeros(0, np.float32)
    peak = np.float32(fin.max()) if fin.size else np.float32(0.0)
    g, flags = gain_for(loudness, peak, target_lufs, max_gain_db, peak_ceiling)
    return dict(loudness=loudness, rel_threshold=gamma, block_ms=z, block_state=state, block_lufs=l, peak=peak, nonfinite=int(bad.sum()), gain=g, flags=flags)


# ---------------------------------------------------------------------------------------------------------------------------------- signals
def sine(freq, seconds, sample_rate, amp=1.0):
    t = np.arange(int(round(seconds * sample_rate)), dtype=np.float64) / sample_rate
    return (amp * np.sin(2.0 * np.pi * freq * t)).astype(np.float32)


def voiced(n, sample_rate=16000, seed=0, amp=0.22):
    """A voiced-like signal: 24 harmonics of 120 Hz with a 1 / h roll-off (below Nyquist), a 3 Hz envelope and a noise floor; float32."""
    t = np.arange(n, dtype=np.float64) / sample_rate
    x = sum(np.sin(2 * np.pi * 120.0 * h * t + 0.37 * h) / h for h in range(1, 25) if 120.0 * h < 0.45 * sample_rate)
    x = x * (0.5 * (1.0 + np.sin(2 * np.pi * 3.0 * t)))
    x = amp * x + 0.002 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32)


def gated_signal(sample_rate=16000):
    """4 s: 2.2 s of a voiced signal, 0.9 s of it at -45 dB (the relative gate's share), 0.9 s of digital zeros (the absolute gate's)."""
    n = 4 * sample_rate
    x = voiced(n, sample_rate, seed=3).astype(np.float64)
    a, b = int(2.2 * sample_rate), int(3.1 * sample_rate)
    x[a:b] *= 10.0 ** (-45.0 / 20.0)
    x[b:] = 0.0
    return x.astype(np.float32)


def spiky(n, sample_rate=16000):
    """A quiet voiced signal with a few full-scale samples: the peak limit binds long before the target is met."""
    x = voiced(n, sample_rate, seed=5, amp=0.01)
    x[n // 3], x[n // 2] = 0.97, -0.99
    return x
