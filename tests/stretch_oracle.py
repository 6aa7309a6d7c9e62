"""The rules of ev_stretch (include/evhip.h) restated in numpy: WSOLA with an integer search on 12-bit decision samples and a two-term
overlap-add in fp64.  Every bit of the device's result is decided here; the tests hold deltas, sum_dist, edge_frames, the fp32 bits and the
int16 against it without a tolerance.  ``Rules`` switches one rule at a time to a deliberately wrong one, for the tests that show each rule
is pinned by a case."""
import dataclasses

import numpy as np

N, H, LAGS = 512, 256, 256            # EV_STRETCH_FRAME, EV_STRETCH_HOP, EV_STRETCH_LAGS: lags -128 .. 127
MAX_SAMPLES = 1 << 30                 # EV_STRETCH_MAX_SAMPLES


@dataclasses.dataclass(frozen=True)
class Rules:
    tie_reversed: bool = False        # ties to the LARGEST |lag|, then the positive one
    a_truncated: bool = False         # a_k = floor(k H L_in / L_out) without the rounding half
    template_nominal: bool = False    # the template at a_(k-1) + H instead of p_(k-1) + H
    q16_wrapping: bool = False        # q at 16 bits (x 32768, clamp to +-32767) with wrapping int32 sums
    window_float: bool = False        # the window as the fp32 rounding of the cosine, off the 2^-23 lattice


RIGHT = Rules()


def window(rules: Rules = RIGHT) -> np.ndarray:
    """The rising half, (256,) float32: rint(2^23 (0.5 - 0.5 cos(2 pi j / N))) / 2^23.  The falling half is 1 - w, exact in fp32."""
    c = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(H, dtype=np.float64) / N)
    if rules.window_float:
        return c.astype(np.float32)
    w = np.rint(c * 2.0 ** 23) / 2.0 ** 23
    assert np.array_equal(w.astype(np.float32).astype(np.float64), w)
    return w.astype(np.float32)


def rint_half_even(v: float) -> int:
    return int(np.rint(np.float64(v)))


def plan_length(L_in: int, speed=None, target=None) -> int:
    """L_out of one segment and the checks of ev_stretch_plan; ValueError names the rule."""
    L_in = int(L_in)
    if target is not None:
        L_out = int(target)
    else:
        s = 1.0 if speed is None else float(speed)
        if not (np.isfinite(s) and s > 0):
            raise ValueError("speed %r is not finite and > 0" % (s,))
        L_out = max(1, rint_half_even(np.float64(L_in) / np.float64(s)))
    check_lengths(L_in, L_out)
    return L_out


def check_lengths(L_in: int, L_out: int) -> None:
    if L_in < 1:
        raise ValueError("L_in = %d < 1" % L_in)
    if L_out < 1:
        raise ValueError("L_out = %d < 1" % L_out)
    if L_in > MAX_SAMPLES or L_out > MAX_SAMPLES:
        raise ValueError("more than EV_STRETCH_MAX_SAMPLES")
    if min(L_in, L_out) >= N and (L_in > 2 * L_out or L_out > 2 * L_in):
        raise ValueError("the ratio %d : %d lies outside [0.5, 2]" % (L_in, L_out))


def as_samples(x) -> np.ndarray:
    """load_sample: int16 s -> s / 32768 (exact), floating -> float32."""
    x = np.asarray(x)
    return (x.astype(np.float32) / np.float32(32768.0)) if x.dtype == np.int16 else x.astype(np.float32)


def quantise(x: np.ndarray, rules: Rules = RIGHT) -> np.ndarray:
    """q: clamp(rint(x 2048), -2047, 2047), 0 for a non-finite sample; int64."""
    scale, top = (32768.0, 32767.0) if rules.q16_wrapping else (2048.0, 2047.0)
    v = x.astype(np.float64) * scale
    fin = np.isfinite(x)
    q = np.clip(np.rint(np.where(fin, v, 0.0)), -top, top)
    return np.where(fin, q, 0.0).astype(np.int64)


def s16_trunc(y: np.ndarray) -> np.ndarray:
    """The clamping int16 of the audio stages: one rounded fp32 product, the clamp, truncation toward zero; NaN -> 0."""
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.clip(y * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))
    return np.where(np.isnan(y), 0, np.trunc(np.where(np.isnan(v), 0, v))).astype(np.int16)


def stretch(x, L_out: int, rules: Rules = RIGHT) -> dict:
    """One segment.  Returns wav (L_out,) float32, wav_i16, deltas (K,) int16, frames, edge_frames, sum_dist, nonfinite."""
    x = as_samples(x).reshape(-1)
    L_in, L_out = int(x.size), int(L_out)
    check_lengths(L_in, L_out)
    K = -(-L_out // H)
    pad_lo, pad_hi = H + LAGS, N + H + 2 * LAGS + 2 * H      # every index a frame can touch lies inside the padding
    a = [((k * H * L_in) // L_out) if rules.a_truncated else ((2 * k * H * L_in + L_out) // (2 * L_out)) for k in range(K)]
    qp = np.zeros(pad_lo + max(L_in, a[-1]) + pad_hi, np.int64)
    qp[pad_lo:pad_lo + L_in] = quantise(x, rules)
    lags = np.arange(-LAGS // 2, LAGS // 2)
    order = np.abs(lags) * 2 + (lags > 0)                   # the tie rule as a key: smallest |lag| first, then the negative one
    if rules.tie_reversed:
        order = order.max() - order
    idx = np.arange(N)
    deltas, p, sum_dist, edges = np.zeros(K, np.int16), np.zeros(K, np.int64), 0, 0
    p[0] = a[0]
    for k in range(1, K):
        t = (a[k - 1] if rules.template_nominal else int(p[k - 1])) + H
        tpl = qp[pad_lo + t + idx]
        cand = qp[pad_lo + a[k] + lags[:, None] + idx[None, :]]
        d = tpl[None, :] - cand
        if rules.q16_wrapping:
            D = ((d * d).sum(1) + 2 ** 31) % 2 ** 32 - 2 ** 31
        else:
            D = (d * d).sum(1)
        best = int(np.lexsort((order, D))[0])
        deltas[k] = lags[best]
        p[k] = a[k] + int(lags[best])
        sum_dist += int(D[best])
        edges += int(lags[best] in (-LAGS // 2, LAGS // 2 - 1))
    xp = np.zeros(qp.size, np.float64)
    xp[pad_lo:pad_lo + L_in] = x.astype(np.float64)
    m = np.arange(L_out)
    k, j = m // H, m % H
    prev = np.concatenate([[-H], p[:-1]])
    w = window(rules)
    w1 = (np.float32(1.0) - w).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (w[j].astype(np.float64) * xp[pad_lo + p[k] + j] + w1[j].astype(np.float64) * xp[pad_lo + prev[k] + H + j]).astype(np.float32)
    return dict(wav=y, wav_i16=s16_trunc(y), deltas=deltas, frames=K, edge_frames=edges, sum_dist=sum_dist & (2 ** 64 - 1),
                nonfinite=int(np.count_nonzero(~np.isfinite(x))))
