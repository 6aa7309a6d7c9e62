"""numpy restatement of ev_deliver's specification (include/evhip.h): every output byte.  y is tests/resample_oracle.py's float32 evaluation (the
specified summation order); the conversions are written with explicit float32 steps: the int16 rule with and without TPDF dither, the dither's
integer hash, G.711 mu-law and A-law, the 16-byte slot layout, peak and clipped."""
import numpy as np

import resample_oracle as ro

F32, S16, ULAW, ALAW = "f32", "s16", "ulaw", "alaw"
DTYPES = {F32: np.float32, S16: np.int16, ULAW: np.uint8, ALAW: np.uint8}
M32 = np.uint64(0xFFFFFFFF)


def h32(x):
    """The hash on uint32 with wraparound (held in uint64, masked after every product)."""
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def mix(seed, c):
    """mix(seed, c) for uint64 counters c: h(h((uint32)c + h(seed ^ (uint32)(c >> 32))) ^ seed)."""
    c = np.asarray(c, np.uint64)
    seed = np.uint64(int(seed) & 0xFFFFFFFF)
    lo, hi = c & M32, c >> np.uint64(32)
    return h32(h32((lo + h32(seed ^ hi)) & M32) ^ seed)


def dither(seed, n):
    """d[m], m < n: (float)((int)ua - (int)ub) * 2^-24 -- exact in float32, |d| < 1."""
    m = np.arange(n, dtype=np.uint64)
    ua = (mix(seed, np.uint64(2) * m) >> np.uint64(8)).astype(np.int64)
    ub = (mix(seed, np.uint64(2) * m + np.uint64(1)) >> np.uint64(8)).astype(np.int64)
    return ((ua - ub).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def to_s16(y, dithered=False, seed=0):
    """(s int16, clipped bool) of float32 y.  t = y * 32768 (one float32 product); without dither truncation toward zero, with it
    rint(t + d) (one float32 add, ties to even); clamped; NaN -> 0.  clipped: t (t + d) below -32768 or above 32767."""
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (y * np.float32(32768.0)).astype(np.float32)
        if dithered:
            t = (t + dither(seed, y.size)).astype(np.float32)
        clipped = (t < np.float32(-32768.0)) | (t > np.float32(32767.0))
        v = np.clip(np.where(np.isnan(t), np.float32(0.0), t), np.float32(-32768.0), np.float32(32767.0))
        q = np.rint(v) if dithered else np.trunc(v)
    return q.astype(np.int16), clipped


def ulaw(s):
    v = np.asarray(s, np.int16).astype(np.int32) >> 2
    neg = v < 0
    mask = np.where(neg, 0x7F, 0xFF)
    v = np.minimum(np.where(neg, -v, v), 8159) + 33
    ends = np.array([0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF])
    seg = (v[..., None] > ends).sum(axis=-1)
    byte = ((seg << 4) | ((v >> (seg + 1)) & 0xF)) ^ mask
    return np.where(seg >= 8, 0x7F ^ mask, byte).astype(np.uint8)      # v = 8192, the clipped magnitude: audioop's answer


def alaw(s):
    v = np.asarray(s, np.int16).astype(np.int32) >> 3
    neg = v < 0
    mask = np.where(neg, 0x55, 0xD5)
    v = np.where(neg, -v - 1, v)
    ends = np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF])
    seg = (v[..., None] > ends).sum(axis=-1)
    nib = np.where(seg < 2, (v >> 1) & 0xF, (v >> seg) & 0xF)
    return (((seg << 4) | nib) ^ mask).astype(np.uint8)


def convert(y, encoding, dithered=False, seed=0):
    """float32 y -> dict(data: the typed array, peak float32, clipped int)."""
    y = np.asarray(y, np.float32)
    fin = np.isfinite(y)
    peak = np.float32(np.abs(y[fin]).max()) if fin.any() else np.float32(0.0)
    if encoding == F32:
        return dict(data=y.copy(), peak=peak, clipped=0)
    s, clipped = to_s16(y, dithered, seed)
    data = s if encoding == S16 else ulaw(s) if encoding == ULAW else alaw(s)
    return dict(data=data, peak=peak, clipped=int(clipped.sum()))


def deliver(x, sr_in, sr_out, encoding, dithered=False, seed=0, taps=None):
    """One utterance (int16 or floating) -> dict(data, peak, clipped, y)."""
    if taps is None:
        h, up, down, _ = ro.design(sr_in, sr_out)
    else:
        h, (up, down) = np.asarray(taps, np.float32), ro.ratio(sr_in, sr_out)
    y = ro.resample32(x, h, up, down)
    out = convert(y, encoding, dithered, seed)
    out["y"] = y
    return out


def slots(n_samples, encoding):
    """byte_offsets (B + 1,) of utterances of n_samples each: every one starts on a 16-byte boundary."""
    es = np.dtype(DTYPES[encoding]).itemsize
    size = (np.asarray(n_samples, np.int64) * es + 15) // 16 * 16
    return np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
