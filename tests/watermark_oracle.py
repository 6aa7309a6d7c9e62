"""Float64 / integer restatement of ev_watermark and ev_watermark_detect (include/evhip.h): the pattern, the embed on denoise_oracle's STFT and
inverse, the quantised log band energies with the interval the forward bar allows each cell, and the integer correlation over the 128 offsets.
tests/test_watermark.py runs it alone; tests/test_gpu_watermark.py holds the device to it."""
import numpy as np

import deliver_oracle as dl
import denoise_oracle as do

N_FFT, HOP, BAND0, BAND_BINS, BANDS, TILE, PERIOD = 1024, 256, 20, 4, 48, 8, 16
CHIPS, OFFSETS, MAX_BITS, PILOT = PERIOD * BANDS, TILE * PERIOD, 16, 255
THRESHOLD = 6.25


def pattern(key, nbits=0, payload=0):
    """(signs int8 (768,), roles uint8 (768,)): chip i = 48 u + v, h = mix(key, i), sign = (h & 1) ? +1 : -1, role = (h >> 1) mod (2 nbits); a role
    < nbits is that payload bit and its sign is flipped where the bit is 1; every other role, and every chip at nbits = 0, is PILOT."""
    h = dl.mix(key, np.arange(CHIPS, dtype=np.uint64)).astype(np.int64)
    signs = np.where(h & 1, 1, -1).astype(np.int8)
    roles = np.full(CHIPS, PILOT, np.uint8)
    if nbits > 0:
        r = (h >> 1) % (2 * nbits)
        carries = r < nbits
        roles[carries] = r[carries]
        flip = carries & (((int(payload) >> np.where(carries, r, 0)) & 1) == 1)
        signs[flip] = -signs[flip]
    return signs, roles


def gains_f32(strength_db):
    """(a, 1 / a) as the float32 values the device holds: a = float32(10^(db / 20)) from float64, 1 / a one float32 division."""
    a = np.float32(10.0 ** (float(np.float32(strength_db)) / 20.0))
    return a, np.float32(1.0) / a


def gain_map(T, signs, strength_db, tile_shift=0, invert_band=None):
    """(T, n_bins) float64: the gain of every cell.  ``tile_shift`` (u off by that many tiles) and ``invert_band`` (one band's chips inverted)
    are the WRONG embeds of the negative controls."""
    a, ia = gains_f32(strength_db)
    s = np.asarray(signs, np.int64).reshape(PERIOD, BANDS).copy()
    if invert_band is not None:
        s[:, invert_band] = -s[:, invert_band]
    u = (np.arange(T) // TILE + tile_shift) % PERIOD
    g = np.ones((T, N_FFT // 2 + 1), np.float64)
    band = np.where(s[u] > 0, float(a), float(ia))                                 # (T, BANDS)
    g[:, BAND0:BAND0 + BAND_BINS * BANDS] = np.repeat(band, BAND_BINS, axis=1)
    return g


def embed64(wav, key, nbits=0, payload=0, strength_db=1.0, **wrong):
    """Steps 1 - 6 for one segment: 256 * (len // 256) float64 samples."""
    re, im = do.stft64(wav, N_FFT, HOP)
    g = gain_map(re.shape[0], pattern(key, nbits, payload)[0], strength_db, **wrong)
    return do.istft64(g * re, g * im, N_FFT, HOP)


def _q_of(E):
    """bits(float32 E) >> 17."""
    return (np.ascontiguousarray(E, np.float32).view(np.uint32) >> np.uint32(17)).astype(np.int64)


def band_q(wav, bar=0.0):
    """D1 - D4 in float64 for one segment -> (q, q_lo, q_hi) int64 (T, 48).  q_lo / q_hi: what q may be when every magnitude is off by up to
    ``bar`` times its frame's largest magnitude (the forward bar of the split-precision GEMM) and every fp32 operation of D1 - D3 by half an
    ulp (five in a chain: relative 5 x 2^-24)."""
    re, im = do.stft64(wav, N_FFT, HOP)
    mag = np.sqrt(re * re + im * im)
    peak = mag.max(axis=1, keepdims=True)
    lo_hi = []
    for sgn in (0.0, -1.0, 1.0):
        m = np.maximum(mag + sgn * bar * peak, 0.0)
        pk = np.maximum(peak + sgn * bar * peak, 0.0)
        rnd = 1.0 + sgn * 5.0 * 2.0 ** -24
        m2 = m * m
        E = m2[:, BAND0:BAND0 + BAND_BINS * BANDS].reshape(-1, BANDS, BAND_BINS).sum(axis=2)
        E = np.maximum(E, pk * pk * 2.0 ** -24) * rnd
        lo_hi.append(_q_of(E))
    return tuple(lo_hi)


def fold(q, q_lo=None, q_hi=None):
    """The key-independent half of D5: for every phase p < 8 the signs of X over the interior tiles, folded over the tile index modulo 16.
    -> dict(F (8, 16, 48) the sums of sign(X) over the tiles j = r mod 16, A likewise of |sign(X)|, and with q_lo / q_hi O: the count of OPEN
    cells -- those whose X interval is wider than a point and contains 0)."""
    q = np.asarray(q, np.int64)
    T = q.shape[0]
    F, A, O = (np.zeros((TILE, PERIOD, BANDS), np.int64) for _ in range(3))
    for p in range(TILE):
        nts = (T - p) // TILE if T >= p else 0
        if nts < 3:
            continue

        def tiles(x):
            return np.asarray(x, np.int64)[p:p + TILE * nts].reshape(nts, TILE, BANDS).sum(axis=1)
        D = tiles(q)
        X = 2 * D[1:-1] - D[:-2] - D[2:]
        S = np.sign(X)
        opened = np.zeros_like(S)
        if q_lo is not None:
            Dl, Dh = tiles(q_lo), tiles(q_hi)
            Xl, Xh = 2 * Dl[1:-1] - Dh[:-2] - Dh[2:], 2 * Dh[1:-1] - Dl[:-2] - Dl[2:]
            opened = ((Xl < Xh) & (Xl <= 0) & (Xh >= 0)).astype(np.int64)
        r = np.arange(1, nts - 1) % PERIOD
        np.add.at(F[p], r, S)
        np.add.at(A[p], r, np.abs(S))
        np.add.at(O[p], r, opened)
    return dict(F=F, A=A, O=O)


def better(Ca, na, sa, Cb, nb, sb):
    """D6: is offset a the better answer?"""
    if (Ca > 0) != (Cb > 0):
        return Ca > 0
    if Ca > 0:
        l, r = int(Ca) * int(Ca) * int(nb), int(Cb) * int(Cb) * int(na)
        if l != r:
            return l > r
    return sa < sb


def correlate(folded, key, nbits=0):
    """D5 - D7 from ``fold``'s sums: dict(offset, C, n, bit_C (16,), bit_n (16,), z, present, bits, payload, C_all (128,), n_all (128,), open:
    the count of open pilot cells at the reported offset, bit_open (16,))."""
    signs, roles = pattern(key, nbits, 0)
    s2, r2 = signs.astype(np.int64).reshape(PERIOD, BANDS), roles.reshape(PERIOD, BANDS)
    pil = np.where(r2 == PILOT, s2, 0)
    C_all, n_all = np.zeros(OFFSETS, np.int64), np.zeros(OFFSETS, np.int64)
    for k in range(PERIOD):
        rolled = np.roll(pil, k, axis=0)                  # rolled[r] = pil[(r - k) mod 16]: tile j = r carries the chips of u = (j - k) mod 16
        C_all[TILE * k:TILE * k + TILE] = (folded["F"] * rolled[None]).sum(axis=(1, 2))
        n_all[TILE * k:TILE * k + TILE] = (folded["A"] * np.abs(rolled)[None]).sum(axis=(1, 2))
    best = 0
    for s in range(1, OFFSETS):
        if better(C_all[s], n_all[s], s, C_all[best], n_all[best], best):
            best = s
    p, k = best % TILE, best // TILE
    chips, rl = np.roll(s2, k, axis=0), np.roll(r2, k, axis=0)
    bit_C, bit_n, bit_open = (np.zeros(MAX_BITS, np.int64) for _ in range(3))
    for b in range(nbits):
        sel = rl == b
        bit_C[b], bit_n[b], bit_open[b] = (folded["F"][p] * chips)[sel].sum(), folded["A"][p][sel].sum(), folded["O"][p][sel].sum()
    C, n = int(C_all[best]), int(n_all[best])
    z = C / np.sqrt(n) if n > 0 else 0.0
    bits = [int(c < 0) for c in bit_C[:nbits]]
    return dict(offset=best, C=C, n=n, bit_C=bit_C, bit_n=bit_n, z=float(z), present=bool(z >= THRESHOLD), bits=bits,
                payload=sum(b << j for j, b in enumerate(bits)), C_all=C_all, n_all=n_all,
                open=int((folded["O"][p] * (np.roll(pil, k, axis=0) != 0)).sum()), bit_open=bit_open)


def detect(wav, key, nbits=0, bar=0.0):
    """One segment -> ``correlate``'s dict (with ``bar`` > 0 its open counts are those of the intervals)."""
    q, lo, hi = band_q(wav, bar)
    return correlate(fold(q, lo, hi) if bar > 0 else fold(q), key, nbits)


# ---------------------------------------------------------------------------------------------------------------------------------- signals
def speech_like(seed, n, sr=16000):
    """The recipe of tests/test_gpu_stretch.py's ``_speech_like``: a few harmonics with a drifting pitch and a 5 Hz tremolo, plus a little noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    f0 = 110.0 + 40.0 * np.sin(2 * np.pi * t / 9000.0)
    ph = 2 * np.pi * np.cumsum(f0) / sr
    x = sum(a * np.sin(h * ph) for h, a in ((1, 0.4), (2, 0.2), (3, 0.1), (5, 0.05)))
    return (x * (0.6 + 0.4 * np.sin(2 * np.pi * t / 3000.0)) + 0.01 * rng.standard_normal(n)).astype(np.float32)


def harmonic_rich(seed, n, sr=16000, vibrato_hz=2.0, vibrato_period=32000.0, tremolo=0.3, tremolo_period=24000.0):
    """27 harmonics of 130 Hz at -6 dB per octave with random phases -- every band of the mark holds a harmonic or its leakage -- a vibrato of
    +-2 Hz over 2 s, a tremolo of 0.3 over 1.5 s and breath noise.  The slow modulation is a CHOICE: the detector's contrast X is a second
    difference over tiles of 0.128 s, and a tremolo or a pitch sweep at the syllable rate (the keywords) moves the band energies by far more
    than 1 dB on that scale; tools/watermark_robustness.py records what such a signal does to z."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    f0 = 130.0 + vibrato_hz * np.sin(2 * np.pi * t / vibrato_period + seed)
    ph = 2 * np.pi * np.cumsum(f0) / sr
    x = sum((0.4 / h) * np.sin(h * ph + rng.uniform(0, 2 * np.pi)) for h in range(1, 28))
    return (x * ((1 - tremolo) + tremolo * np.sin(2 * np.pi * t / tremolo_period)) + 0.01 * rng.standard_normal(n)).astype(np.float32)


def ulaw_decode(u):
    """G.711 mu-law bytes -> int16 (the decoder of ITU-T G.711: bias 0x84, 3-bit exponent, 4-bit mantissa)."""
    u = ~np.asarray(u, np.uint8)
    t = (((u & 0x0F).astype(np.int32) << 3) + 0x84) << ((u & 0x70) >> 4).astype(np.int32)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)
