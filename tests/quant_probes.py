"""Probe inputs for the activation quantisers (MX fp4 plane sets, E5M2 operands) and an independent reference of the format (numpy only, no GPU).

The exact lattices of tests/exact_lattice.py are built so that no quantiser ever rounds; the plane tests on ``randn`` data meet a close decision only by
accident.  This module builds the inputs on which every decision of emotivoice_amd/mxfp4.py IS close: block maxima at every mantissa that could move the
scale, elements on every rounding threshold of the fp4 grid and on both of its representable neighbours, the fp16 split at its ties, E5M2 at its ties.

Domain (every probe is inside it; ``in_domain`` states it, tests/test_quant_probes.py asserts it): finite fp32 values, |v| < 65520 (the fp16 hi part is
finite), and v == 0 or |v| >= 2^-100.  Non-finite values, fp32 denormals and the E8M0 clamp at 254 are outside what the engine produces and outside this set.

Probe blocks: ``BLOCKS`` [n][32] fp32, one scale block per row: one PIN that fixes the block maximum of the plane the block aims at, up to 31 probes, zeros.
  hi-plane blocks  every value is an fp16 number (the remainder plane is all zero, scale byte 1).  Pin = m 2^E with the fp16 mantissas m of ``PIN_NAMES``
                   and the binades ``HI_BINADES`` (the last one fp16-subnormal); the probes are t 2^(E-2) for the seven thresholds t and the fp16 neighbours
                   of each: every tie is an fp16 number.
  lo-plane blocks  v = H + lo with H = 1.5 2^(L+12) (the middle of an fp16 binade: |lo| < 2^(L+1) is below half an ulp of H on both sides, so
                   fp16(v) == H), lo = +-m 2^L for the pin, +-t 2^(L-2) and the neighbours one fp32 ulp of v away for the probes.  A remainder of a value
                   with a nonzero hi part has at most 12 significant bits, so the finest mantissa step of such a pin is 2^-11 (2^-12 under the subnormal
                   H); the blocks with H == 0 (|v| < 2^-25: the whole value is the remainder) carry the full fp32 step 2^-23.
  Probes larger than the pin are left out of a block (they would be the maximum); the saturation band (6, 8) x scale is probed in the blocks whose pin is
  2 - ulp.  Every family exists with all signs positive, all negative and alternating (lo-plane: the sign of lo; and once more with v negated), the pin at
  elements 0, 7, 8, 31, 16, 23 in turn, the probes spread over the four 8-element groups whose lanes must agree on the maximum.
  Specials: an all-zero block, blocks whose only nonzero element is -pin, the split's own ties (half an fp16 ulp above an even and above an odd fp16 number,
  4 - 6 2^-12, +-0, the subnormal range, the largest value of the domain).

Per element: ``THR`` (0..6 = index into THRESHOLDS, 7 = saturation band, -1 = none), ``SIDE`` (-1 / 0 / +1: below / on / above the threshold), per block:
``PLANE`` (0 hi, 1 lo, -1 special), ``PIN`` (index into PIN_NAMES or -1), ``PINPOS``, ``KIND``.

E5M2: ``E5_HI`` (fp16 hi parts whose low byte is 0x00 / 0x7f / 0x80 / 0xff, even and odd top bytes, normal and subnormal, both signs) and ``E5_V`` (fp32
values whose remainder, times 2^11, sits on a tie of the E5M2 grid or one fp32 ulp of v beside it: a normal binade, the lowest normal binade 2^-14, the
subnormal band, remainders that round to zero, the largest remainder of an fp16-normal value) with ``E5_TAG`` = (band, tie, side, sign of lo).

The reference (``ref_*``) shares no code with mxfp4.py: the scale byte from frexp of the block maximum, the fp4 code and the E5M2 byte by exhaustive
search for the nearest grid value in fp64 (a tie to the even code / byte), the fp16 split by rint on the binade's quantum.

The last section (``pair_*``) is not part of that reference: it states, WITH the host functions of mxfp4.py, what the fused C = 32 pair kernels must write to
out32 when their convs are identities, which probes that route carries exactly, and which codes it can see (tests/test_gpu_quant_edges.py)."""
from __future__ import annotations

import numpy as np

THRESHOLDS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
SAT = 7
PIN_NAMES = ("1", "1+ulp", "1.5-ulp", "1.5", "1.75", "2-ulp")
HI_BINADES = (-14, -13, -3, 0, 5, 13, -16)          # -16: an fp16-subnormal pin (quantum 2^-24: mantissa step 2^-8)
LO_BINADES = tuple(e - 12 for e in HI_BINADES[:-1]) + (-27,)          # the remainders under those hi parts; -27 under the subnormal H = 1.5 2^-16
LO_ZERO_HI = (-27, -40, -90)          # binades of blocks with H == 0
PIN_POSITIONS = (0, 7, 8, 31, 16, 23)
DOMAIN_MAX, DOMAIN_MIN = 65520.0, 2.0 ** -100


def in_domain(v):
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    return bool(np.all(np.isfinite(v) & (a < DOMAIN_MAX) & ((a == 0) | (a >= DOMAIN_MIN))))


def pin_mantissas(u):
    return (1.0, 1.0 + u, 1.5 - u, 1.5, 1.75, 2.0 - u)


def _f16_next(c, up):
    return float(np.nextafter(np.float16(c), np.float16(np.inf if up else -np.inf)))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the independent reference
_FP4_GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def ref_scale_byte(amax):
    """E8M0 byte of 2^(floor(log2 amax) - 2), from frexp; an all-zero block gets 1"""
    amax = np.asarray(amax, np.float64)
    m, e = np.frexp(amax)          # amax = m 2^e, m in [.5, 1): floor(log2 amax) = e - 1
    return np.where(amax == 0, 1, np.clip(e - 1 - 2 + 127, 1, 254)).astype(np.uint8)


def _nearest(y, grid):
    """index of the grid value nearest to y >= 0 (fp64, exhaustive search); a tie goes to the even index"""
    d = np.abs(y[..., None] - grid)
    i = d.argmin(-1)          # the first minimum: the lower of two tied neighbours
    nxt = np.minimum(i + 1, len(grid) - 1)
    tie = (np.take_along_axis(d, nxt[..., None], -1)[..., 0] == np.take_along_axis(d, i[..., None], -1)[..., 0]) & (nxt != i)
    return np.where(tie & (i % 2 == 1), nxt, i)


def ref_quantize(part):
    """part [n][32] (one plane's values, fp32) -> (codes [n][32] with the sign in bit 3, scale bytes [n])"""
    p = np.asarray(part, np.float64)
    sb = ref_scale_byte(np.abs(p).max(-1))
    y = np.abs(p) / np.ldexp(1.0, sb.astype(np.int64) - 127)[:, None]
    c = _nearest(y, _FP4_GRID).astype(np.uint8)
    return (c | (np.signbit(p).astype(np.uint8) << 3)).astype(np.uint8), sb


def ref_split(v):
    """fp32 -> (nearest fp16 number, ties to even, as fp64; exact remainder as fp64) inside the domain"""
    v = np.asarray(v, np.float64)
    _, e = np.frexp(np.where(v == 0, 1.0, v))
    q = np.ldexp(1.0, np.maximum(e - 1, -14) - 10)          # the quantum of v's fp16 binade (subnormals share 2^-24)
    hi = np.rint(v / q) * q          # rint: half to even; v / q is exact (a power of two)
    hi = np.where(np.signbit(v) & (hi == 0), -0.0, hi)
    return hi, v - hi


def _e5m2_table():
    vals = np.empty(128)
    for b in range(128):
        e, m = b >> 2, b & 3
        vals[b] = m / 4.0 * 2.0 ** -14 if e == 0 else ((1 + m / 4.0) * 2.0 ** (e - 15) if e < 31 else np.inf)
    return vals[:124]          # 0x7c .. 0x7f: infinity and NaNs


_E5_GRID = _e5m2_table()


def ref_e5m2_nearest(y):
    """fp64 -> E5M2 byte of the nearest finite value, ties to the even byte, saturating"""
    y = np.asarray(y, np.float64)
    return (_nearest(np.abs(y), _E5_GRID) | (np.signbit(y).astype(np.int64) << 7)).astype(np.uint8)


def ref_e5m2_trunc(h):
    """fp16-representable values -> the E5M2 byte of the largest grid magnitude <= |h| (truncation)"""
    h = np.asarray(h, np.float64)
    i = (np.abs(h)[..., None] >= _E5_GRID).sum(-1) - 1
    return (i | (np.signbit(h).astype(np.int64) << 7)).astype(np.uint8)


def ref_e5m2_lo(lo):
    return ref_e5m2_nearest(np.asarray(lo, np.float64) * 2048.0)


def fold_fp4(c):
    """-0 (code 8) onto +0"""
    c = np.asarray(c, np.uint8)
    return np.where(c == 8, 0, c)


def fold_e5(b):
    b = np.asarray(b, np.uint8)
    return np.where(b == 0x80, 0, b)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the probe blocks
class _Builder:
    def __init__(self):
        self.blocks, self.thr, self.side, self.plane, self.pin, self.pinpos, self.kind = [], [], [], [], [], [], []

    def add(self, values, thr, side, plane, pin, pinpos, kind):
        assert len(values) == 32
        self.blocks.append(np.asarray(values, np.float64))
        self.thr.append(np.asarray(thr, np.int8))
        self.side.append(np.asarray(side, np.int8))
        self.plane.append(plane)
        self.pin.append(pin)
        self.pinpos.append(pinpos)
        self.kind.append(kind)

    def family(self, probes, pin_value, pin_index, plane, kind, signs, compose):
        """probes: [(magnitude, thr, side)]; one block per 31 of them.  signs "pos" / "neg" / "mix"; compose(magnitude, sign, element) -> the fp64 value"""
        probes = [p for p in probes if p[0] <= pin_value]
        for first in range(0, len(probes), 31):
            chunk = probes[first:first + 31]
            pos = PIN_POSITIONS[len(self.blocks) % len(PIN_POSITIONS)]
            order = [e for e in ((5 * i + 3) % 32 for i in range(32)) if e != pos]          # consecutive probes land in different 8-element groups
            sg = lambda e: {"pos": 1.0, "neg": -1.0, "mix": -1.0 if e % 2 else 1.0}[signs]          # noqa: E731
            v, t, s = np.zeros(32), np.full(32, -1), np.zeros(32)
            v[pos] = compose(pin_value, sg(pos), pos)
            for (mag, th, sd), e in zip(chunk, order):
                v[e], t[e], s[e] = compose(mag, sg(e), e), th, sd
            self.add(v, t, s, plane, pin_index, pos, "%s %s" % (kind, signs))


def _threshold_probes(scale, below, above, with_sat):
    """[(magnitude, thr, side)] around every threshold times ``scale``; below / above give the representable neighbours"""
    out = []
    for i, t in enumerate(THRESHOLDS):
        c = t * scale
        out += [(below(c), i, -1), (c, i, 0), (above(c), i, 1)]
    if with_sat:
        out += [(6.0 * scale, SAT, 0), (above(6.0 * scale), SAT, 0), (6.5 * scale, SAT, 0), (7.0 * scale, SAT, 0), (7.5 * scale, SAT, 0)]
    return out


def _build_blocks():
    b = _Builder()
    # hi-plane blocks: fp16 values
    for E in HI_BINADES:
        u = 2.0 ** -10 if E >= -14 else 2.0 ** (-24 - E)
        for pi, m in enumerate(pin_mantissas(u)):
            probes = _threshold_probes(2.0 ** (E - 2), lambda c: _f16_next(c, False), lambda c: _f16_next(c, True), pi == 5)
            for signs in ("pos", "neg", "mix"):
                b.family(probes, m * 2.0 ** E, pi, 0, "hi 2^%d" % E, signs, lambda mag, sg, e: sg * mag)
    # lo-plane blocks under a nonzero hi part
    for L in LO_BINADES:
        H = 1.5 * 2.0 ** (L + 12) if L != -27 else 1.5 * 2.0 ** -16
        g = 2.0 ** (int(np.floor(np.log2(H))) - 23)          # one fp32 ulp of v = H + lo
        u = g / 2.0 ** L
        for pi, m in enumerate(pin_mantissas(u)):
            probes = _threshold_probes(2.0 ** (L - 2), lambda c: c - g, lambda c: c + g, pi == 5)
            for signs in ("pos", "neg", "mix"):
                for mirror in (1.0, -1.0):
                    b.family(probes, m * 2.0 ** L, pi, 1, "lo 2^%d under %s%g" % (L, "-" if mirror < 0 else "", H), signs,
                             lambda mag, sg, e, H=H, mirror=mirror: mirror * (H + sg * mag))
    # lo-plane blocks with a zero hi part: the whole value is the remainder
    f32 = lambda c, up: float(np.nextafter(np.float32(c), np.float32(np.inf if up else -np.inf)))          # noqa: E731
    for L in LO_ZERO_HI:
        for pi, m in enumerate(pin_mantissas(2.0 ** -23)):
            probes = _threshold_probes(2.0 ** (L - 2), lambda c: f32(c, False), lambda c: f32(c, True), pi == 5)
            for signs in ("pos", "neg", "mix"):
                b.family(probes, m * 2.0 ** L, pi, 1, "lo 2^%d, hi == 0" % L, signs, lambda mag, sg, e: sg * mag)
    # specials
    none, zero = np.full(32, -1), np.zeros(32)
    b.add(zero, none, zero, -1, -1, -1, "all zero")
    for pos, val in ((5, -1.5), (31, -(1.5 + 1.5 * 2.0 ** -12)), (0, -1.75 * 2.0 ** -40), (8, -(1.0 + 2.0 ** -10) * 2.0 ** -14)):
        v = zero.copy()
        v[pos] = val
        b.add(v, none, zero, -1, -1, pos, "only -pin")
    split = []
    for E in (-14, -3, 0, 5, 15):
        s, h = 2.0 ** E, 2.0 ** (E - 11)          # half an fp16 ulp of the binade
        split += [s + h, s * (1 + 2.0 ** -10) + h, s * (1 + 2.0 ** -9) + h, s * (1 + 3 * 2.0 ** -10) + h, s * (2 - 2.0 ** -10) - h,
                  s + h + s * 2.0 ** -23, s + h - s * 2.0 ** -23, s * (1 + 2.0 ** -10) + h + s * 2.0 ** -23, s * (1 + 2.0 ** -10) + h - s * 2.0 ** -23]
    split += [4 - 6 * 2.0 ** -12, 2.0 ** -10 * (4 - 6 * 2.0 ** -12), 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -25 * (1 + 2.0 ** -23), 2.0 ** -25 * (1 - 2.0 ** -24),
              2.0 ** -24 + 2.0 ** -25, 2 * 2.0 ** -24 + 2.0 ** -25, 5 * 2.0 ** -24 + 2.0 ** -25, 1023 * 2.0 ** -24 + 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25,
              65504.0, 65504.0 + 16 - 2.0 ** -8, 65519.99609375, 2.0 ** -100, 2.0 ** -26]
    split = [s * v for v in split for s in (1.0, -1.0)] + [0.0, -0.0]
    for first in range(0, len(split), 32):
        chunk = split[first:first + 32]
        b.add(chunk + [0.0] * (32 - len(chunk)), none, zero, -1, -1, -1, "split")
    blocks = np.array(b.blocks)
    out = blocks.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), blocks), "a probe is not an fp32 number"
    return (out, np.array(b.thr, np.int8), np.array(b.side, np.int8), np.array(b.plane, np.int8), np.array(b.pin, np.int8), np.array(b.pinpos, np.int8),
            list(b.kind))


BLOCKS, THR, SIDE, PLANE, PIN, PINPOS, KIND = _build_blocks()
NONNEG = ~np.signbit(BLOCKS).any(1)          # the blocks the fused pairs can take (their leaky-relu slope is not dyadic)


def describe(block, element=None):
    s = "block %d (%s, pin %s at %d)" % (block, KIND[block], PIN_NAMES[PIN[block]] if PIN[block] >= 0 else "-", PINPOS[block])
    if element is not None:
        t = THR[block, element]
        s += " element %d = %r" % (element, float(BLOCKS[block, element]))
        if t >= 0:
            s += " (saturation band)" if t == SAT else " (threshold %g, side %+d)" % (THRESHOLDS[t], SIDE[block, element])
    return s


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# E5M2
E5_BANDS = ("normal 2^-1", "normal 2^-5", "lowest normal 2^-14", "subnormal", "subnormal, hi == 0", "to zero", "largest")


def _build_e5():
    hi = []
    for top in (0x3c, 0x3d, 0x04, 0x05, 0x00, 0x01, 0x7a, 0x7b, 0x30, 0x57):
        for low in (0x00, 0x7f, 0x80, 0xff):
            for sign in (0, 0x8000):
                hi.append(sign | (top << 8) | low)
    e5_hi = np.array(hi, np.uint16).view(np.float16)
    vals, tags = [], []

    def probe(H, y, band, tie, g):
        """remainders y 2^-11 (+-, and one ulp g of v on both sides) on top of the hi part H"""
        for sign in (1.0, -1.0):
            for side in (-1, 0, 1):
                lo = sign * (y / 2048.0 + side * g)
                vals.append(H + lo)
                tags.append((band, tie, side, int(sign)))

    for band, H, e in ((0, 1.5, -1), (1, 1.5, -5), (2, 1.5 * 2.0 ** -13, -14)):
        g = 2.0 ** (int(np.floor(np.log2(H))) - 23)
        for k in range(4):
            probe(H, (1 + (2 * k + 1) / 8.0) * 2.0 ** e, band, k, g)
    for k in range(4):
        probe(1.5 * 2.0 ** -14, (k + 0.5) * 2.0 ** -16, 3, k, 2.0 ** -37)
        y = (k + 0.5) * 2.0 ** -16
        probe(0.0, y, 4, k, 2.0 ** (int(np.floor(np.log2(y / 2048.0))) - 23))
    for i, (H, lo) in enumerate(((1.5 * 2.0 ** -14, 2.0 ** -31), (1.5 * 2.0 ** -14, 2.0 ** -37), (0.0, 2.0 ** -60), (0.0, 2.0 ** -29), (1.5, 2.0 ** -23))):
        for sign in (1.0, -1.0):
            vals.append(H + sign * lo)
            tags.append((5, i, 0, int(sign)))
    for i, H in enumerate((65504.0, 49152.0, 32768.0 + 32)):
        for sign in (1.0, -1.0):
            vals.append(H + sign * (16 - 2.0 ** -8))
            tags.append((6, i, 0, int(sign)))
    v = np.array(vals)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v), "an E5M2 probe is not an fp32 number"
    return e5_hi, out, tags


E5_HI, E5_V, E5_TAG = _build_e5()


def e5_rows():
    """the non-negative E5M2 probes as [n][32] rows (C = 32 activations), zero padded: first the remainder probes E5_V, then (from a fresh row on) the hi-part
    probes E5_HI -> (rows fp32, index into E5_V per element or -1, index into E5_HI per element or -1)"""
    iv = [i for i, v in enumerate(E5_V) if not np.signbit(v)]
    ih = [i for i, h in enumerate(E5_HI) if not np.signbit(h)]
    nv, nh = (len(iv) + 31) // 32, (len(ih) + 31) // 32
    rows, src_v, src_h = np.zeros((nv + nh, 32), np.float32), np.full((nv + nh, 32), -1), np.full((nv + nh, 32), -1)
    for j, i in enumerate(iv):
        rows[j // 32, j % 32], src_v[j // 32, j % 32] = E5_V[i], i
    for j, i in enumerate(ih):
        rows[nv + j // 32, j % 32], src_h[nv + j // 32, j % 32] = np.float32(E5_HI[i]), i
    return rows, src_v, src_h


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The fused C = 32 pairs: their two quantisers (of the fp32 input x, of the intermediate xt in LDS) show only through out32.  A conv whose weight is the
# identity at the centre tap with value 1 + 2^-13 (hi part 1, remainder 2^-13, both exact in the weight planes) turns an operand row u into
#     u_h + 2^-13 Q(u_h) + Q(u_l)          (fp16 MFMA, then the two cross terms, in this order)
# per element, so a wrong code in either operand plane changes the fp32 result -- provided the sum is an fp32 number at every step.  Where it is not, the
# element is DROPPED (not compared): a condition on the input, not a tolerance.  The expected values come from the host functions (mxfp4.py) in fp64.
PAIR_W_LO = 2.0 ** -13


def _exact_add(x, y):
    """x + y in fp64 -> (sum, whether the sum is exact AND an fp32 number)"""
    s = x + y
    big, small = np.where(np.abs(x) >= np.abs(y), x, y), np.where(np.abs(x) >= np.abs(y), y, x)
    return s, ((s - big) == small) & (s.astype(np.float32).astype(np.float64) == s)


def pair_operand_parts(u, fmt):
    """(hi, Q(hi), Q(lo)) of an activation u [n][32] fp32 as the pair kernel of format fmt ("fp4" / "e5m2") reads them, by the host functions, fp64"""
    from emotivoice_amd import mxfp4
    hi, lo = mxfp4.split_hi_lo(u)
    if fmt == "e5m2":
        qh, ql = mxfp4.e5m2_decode(mxfp4.e5m2_hi_codes(hi)), mxfp4.e5m2_lo_decode(mxfp4.e5m2_lo_codes(lo))
    else:
        qh, ql = (mxfp4.dequantize(*mxfp4.quantize(p, 32), 32) for p in (hi, lo))
    return hi.astype(np.float64), qh.astype(np.float64), ql.astype(np.float64)


PAIR_ROUTES = ("intermediate", "input_lo", "input_hi")


def pair_expected(u, fmt, route, alt=None):
    """out32 of the pair (out_scale 1, zero b2) for an operand u [n][32] >= 0 -> (expected fp64 [n][32], compared mask).
    route "intermediate": x = 0, b1 = u, conv2 = the identity of weight 1 + 2^-13: the intermediate IS u and the result is u_h + 2^-13 Q(u_h) + Q(u_l).
    The input quantiser is followed by the intermediate's, which would round the sum above again and could hide a wrong code; so its two planes are read by
    two launches, both with conv2 = MINUS the identity (weight exactly -1.0: the kernels add their residual, which is always x itself, so the result is a small
    difference that stays an fp32 number where a sum would lose the last bit of every remainder):
    route "input_lo": conv1 = the identity of weight exactly 1.0: t = u_h + Q(u_l), whose remainder Q(u_l) is on the quantiser's own grid (the second
      quantisation is lossless): the result is u - (t_h + Q(t_l)) = u_l - Q(u_l);
    route "input_hi": conv1 = the identity of weight 1 + 2^-13: t = u_h + 2^-13 Q(u_h) + Q(u_l); for a probe that is an fp16 number (every hi-plane block, the
      E5M2 hi-part probes) t's remainder is 2^-13 Q(u_h), again on the grid, and the result is -2^-13 Q(u_h).
    alt = (Q(u_h), Q(u_l)) replaces what the host functions give for u's quantiser: what a kernel with other codes would produce (pair_survival)."""
    u = np.ascontiguousarray(u, np.float32)
    assert not np.signbit(u).any() and route in PAIR_ROUTES          # the pairs' slope 0.1 is not dyadic: no leaky-relu may act
    a, qh, ql = pair_operand_parts(u, fmt)
    if alt is not None:
        qh, ql = alt
    b = (0.0 if route == "input_lo" else PAIR_W_LO) * qh
    ab, ok1 = _exact_add(a, b)
    _, ok2 = _exact_add(a, ql)
    _, ok3 = _exact_add(b, ql)
    v, ok4 = _exact_add(ab, ql)
    ok = ok1 & ok2 & ok3 & ok4          # every partial sum, in any order, is exact and an fp32 number
    if route == "intermediate":
        return v, ok
    ok = ok & (np.abs(v) < DOMAIN_MAX)
    t = np.where(ok, v, 0.0).astype(np.float32)          # (exact where ok)
    if fmt == "fp4":          # the block scales of t come from the REAL intermediate, dropped elements included: only blocks without one are compared
        ok = ok & ok.all(1, keepdims=True)
    th, _, tl = pair_operand_parts(t, fmt)
    c2, ok5 = _exact_add(th, tl)
    out, ok6 = _exact_add(u.astype(np.float64), -c2)
    return out, ok & ok5 & ok6


def pair_feed(u, fmt, route):
    """u as it is fed on ``route``: on the input routes an element whose intermediate t would leave the domain (|t| >= 65520: its fp16 hi part is infinite,
    and an infinity times a zero weight is a NaN in every output of the rows around it) is replaced by zero; pair_survival counts it as dropped"""
    u = np.ascontiguousarray(u, np.float32)
    if route == "intermediate":
        return u
    a, qh, ql = pair_operand_parts(u, fmt)
    t = a + (0.0 if route == "input_lo" else PAIR_W_LO) * qh + ql
    return np.where(np.abs(t) < DOMAIN_MAX, u, np.float32(0.0)).astype(np.float32)


def _other_fp4(part):
    """Q4 of a plane with every on-tie element sent to the OTHER neighbour of its tie (what a quantiser with > and >= swapped gives) -> fp64"""
    p = np.asarray(part, np.float64)
    codes, sb = ref_quantize(p)
    sc = np.ldexp(1.0, sb.astype(np.int64) - 127)[:, None]
    y = np.abs(p) / sc
    mag = (codes & 7).astype(np.int64)
    for i, t in enumerate(THRESHOLDS):
        mag = np.where(y == t, np.where(mag == i, i + 1, i), mag)
    return np.where(np.signbit(p), -1.0, 1.0) * _FP4_GRID[mag] * sc


def pair_survival(fmt, route):
    """for the non-negative probe blocks (fp4) / the E5M2 probe rows on one route -> dict(blocks, dropped_blocks: blocks with ANY element not compared,
    elements, dropped_elements, thresholds: {key: on-tie probes that are compared AND whose expected value changes when the probe's code goes to the other
    neighbour}); keys (plane, threshold index) for fp4, ("lo", band, tie) / ("hi", low byte) for E5M2"""
    from emotivoice_amd import mxfp4
    thr = {}
    if fmt == "fp4":
        idx = np.flatnonzero(NONNEG)
        fed = BLOCKS[idx]
        u = pair_feed(fed, fmt, route)
        want, ok = pair_expected(u, fmt, route)
        hi, lo = mxfp4.split_hi_lo(u)
        _, qh, ql = pair_operand_parts(u, fmt)
        for plane in (0, 1):          # one plane's codes changed at a time
            other, ok_o = pair_expected(u, fmt, route, alt=(_other_fp4(hi), ql) if plane == 0 else (qh, _other_fp4(lo)))
            seen = ok & ok_o & (other != want)
            for t in range(7):
                hit = (PLANE[idx] == plane)[:, None] & (THR[idx] == t) & (SIDE[idx] == 0)
                thr[(plane, t)] = int((hit & seen).sum())
    else:
        fed, src_v, src_h = e5_rows()
        u = pair_feed(fed, fmt, route)
        want, ok = pair_expected(u, fmt, route)
        a, qh, ql = pair_operand_parts(u, fmt)
        hi, lo = mxfp4.split_hi_lo(u)
        up = lambda codes: mxfp4.e5m2_decode(np.minimum((codes & 0x7f) + 1, 0x7b) | (codes & 0x80)).astype(np.float64)          # noqa: E731  (the next byte up in magnitude)
        other, ok_o = pair_expected(u, fmt, route, alt=(qh, up(mxfp4.e5m2_lo_codes(lo)) / 2048.0))
        seen = ok & ok_o & (other != want)
        for band in range(5):
            for tie in range(4):
                hit = np.array([[s >= 0 and E5_TAG[s][:3] == (band, tie, 0) for s in row] for row in src_v])
                thr[("lo", band, tie)] = int((hit & seen).sum())
        other, ok_o = pair_expected(u, fmt, route, alt=(up(mxfp4.e5m2_hi_codes(hi)), ql))
        seen = ok & ok_o & (other != want)
        low = E5_HI.view(np.uint16) & 0xff
        for byte in (0x00, 0x7f, 0x80, 0xff):
            hit = np.array([[s >= 0 and low[s] == byte for s in row] for row in src_h])
            thr[("hi", byte)] = int((hit & seen).sum())
    nz = fed != 0
    lost = (~ok | (u != fed)) & nz
    return dict(blocks=len(u), dropped_blocks=int(lost.any(1).sum()), dropped_elements=int(lost.sum()), elements=int(nz.sum()), thresholds=thr)


def pair_identity(k, value):
    """[32][k][32] GEMM-layout weight: ``value`` at the centre tap on the diagonal"""
    w = np.zeros((32, k, 32), np.float32)
    n = np.arange(32)
    w[n, (k - 1) // 2, n] = np.float32(value)
    assert float(w[0, (k - 1) // 2, 0]) == value
    return w
