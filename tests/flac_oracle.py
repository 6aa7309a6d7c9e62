"""numpy restatement of ev_flac (include/evhip.h) and an independent FLAC decoder.

`encode` follows the specification byte for byte: fixed block size, CONSTANT / VERBATIM / FIXED 0..4 subframes, the exact bit-cost search over
partition orders and Rice parameters, method-0 residual coding, CRC-8 and CRC-16.  `decode` is written from the format, not from the encoder: it
also reads what the encoder never writes (5-bit Rice parameters, escape partitions, frame numbers of up to 6 bytes, LPC subframes are refused)
and checks both CRCs, the frame numbering, the header codes against STREAMINFO, the sample count and the min / max frame sizes.
"""
import numpy as np

SAMPLE_RATE_CODE = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}
BLOCK_SIZES = (256, 512, 1024, 2048, 4096)
FIXED_COEF = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))
KIND_CONSTANT, KIND_VERBATIM, KIND_FIXED = 0, 1, 8


# ---------------------------------------------------------------------------------------------------------------- CRCs
def _crc_table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    tab = []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        tab.append(c)
    return tab


_CRC8_TAB, _CRC16_TAB = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c = _CRC8_TAB[c ^ b]
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16_TAB[(c >> 8) ^ b]
    return c


# ---------------------------------------------------------------------------------------------------------------- conversion
def to_i16(x_f32, convert=0) -> np.ndarray:
    """t = x * 32768 in fp32; NaN -> 0; truncation toward zero, saturated to int32; convert 0 keeps the low 16 bits, convert 1 clamps."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(x_f32, np.float32) * np.float32(32768.0)
    t = np.where(np.isnan(t), np.float32(0), t)
    v = np.clip(np.trunc(t.astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
    if convert == 0:
        return (v & 0xFFFF).astype(np.uint16).view(np.int16)
    if convert == 1:
        return np.clip(v, -32768, 32767).astype(np.int16)
    raise ValueError("convert must be 0 (wrap) or 1 (clamp)")


# ---------------------------------------------------------------------------------------------------------------- encoder
def _bits_of(value, nbits):
    return [(value >> (nbits - 1 - i)) & 1 for i in range(nbits)]


def _utf8_number(v):
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):      # n bytes carry 5 n + 1 bits (n = 2 .. 6)
        n += 1
    out = [((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))]
    for i in range(n - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * i)) & 0x3F))
    return bytes(out)


def residual(x, o):
    """The o-th finite difference of x (int64), entries o .. n - 1."""
    r = np.asarray(x, np.int64)
    for _ in range(o):
        r = r[1:] - r[:-1]
    return r


def choose(x, max_fixed_order=4, max_partition_order=5):
    """The subframe decision for one block.  Returns dict(kind, order, porder, params, bits): kind 0 constant, 1 verbatim, 8 + o fixed; params
    the Rice parameter of every partition; bits the subframe's size (its 8 header bits included)."""
    x = np.asarray(x, np.int64)
    n = x.size
    if np.all(x == x[0]):
        return dict(kind=KIND_CONSTANT, order=0, porder=0, params=[], bits=8 + 16)
    ks = np.arange(15, dtype=np.int64)[:, None]
    best = None
    for o in range(0, min(max_fixed_order, n - 1) + 1):
        r = residual(x, o)
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        full = np.zeros(n, np.int64)
        full[o:] = u
        sh = full[None, :] >> ks                                  # (15, n); the warm-up entries are 0 and are not counted below
        best_p = None
        for p in range(0, max_partition_order + 1):
            if n % (1 << p) or (n >> p) <= o:
                continue
            sums = sh.reshape(15, 1 << p, n >> p).sum(axis=2)     # (15, 2^p)
            count = np.full(1 << p, n >> p, np.int64)
            count[0] -= o
            cost = (ks + 1) * count[None, :] + sums
            kbest = np.argmin(cost, axis=0)                       # the first minimum: ties go to the smaller k
            total = 4 + int(np.sum(4 + cost[kbest, np.arange(1 << p)]))
            if best_p is None or total < best_p[0]:
                best_p = (total, p, kbest.tolist())
        bits = 8 + 16 * o + 2 + best_p[0]
        if best is None or bits < best["bits"]:
            best = dict(kind=KIND_FIXED + o, order=o, porder=best_p[1], params=best_p[2], bits=bits)
    if best["bits"] >= 8 + 16 * n:
        return dict(kind=KIND_VERBATIM, order=0, porder=0, params=[], bits=8 + 16 * n)
    return best


def _rice_bits(u, k):
    q = u >> k
    ln = q + 1 + k
    end = np.cumsum(ln)
    start = end - ln
    bits = np.zeros(int(end[-1]) if u.size else 0, np.uint8)
    bits[start + q] = 1
    for b in range(k):
        bits[start + q + 1 + b] = (u >> (k - 1 - b)) & 1
    return bits


def subframe_bits(x, ch):
    """The subframe of block x under the decision ch, as an array of bits."""
    x = np.asarray(x, np.int64)
    n = x.size
    s16 = lambda v: _bits_of(int(v) & 0xFFFF, 16)
    out = [np.array([0] + _bits_of(ch["kind"], 6) + [0], np.uint8)]
    if ch["kind"] == KIND_CONSTANT:
        out.append(np.array(s16(x[0]), np.uint8))
    elif ch["kind"] == KIND_VERBATIM:
        out.append(np.unpackbits((x & 0xFFFF).astype(">u2").view(np.uint8)))
    else:
        o, p = ch["order"], ch["porder"]
        for v in x[:o]:
            out.append(np.array(s16(v), np.uint8))
        out.append(np.array([0, 0] + _bits_of(p, 4), np.uint8))
        r = residual(x, o)
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        size = n >> p
        for j, k in enumerate(ch["params"]):
            lo, hi = max(j * size, o) - o, (j + 1) * size - o
            out.append(np.array(_bits_of(k, 4), np.uint8))
            out.append(_rice_bits(u[lo:hi], k))
    return np.concatenate(out)


def encode_frame(x, index, sample_rate, block_size, max_fixed_order=4, max_partition_order=5):
    """One frame: (bytes, decision)."""
    x = np.asarray(x, np.int64)
    n = x.size
    if n == block_size:
        bs_code, tail = 8 + BLOCK_SIZES.index(block_size), b""
    elif n <= 256:
        bs_code, tail = 6, bytes([n - 1])
    else:
        bs_code, tail = 7, bytes([(n - 1) >> 8, (n - 1) & 0xFF])
    hdr = bytes([0xFF, 0xF8, (bs_code << 4) | SAMPLE_RATE_CODE[sample_rate], (0 << 4) | (4 << 1) | 0]) + _utf8_number(index) + tail
    hdr += bytes([crc8(hdr)])
    ch = choose(x, max_fixed_order, max_partition_order)
    bits = subframe_bits(x, ch)
    assert bits.size == ch["bits"], (bits.size, ch)
    body = hdr + np.packbits(bits).tobytes()      # packbits pads with zero bits to the byte boundary
    c = crc16(body)
    return body + bytes([c >> 8, c & 0xFF]), ch


def stream_header(n, sample_rate, block_size, min_frame, max_frame):
    v = (sample_rate << 44) | (0 << 41) | (15 << 36) | n      # 20 + 3 + 5 + 36 bits
    return (b"fLaC" + bytes([0x80, 0x00, 0x00, 0x22]) + block_size.to_bytes(2, "big") * 2 + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big")
            + v.to_bytes(8, "big") + bytes(16))


def encode(pcm_i16, sample_rate=16000, block_size=4096, max_fixed_order=4, max_partition_order=5, info=None):
    """The stream of one segment.  `info`, a dict, receives frame_kind, frame_porder, frame_sizes and the decisions."""
    x = np.asarray(pcm_i16)
    assert x.dtype == np.int16 and x.ndim == 1 and x.size >= 1
    assert sample_rate in SAMPLE_RATE_CODE and block_size in BLOCK_SIZES
    frames, decisions = [], []
    for f, lo in enumerate(range(0, x.size, block_size)):
        data, ch = encode_frame(x[lo:lo + block_size], f, sample_rate, block_size, max_fixed_order, max_partition_order)
        frames.append(data)
        decisions.append(ch)
    sizes = [len(fr) for fr in frames]
    if info is not None:
        info.update(frame_kind=np.array([d["kind"] for d in decisions], np.uint8), frame_porder=np.array([d["porder"] for d in decisions], np.uint8),
                    frame_sizes=np.array(sizes, np.int64), decisions=decisions)
    return stream_header(x.size, sample_rate, block_size, min(sizes), max(sizes)) + b"".join(frames)


# ---------------------------------------------------------------------------------------------------------------- decoder
class _Bits:
    def __init__(self, data: bytes):
        self.data = data
        self.s = (np.unpackbits(np.frombuffer(data, np.uint8)) + 48).tobytes()      # b"0101..."
        self.pos = 0

    def u(self, n):
        if n == 0:
            return 0
        if self.pos + n > len(self.s):
            raise ValueError("flac: stream ends inside a field")
        v = int(self.s[self.pos:self.pos + n], 2)
        self.pos += n
        return v

    def s_(self, n):
        v = self.u(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self):
        i = self.s.find(b"1", self.pos)
        if i < 0:
            raise ValueError("flac: unary code runs off the stream")
        q = i - self.pos
        self.pos = i + 1
        return q


def _read_utf8_number(br):
    b0 = br.u(8)
    if b0 < 0x80:
        return b0, 1
    n = 0
    while b0 & (0x80 >> n):
        n += 1
    if n < 2 or n > 7:
        raise ValueError("flac: bad frame-number lead byte 0x%02x" % b0)
    v = b0 & (0x7F >> n)
    for _ in range(n - 1):
        c = br.u(8)
        if c & 0xC0 != 0x80:
            raise ValueError("flac: bad frame-number continuation byte")
        v = (v << 6) | (c & 0x3F)
    return v, n


_BS_TABLE = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
_SR_TABLE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_BPS_TABLE = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24}


def _decode_residual(br, n, order, out):
    method = br.u(2)
    if method > 1:
        raise ValueError("flac: reserved residual coding method")
    pbits, escape = (4, 15) if method == 0 else (5, 31)
    p = br.u(4)
    if n % (1 << p) or (n >> p) < order or (p > 0 and (n >> p) == 0):
        raise ValueError("flac: partition order %d does not fit a block of %d" % (p, n))
    for j in range(1 << p):
        count = (n >> p) - (order if j == 0 else 0)
        k = br.u(pbits)
        if k == escape:
            w = br.u(5)
            for _ in range(count):
                out.append(br.s_(w) if w else 0)
        else:
            for _ in range(count):
                q = br.unary()
                u = (q << k) | br.u(k)
                out.append((u >> 1) ^ -(u & 1))
    return p


def _decode_subframe(br, n, bps):
    if br.u(1):
        raise ValueError("flac: subframe padding bit set")
    t = br.u(6)
    wasted, porder = 0, 0
    if br.u(1):
        wasted = br.unary() + 1
    bps -= wasted
    if t == 0:
        x = [br.s_(bps)] * n
    elif t == 1:
        x = [br.s_(bps) for _ in range(n)]
    elif 8 <= t <= 12:
        o = t - 8
        if o > n:
            raise ValueError("flac: fixed order beyond the block")
        x = [br.s_(bps) for _ in range(o)]
        res = []
        porder = _decode_residual(br, n, o, res)
        c = FIXED_COEF[o]
        for r in res:
            x.append(r + sum(c[i] * x[-1 - i] for i in range(o)))
    elif t >= 32:
        raise ValueError("flac: LPC subframe (not read by this decoder)")
    else:
        raise ValueError("flac: reserved subframe type %d" % t)
    return ([v << wasted for v in x] if wasted else x), t, porder


def decode(data: bytes, info=None):
    """Decodes a mono stream to int16.  Raises ValueError on anything that is wrong.  `info` receives sample_rate, block_size, frame_kind."""
    if data[:4] != b"fLaC":
        raise ValueError("flac: no fLaC marker")
    pos, si = 4, None
    while True:
        if pos + 4 > len(data):
            raise ValueError("flac: truncated metadata")
        last, kind, ln = data[pos] >> 7, data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + ln]
        if len(body) != ln:
            raise ValueError("flac: truncated metadata block")
        if kind == 0:
            if ln != 34 or si is not None or pos != 4:
                raise ValueError("flac: bad STREAMINFO")
            si = body
        pos += 4 + ln
        if last:
            break
    if si is None:
        raise ValueError("flac: no STREAMINFO")
    min_bs, max_bs = int.from_bytes(si[0:2], "big"), int.from_bytes(si[2:4], "big")
    min_fs, max_fs = int.from_bytes(si[4:7], "big"), int.from_bytes(si[7:10], "big")
    v = int.from_bytes(si[10:18], "big")
    sr, ch, bps, total = v >> 44, ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1)
    if ch != 1 or bps != 16:
        raise ValueError("flac: this decoder reads 16-bit mono only (got %d channels, %d bits)" % (ch, bps))
    if min_bs != max_bs:
        raise ValueError("flac: variable block size in STREAMINFO")
    out, sizes, kinds, porders, expect = [], [], [], [], 0
    while pos < len(data):
        br = _Bits(data[pos:])
        if br.u(15) != 0x7FFC:
            raise ValueError("flac: lost sync at byte %d" % pos)
        if br.u(1):
            raise ValueError("flac: variable-blocksize frame in a fixed-blocksize stream")
        bs_code, sr_code = br.u(4), br.u(4)
        ch_code, ss_code = br.u(4), br.u(3)
        if br.u(1):
            raise ValueError("flac: reserved header bit set")
        number, _ = _read_utf8_number(br)
        if bs_code == 0:
            raise ValueError("flac: reserved block-size code")
        n = br.u(8) + 1 if bs_code == 6 else br.u(16) + 1 if bs_code == 7 else _BS_TABLE[bs_code]
        if sr_code in (0, 15):
            raise ValueError("flac: sample-rate code %d" % sr_code)
        fsr = br.u(8) * 1000 if sr_code == 12 else br.u(16) if sr_code == 13 else br.u(16) * 10 if sr_code == 14 else _SR_TABLE[sr_code]
        hdr_len = br.pos // 8
        if br.u(8) != crc8(br.data[:hdr_len]):
            raise ValueError("flac: frame %d: header CRC-8 mismatch" % expect)
        if number != expect:
            raise ValueError("flac: frame number %d where %d was due" % (number, expect))
        if fsr != sr:
            raise ValueError("flac: frame %d: sample rate %d, STREAMINFO %d" % (expect, fsr, sr))
        if ch_code != 0 or _BPS_TABLE.get(ss_code) != 16:
            raise ValueError("flac: frame %d: channel / sample-size code %d / %d" % (expect, ch_code, ss_code))
        if n > max_bs or (n != max_bs and len(out) + n != total):
            raise ValueError("flac: frame %d: block of %d in a stream of block size %d" % (expect, n, max_bs))
        x, kind, porder = _decode_subframe(br, n, 16)
        kinds.append(kind)
        porders.append(porder)
        while br.pos % 8:
            if br.u(1):
                raise ValueError("flac: frame %d: padding bit set" % expect)
        body_len = br.pos // 8
        if br.u(16) != crc16(br.data[:body_len]):
            raise ValueError("flac: frame %d: CRC-16 mismatch" % expect)
        sizes.append(body_len + 2)
        pos += body_len + 2
        out.extend(x)
        expect += 1
    if len(out) != total:
        raise ValueError("flac: %d samples decoded, STREAMINFO says %d" % (len(out), total))
    if not sizes or min(sizes) != min_fs or max(sizes) != max_fs:
        raise ValueError("flac: frame sizes %s..%s, STREAMINFO says %d..%d" % (min(sizes, default=None), max(sizes, default=None), min_fs, max_fs))
    arr = np.array(out, np.int64)
    if arr.min() < -32768 or arr.max() > 32767:
        raise ValueError("flac: decoded sample outside 16 bits")
    if info is not None:
        info.update(sample_rate=sr, block_size=max_bs, total=total, frame_sizes=sizes, frame_kind=kinds, frame_porder=porders)
    return arr.astype(np.int16)


# ---------------------------------------------------------------------------------------------------------------- signals
def voiced(n, sample_rate=16000, seed=0):
    """The synthetic voiced signal: 24 harmonics of 120 Hz with a 1 / h roll-off, a 3 Hz envelope and a noise floor; int16."""
    t = np.arange(n, dtype=np.float64) / sample_rate
    x = sum(np.sin(2 * np.pi * 120.0 * h * t + 0.37 * h) / h for h in range(1, 25))
    x *= 0.5 * (1.0 + np.sin(2 * np.pi * 3.0 * t))
    x = 0.22 * x + 0.002 * np.random.default_rng(seed).standard_normal(n)
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def _regimes(amps, n, rng):
    seg = n // len(amps)
    return np.concatenate([rng.integers(-a, a + 1, seg) for a in amps]).astype(np.int16)


def signal_set():
    """name -> int16 signal.  Together they reach CONSTANT, VERBATIM, FIXED 0 .. 4 and the partition orders 0 .. 5 (tests/test_flac.py asserts
    which signal reaches what, from this oracle's own choices)."""
    rng = np.random.default_rng(1)
    s = {}
    s["zeros"] = np.zeros(5000, np.int16)
    s["dc"] = np.full(5000, -1234, np.int16)
    s["noise_full"] = rng.integers(-32768, 32768, 5000).astype(np.int16)
    alt = np.empty(5000, np.int16)
    alt[0::2], alt[1::2] = 32767, -32768
    s["alternation"] = alt
    imp = np.zeros(4096, np.int16)
    imp[100] = 32767
    s["impulse"] = imp
    s["ramp"] = (np.arange(5000) * 3 - 7000).astype(np.int16)
    s["sine440"] = np.round(12000 * np.sin(2 * np.pi * 440 * np.arange(6000) / 16000)).astype(np.int16)
    s["noise_small"] = rng.integers(-3, 4, 4096 + 96).astype(np.int16)
    s["voiced"] = voiced(16384)
    s["sine80_noise"] = (np.round(8000 * np.sin(2 * np.pi * 80 * np.arange(4096) / 16000)) + rng.integers(-2, 3, 4096)).astype(np.int16)
    s["two_levels"] = _regimes([4, 400], 4096, rng)
    s["four_levels"] = _regimes([4, 400, 4, 400], 4096, rng)
    return s
