"""numpy restatement of ev_flac_lpc (include/evhip.h, rules 4 .. 9, the LPC subframe and the MD5) and a FLAC decoder of its own.

`encode` produces whole streams; with max_lpc_order = 0 and md5 = False they are `flac_oracle.encode`'s.  The fp64 steps are Python floats: one
IEEE operation per rounding, in the order the header states.  `decode` is written from the format and shares nothing with the encoder or with
`flac_oracle.decode`: it reads FIXED and LPC subframes, both Rice methods and escape partitions, refuses a negative shift and the precision code
15, checks both CRCs and, when STREAMINFO carries a digest, the MD5.
"""
import hashlib
import math

import numpy as np

import flac_oracle as fo

KIND_LPC = 32
MAX_LPC_ORDER = 12


# ---------------------------------------------------------------------------------------------------------------- analysis (rules 4 .. 7)
def window(m):
    i = np.arange(m, dtype=np.int64)
    return (32767 * 4 * i * (m - 1 - i)) // ((m - 1) * (m - 1))


def analyse(x, max_lpc_order, q, events=None):
    """Rules 4 .. 7 for one block: R (13 int64, zero beyond L), shift (12, -1 = no candidate), coef (12, 12) [order - 1][j].  `events`, a set,
    receives the names of the branches taken."""
    x = np.asarray(x, np.int64)
    m = x.size
    R = np.zeros(13, np.int64)
    shift = np.full(MAX_LPC_ORDER, -1, np.int64)
    coef = np.zeros((MAX_LPC_ORDER, MAX_LPC_ORDER), np.int64)
    ev = events if events is not None else set()
    L = min(max_lpc_order, m - 1)
    if L < 1:
        return R, shift, coef
    y = (x * window(m)) >> 15
    assert np.abs(y).max(initial=0) < 1 << 15
    for l in range(L + 1):
        R[l] = int(np.sum(y[l:] * y[:m - l]))
    if R[0] == 0:
        ev.add("r0_zero")
        return R, shift, coef
    levinson(R, L, q, shift, coef, ev)
    return R, shift, coef


def levinson(R, L, q, shift, coef, ev):
    """Rules 6 and 7 on the autocorrelation R[0 .. L], R[0] > 0: fills shift and coef."""
    a = []
    err = float(R[0])
    for it in range(L):
        acc = float(R[it + 1])
        for j in range(it):
            acc = acc - a[j] * float(R[it - j])
        k = acc / err
        a = [a[j] - k * a[it - 1 - j] for j in range(it)] + [k]
        err = err * (1.0 - k * k)
        if not math.isfinite(err) or err <= 0.0:
            ev.add("levinson_stop")
            break
        cmax = max(abs(v) for v in a)
        if cmax == 0.0 or not math.isfinite(cmax):
            ev.add("cmax_zero")
            continue
        e = math.frexp(cmax)[1]
        sh = q - 1 - e
        if sh < 0:
            ev.add("shift_negative")
            continue
        if sh > 15:
            ev.add("shift_clamped")
            sh = 15
        lo, hi = -(1 << (q - 1)), (1 << (q - 1)) - 1
        for j, v in enumerate(a):
            c = int(np.rint(v * float(1 << sh)))
            if c > hi:
                ev.add("coef_clamped")
            coef[it, j] = min(max(c, lo), hi)
        shift[it] = sh


def lpc_residual(x, c, sh):
    """r_i, i = o .. m - 1 (rule 8), int64."""
    x = np.asarray(x, np.int64)
    o, m = len(c), x.size
    pred = np.zeros(m - o, np.int64)
    for j in range(o):
        pred += int(c[j]) * x[o - 1 - j:m - 1 - j]
    return x[o:] - (pred >> int(sh))


def rice_search(r, m, o, max_partition_order):
    """Rule 2's search for the residual r of samples o .. m - 1: (cost with the 4 bits of the partition order, p, parameters)."""
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    full = np.zeros(m, np.int64)
    full[o:] = u
    ks = np.arange(15, dtype=np.int64)[:, None]
    pmax = min(max_partition_order, (m & -m).bit_length() - 1)
    fine = (full[None, :] >> ks).reshape(15, 1 << pmax, m >> pmax).sum(axis=2)
    best = None
    for p in range(pmax + 1):
        if (m >> p) <= o:
            continue
        sums = fine.reshape(15, 1 << p, 1 << (pmax - p)).sum(axis=2)
        count = np.full(1 << p, m >> p, np.int64)
        count[0] -= o
        cost = (ks + 1) * count[None, :] + sums
        kb = np.argmin(cost, axis=0)
        total = 4 + int(np.sum(4 + cost[kb, np.arange(1 << p)]))
        if best is None or total < best[0]:
            best = (total, p, kb.tolist())
    return best


def choose(x, max_fixed_order=4, max_partition_order=5, max_lpc_order=0, q=12, events=None):
    """The decision for one block: flac_oracle.choose's dict; an LPC winner adds coef and shift.  `events` also receives ("lpc", o) for a
    chosen order and ("margin", d) with d = best LPC bits - best FIXED bits."""
    x = np.asarray(x, np.int64)
    m = x.size
    base = fo.choose(x, max_fixed_order, max_partition_order)
    if base["kind"] == fo.KIND_CONSTANT or max_lpc_order < 1:
        return base
    fixed_bits = base["bits"]
    if base["kind"] == fo.KIND_VERBATIM:      # the best FIXED candidate, which VERBATIM displaced
        fixed_bits = min(8 + 16 * o + 2 + rice_search(fo.residual(x, o), m, o, max_partition_order)[0] for o in range(min(max_fixed_order, m - 1) + 1))
    _, shift, coef = analyse(x, max_lpc_order, q, events)
    best, best_bits = None, fixed_bits
    lpc_min = None
    for o in range(1, min(max_lpc_order, m - 1) + 1):
        if shift[o - 1] < 0:
            continue
        c = coef[o - 1, :o]
        r = lpc_residual(x, c, shift[o - 1])
        if np.abs(r).max() >= 1 << 31:
            if events is not None:
                events.add("residual_overflow")
            continue
        cost, p, ks = rice_search(r, m, o, max_partition_order)
        bits = 8 + 16 * o + 4 + 5 + q * o + 2 + cost
        lpc_min = bits if lpc_min is None else min(lpc_min, bits)
        if bits < best_bits:
            best_bits = bits
            best = dict(kind=KIND_LPC + o - 1, order=o, porder=p, params=ks, bits=bits, coef=[int(v) for v in c], shift=int(shift[o - 1]), q=q)
    if events is not None and lpc_min is not None:
        events.add(("margin", int(lpc_min - fixed_bits)))
    if best is None or best_bits >= 8 + 16 * m:
        return base
    if events is not None:
        events.add(("lpc", best["order"]))
    return best


# ---------------------------------------------------------------------------------------------------------------- encoder
def subframe_bits(x, ch):
    if ch["kind"] < KIND_LPC:
        return fo.subframe_bits(x, ch)
    x = np.asarray(x, np.int64)
    m, o, p, q = x.size, ch["order"], ch["porder"], ch["q"]
    bits = [0] + fo._bits_of(ch["kind"], 6) + [0]
    for v in x[:o]:
        bits += fo._bits_of(int(v) & 0xFFFF, 16)
    bits += fo._bits_of(q - 1, 4) + fo._bits_of(ch["shift"], 5)
    for c in ch["coef"]:
        bits += fo._bits_of(c & ((1 << q) - 1), q)
    bits += [0, 0] + fo._bits_of(p, 4)
    out = [np.array(bits, np.uint8)]
    r = lpc_residual(x, ch["coef"], ch["shift"])
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    size = m >> p
    for j, k in enumerate(ch["params"]):
        lo, hi = max(j * size, o) - o, (j + 1) * size - o
        out.append(np.array(fo._bits_of(k, 4), np.uint8))
        out.append(fo._rice_bits(u[lo:hi], k))
    return np.concatenate(out)


def encode_frame(x, index, sample_rate, block_size, max_fixed_order=4, max_partition_order=5, max_lpc_order=0, q=12, events=None):
    x = np.asarray(x, np.int64)
    n = x.size
    if n == block_size:
        bs_code, tail = 8 + fo.BLOCK_SIZES.index(block_size), b""
    elif n <= 256:
        bs_code, tail = 6, bytes([n - 1])
    else:
        bs_code, tail = 7, bytes([(n - 1) >> 8, (n - 1) & 0xFF])
    hdr = bytes([0xFF, 0xF8, (bs_code << 4) | fo.SAMPLE_RATE_CODE[sample_rate], 4 << 1]) + fo._utf8_number(index) + tail
    hdr += bytes([fo.crc8(hdr)])
    ch = choose(x, max_fixed_order, max_partition_order, max_lpc_order, q, events)
    bits = subframe_bits(x, ch)
    assert bits.size == ch["bits"], (bits.size, ch)
    body = hdr + np.packbits(bits).tobytes()
    c = fo.crc16(body)
    return body + bytes([c >> 8, c & 0xFF]), ch


def encode(pcm_i16, sample_rate=16000, block_size=4096, max_fixed_order=4, max_partition_order=5, max_lpc_order=0, qlp_precision=12, md5=False,
           info=None, events=None):
    """The stream of one segment.  `info` receives frame_kind, frame_porder, frame_sizes and the decisions; `events` the branches taken."""
    x = np.asarray(pcm_i16)
    assert x.dtype == np.int16 and x.ndim == 1 and x.size >= 1
    frames, decisions = [], []
    for f, lo in enumerate(range(0, x.size, block_size)):
        blk = x[lo:lo + block_size]
        if events is not None and blk.size <= max_lpc_order:
            events.add(("short_block", int(blk.size)))
        data, ch = encode_frame(blk, f, sample_rate, block_size, max_fixed_order, max_partition_order, max_lpc_order, qlp_precision, events)
        frames.append(data)
        decisions.append(ch)
    sizes = [len(fr) for fr in frames]
    if info is not None:
        info.update(frame_kind=np.array([d["kind"] for d in decisions], np.uint8), frame_porder=np.array([d["porder"] for d in decisions], np.uint8),
                    frame_sizes=np.array(sizes, np.int64), decisions=decisions)
    head = fo.stream_header(x.size, sample_rate, block_size, min(sizes), max(sizes))
    if md5:
        head = head[:26] + hashlib.md5(x.astype("<i2").tobytes()).digest()
    return head + b"".join(frames)


# ---------------------------------------------------------------------------------------------------------------- decoder
class _Reader:
    """Big-endian bit reader over one Python integer."""

    def __init__(self, data):
        self.n = 8 * len(data)
        self.v = int.from_bytes(data, "big")
        self.pos = 0

    def bits(self, k):
        if k == 0:
            return 0
        if self.pos + k > self.n:
            raise ValueError("flac: the stream ends inside a field")
        self.pos += k
        return (self.v >> (self.n - self.pos)) & ((1 << k) - 1)

    def signed(self, k):
        u = self.bits(k)
        return u - (1 << k) if u >> (k - 1) else u


def _residuals(bitstr, pos, n, order):
    """Reads the residual section from the ASCII bit string; returns (values, new position, partition order)."""
    def take(k):
        nonlocal pos
        if pos + k > len(bitstr):
            raise ValueError("flac: the stream ends inside the residual")
        v = int(bitstr[pos:pos + k], 2) if k else 0
        pos += k
        return v
    method = take(2)
    if method > 1:
        raise ValueError("flac: reserved residual coding method %d" % method)
    pw = 4 if method == 0 else 5
    p = take(4)
    if n % (1 << p) or (n >> p) < order:
        raise ValueError("flac: partition order %d does not fit %d samples at predictor order %d" % (p, n, order))
    out = []
    for j in range(1 << p):
        cnt = (n >> p) - (order if j == 0 else 0)
        k = take(pw)
        if k == (1 << pw) - 1:
            w = take(5)
            for _ in range(cnt):
                u = take(w)
                out.append(u - (1 << w) if w and u >> (w - 1) else u)
            continue
        for _ in range(cnt):
            one = bitstr.find(b"1", pos)
            if one < 0:
                raise ValueError("flac: a unary code runs off the stream")
            u = ((one - pos) << k) | (int(bitstr[one + 1:one + 1 + k], 2) if k else 0)
            pos = one + 1 + k
            if pos > len(bitstr):
                raise ValueError("flac: the stream ends inside the residual")
            out.append((u >> 1) if not u & 1 else -((u + 1) >> 1))
    return out, pos, p


_FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))
_BLOCK = {1: 192, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
_BLOCK.update({c: 576 << (c - 2) for c in (2, 3, 4, 5)})
_RATE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}


def _predict(x, res, coefs, shift):
    o = len(coefs)
    for r in res:
        s = 0
        for j in range(o):
            s += coefs[j] * x[-1 - j]
        x.append(r + (s >> shift))      # Python's >> on a negative integer is the arithmetic shift


def decode(data, info=None):
    """A 16-bit mono fixed-blocksize stream -> int16.  ValueError on anything wrong.  `info` receives frame_kind, frame_porder, md5_checked."""
    if data[:4] != b"fLaC":
        raise ValueError("flac: no fLaC marker")
    if len(data) < 42 or data[4] & 0x7F != 0 or data[5:8] != b"\x00\x00\x22":
        raise ValueError("flac: the first metadata block is not a STREAMINFO of 34 bytes")
    pos, last = 42, data[4] >> 7
    while not last:
        if pos + 4 > len(data):
            raise ValueError("flac: truncated metadata")
        last = data[pos] >> 7
        pos += 4 + int.from_bytes(data[pos + 1:pos + 4], "big")
    si = _Reader(data[8:42])
    min_bs, max_bs, min_fs, max_fs = si.bits(16), si.bits(16), si.bits(24), si.bits(24)
    rate, channels, bps, total = si.bits(20), si.bits(3) + 1, si.bits(5) + 1, si.bits(36)
    digest = data[26:42]
    if channels != 1 or bps != 16 or min_bs != max_bs:
        raise ValueError("flac: not a 16-bit mono stream of fixed block size")
    out, kinds, porders, sizes, number = [], [], [], [], 0
    while pos < len(data):
        frame = data[pos:]
        rd = _Reader(frame)
        if rd.bits(16) != 0xFFF8:
            raise ValueError("flac: no fixed-blocksize sync code at byte %d" % pos)
        bs_code, sr_code, ch_code, ss_code, rsv = rd.bits(4), rd.bits(4), rd.bits(4), rd.bits(3), rd.bits(1)
        lead = rd.bits(8)
        extra = 0
        while lead & (0x80 >> extra):
            extra += 1
        if extra == 1 or extra > 7:
            raise ValueError("flac: bad frame-number lead byte")
        idx = lead & (0xFF >> (extra + 1)) if extra else lead
        for _ in range(max(extra - 1, 0)):
            b = rd.bits(8)
            if b >> 6 != 2:
                raise ValueError("flac: bad frame-number continuation byte")
            idx = (idx << 6) | (b & 0x3F)
        if bs_code == 0 or sr_code in (0, 15) or rsv:
            raise ValueError("flac: reserved code in a frame header")
        n = rd.bits(8) + 1 if bs_code == 6 else rd.bits(16) + 1 if bs_code == 7 else _BLOCK[bs_code]
        frate = rd.bits(8) * 1000 if sr_code == 12 else rd.bits(16) if sr_code == 13 else rd.bits(16) * 10 if sr_code == 14 else _RATE[sr_code]
        hl = rd.pos // 8
        if rd.bits(8) != fo.crc8(frame[:hl]):
            raise ValueError("flac: frame %d: CRC-8 mismatch" % number)
        if idx != number or frate != rate or ch_code != 0 or ss_code != 4:
            raise ValueError("flac: frame %d: header disagrees with the stream (number %d, rate %d, channel code %d, size code %d)" % (number, idx, frate, ch_code, ss_code))
        if n > max_bs or (n != max_bs and len(out) + n != total):
            raise ValueError("flac: frame %d: %d samples in a stream of block size %d" % (number, n, max_bs))
        # the subframe
        if rd.bits(1):
            raise ValueError("flac: subframe padding bit")
        t = rd.bits(6)
        if rd.bits(1):
            raise ValueError("flac: wasted bits are not read by this decoder")
        porder = 0
        if t == 0:
            x = [rd.signed(16)] * n
        elif t == 1:
            x = [rd.signed(16) for _ in range(n)]
        elif 8 <= t <= 12 or t >= 32:
            o = t - 8 if t < 32 else t - 31
            if o > n:
                raise ValueError("flac: frame %d: predictor order %d beyond the block" % (number, o))
            x = [rd.signed(16) for _ in range(o)]
            coefs, shift = _FIXED[o] if t < 32 else None, 0
            if t >= 32:
                prec = rd.bits(4) + 1
                if prec == 16:
                    raise ValueError("flac: frame %d: invalid coefficient precision code 15" % number)
                shift = rd.signed(5)
                if shift < 0:
                    raise ValueError("flac: frame %d: negative LPC shift" % number)
                coefs = [rd.signed(prec) for _ in range(o)]
            bitstr = bin(rd.v | (1 << rd.n))[3:].encode()
            res, rd.pos, porder = _residuals(bitstr, rd.pos, n, o)
            _predict(x, res, coefs, shift)
        else:
            raise ValueError("flac: frame %d: reserved subframe type %d" % (number, t))
        while rd.pos % 8:
            if rd.bits(1):
                raise ValueError("flac: frame %d: padding bit set" % number)
        bl = rd.pos // 8
        if rd.bits(16) != fo.crc16(frame[:bl]):
            raise ValueError("flac: frame %d: CRC-16 mismatch" % number)
        out.extend(x)
        kinds.append(t)
        porders.append(porder)
        sizes.append(bl + 2)
        pos += bl + 2
        number += 1
    if len(out) != total:
        raise ValueError("flac: %d samples decoded, STREAMINFO says %d" % (len(out), total))
    if not sizes or min(sizes) != min_fs or max(sizes) != max_fs:
        raise ValueError("flac: frame sizes disagree with STREAMINFO")
    arr = np.array(out, np.int64)
    if arr.min() < -32768 or arr.max() > 32767:
        raise ValueError("flac: a decoded sample leaves 16 bits")
    pcm = arr.astype(np.int16)
    checked = digest != bytes(16)
    if checked and hashlib.md5(pcm.astype("<i2").tobytes()).digest() != digest:
        raise ValueError("flac: MD5 mismatch")
    if info is not None:
        info.update(frame_kind=kinds, frame_porder=porders, frame_sizes=sizes, sample_rate=rate, block_size=max_bs, md5_checked=checked)
    return pcm


# ---------------------------------------------------------------------------------------------------------------- signals
def ar_signal(poles, n, amp, seed):
    """Noise through the all-pole filter with the given complex poles (and their conjugates), scaled to `amp` peak; int16."""
    a = np.array([1.0])
    for p in poles:
        a = np.convolve(a, [1.0, -2.0 * p.real, abs(p) ** 2] if abs(p.imag) > 0 else [1.0, -p.real])
    e = np.random.default_rng(seed).standard_normal(n)
    y = np.zeros(n)
    for i in range(n):
        acc = e[i]
        for j in range(1, min(len(a), i + 1)):
            acc -= a[j] * y[i - j]
        y[i] = acc
    return np.round(y * (amp / np.abs(y).max())).astype(np.int16)


def _pole(r, f, sr=16000.0):
    return r * np.exp(2j * np.pi * f / sr)


def signal_set():
    """flac_oracle.signal_set() and the signals the LPC branches need (tests/test_flac_lpc.py asserts which branches the oracle reaches)."""
    rng = np.random.default_rng(7)
    s = dict(fo.signal_set())
    s["ar2"] = ar_signal([_pole(0.98, 700)], 4096, 9000, 11)
    s["ar4"] = ar_signal([_pole(0.985, 500), _pole(0.97, 1900)], 4096, 12000, 12)
    s["ar8"] = ar_signal([_pole(0.99, 300), _pole(0.98, 1200), _pole(0.97, 2500), _pole(0.96, 3600)], 8192, 16000, 13)
    s["ar12"] = ar_signal([_pole(0.995, 250), _pole(0.99, 800), _pole(0.985, 1500), _pole(0.98, 2400), _pole(0.975, 3300), _pole(0.97, 5200)], 8192, 20000, 14)
    t = np.arange(8192)
    s["sines5"] = np.round(sum(a * np.sin(2 * np.pi * f * t / 16000 + 0.3 * i) for i, (a, f) in enumerate(
        [(6000, 210.0), (4000, 655.0), (3000, 1370.0), (2000, 2890.0), (1500, 4100.0)])) + rng.integers(-1, 2, t.size)).astype(np.int16)
    b01 = rng.integers(0, 2, 4096 + 2).astype(np.int16)      # 0 / +1: the windowed block is all zero (a -1 would give (-w) >> 15 = -1)
    b01[0], b01[-1] = 0, 1
    s["binary01"] = b01
    for m in (1, 2, 3, 10):
        s["tail%d" % m] = np.round(7000 * np.sin(2 * np.pi * 333.0 * np.arange(4096 + m) / 16000)).astype(np.int16) + rng.integers(-3, 4, 4096 + m).astype(np.int16)
    return s


CONFIGS = ((8, 12), (12, 12), (12, 5), (4, 15))      # (max_lpc_order, qlp_precision)
BLOCKS = (256, 4096)
