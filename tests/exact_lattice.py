"""Exact-lattice inputs and references for the GEMM family (numpy only, no GPU).

Every product of the conv-GEMM kernels is exact in fp32 (fp16 x fp16, fp4 x fp4 with power-of-two scales); the only rounding is the fp32
accumulation.  Operands taken from a dyadic lattice on which every partial sum, in any order, is an integer multiple of one quantum below 2^24
of it make that accumulation exact as well: the result no longer depends on the summation order, the tile, the MFMA variant or the split-K
count, and every output element has one correct bit pattern.  This module builds such inputs (``make_inputs``), proves the precondition
(``budget``), evaluates what each precision promises in fp64 (``expected``) and compares element by element (``mismatches`` / ``compare``).

Lattices
  L0  x = small integers 2^-2, w = small integers 2^-4, dense; bias / residual / addends dyadic.  Everything is fp16-representable, so all lo
      parts (and with them the cross terms of the split and MX precisions) are exactly zero.
  L1  two-level: v = a 2^p + b 2^(p-13), a in +-{4, 6} or 0, b in +-{0, .5, 1, 1.5, 2, 3, 4, 6} and 0 wherever a is; every scale block
      (activations 32, weights 128 along K) has one pinned |a| = 4 with |b| = 4, so the OCP scale rule puts the fp4 grid on the lattice.
      mxfp4.split_hi_lo / quantize / dequantize / e5m2_hi_codes / e5m2_lo_codes are lossless on it (offset 13 is the smallest for which the
      fp16 split is: 4 - 6 2^-12 rounds into the lower binade).  Sparse by necessity: 36 2^(p+q) against a quantum of 2^(p+q-13) leaves
      ~5.8 bits of head-room.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from emotivoice_amd import mxfp4

PAD = 64                        # slack rows on both sides of every activation (the layout of tests/test_gpu_ops.py)
LIMIT_BITS = 24                 # budget: sum of |terms| / smallest quantum < 2^24 <=> every partial sum in any order is exact in fp32
L1_OFFSET = 13
L1_B = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
SCALES = (1.0, 0.5, 0.25)       # out_scale values (dyadic: nothing rounds, FMA contraction cannot matter)
SLOPES = (0.5, 0.125)           # leaky-relu slopes


@dataclasses.dataclass(frozen=True)
class Case:
    """One launch.  epi: any of "bias", "pro" (leaky-relu prologue), "relu", "lrelu", "seq_bias", "res16", "res32", "respl" (MX: the residual comes from the
    plane set of lrelu(residual, slope): hi + Q4(lo), then the inverse leaky-relu), "scale", "acc32", "accpl" (MX: the addend is a partial plane set's
    hi + Q4(lo)), "add16", "post", "before_post"; outs: which of out16 / out32 the launch writes; mask: valid_shift of a row mask (0 = none); mask_runs: (first group, groups) runs of
    invalid row groups in addition to the default ones."""
    name: str
    kernel: str
    dtype: int                  # 0 fp16, 1 fp32, 2 split precision, 3 MX
    M: int
    K: int
    N: int
    taps: int
    dil: int = 1
    lattice: str = "L0"
    density: float = 1.0        # L1: probability of a nonzero hi part (x and w alike)
    epi: tuple = ("bias",)
    outs: str = "both"
    mask: int = 0
    mask_runs: tuple = ()
    dbg: int = 0                # ev_conv_gemm_desc.reserved0
    ksplit: int = 0
    slope: float = 0.5          # every leaky-relu of the case
    scale: float = 0.5          # out_scale when "scale" is in epi
    seed: int = 0
    extra: tuple = ()           # test-specific switches (plane-set input, emitted planes, ...)

    @property
    def center(self):
        return (self.taps - 1) // 2

    def has(self, what):
        return what in self.epi


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# lattices
def ints(rng, shape, amp, exp):
    """integers in [-amp, amp] times 2^exp, fp32"""
    return np.ldexp(rng.integers(-amp, amp + 1, shape).astype(np.float32), exp)


def two_level(rng, shape, block, p, density):
    """L1 along the last axis (a multiple of ``block``) -> fp32"""
    K = shape[-1]
    assert K % block == 0
    sgn = lambda: rng.choice(np.array([-1.0, 1.0]), shape)          # noqa: E731
    a = rng.choice(np.array([4.0, 6.0]), shape) * sgn() * (rng.random(shape) < density)
    b = rng.choice(L1_B, shape) * sgn() * (a != 0)
    ab = a.reshape(-1, K // block, block)
    bb = b.reshape(-1, K // block, block)
    pin = rng.integers(0, block, ab.shape[:2])
    i, j = np.meshgrid(np.arange(ab.shape[0]), np.arange(ab.shape[1]), indexing="ij")
    ab[i, j, pin] = 4.0 * rng.choice(np.array([-1.0, 1.0]), pin.shape)
    bb[i, j, pin] = 4.0 * rng.choice(np.array([-1.0, 1.0]), pin.shape)
    v = np.ldexp(ab, p) + np.ldexp(bb, p - L1_OFFSET)
    out = v.reshape(shape).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v.reshape(shape))
    return out


def lrelu(v, s):
    return np.where(v > 0, v, v * s)


def valid_bytes(case):
    """row_valid bytes (one per 2^mask rows): invalid groups at both ends, a run in the middle, and the case's own runs"""
    if not case.mask:
        return None
    g = case.M >> case.mask
    v = np.ones(g, np.uint8)
    v[:2] = 0
    v[-1:] = 0
    v[g // 3:g // 3 + 3] = 0
    for first, n in case.mask_runs:
        v[first:first + n] = 0
    return v


def make_inputs(case):
    """-> dict of numpy arrays in the layouts of the op tests: x [PAD + M + PAD][K] (fp32 values; halo and masked rows zero), w [N][taps][K], and whatever the
    epilogue of the case reads.  With a leaky-relu prologue x is the pre-image of a lattice tensor, so the lattice is what the kernel multiplies."""
    assert case.slope in SLOPES and (case.scale in SCALES or not case.has("scale"))
    rng = np.random.default_rng(case.seed * 1000 + case.M % 997 + case.K + case.N + case.taps)
    M, K, N, taps = case.M, case.K, case.N, case.taps
    inp = {}
    if case.lattice == "L0":
        y = ints(rng, (M, K), 8, -2)
        w = ints(rng, (N, taps, K), 8, -4)
    else:
        assert case.dtype in (2, 3) and case.lattice == "L1"
        y = two_level(rng, (M, K), 32, -2, case.density)
        w = two_level(rng, (N, taps, K), 128 if K % 128 == 0 else 32, -3, case.density)
    if case.has("pro"):
        y = np.where(y > 0, y, y / np.float32(case.slope)).astype(np.float32)          # lrelu(x) == the lattice tensor
    vb = valid_bytes(case)
    if vb is not None:
        inp["valid"] = vb
        inp["vrow"] = np.repeat(vb != 0, 1 << case.mask)
        y[~inp["vrow"]] = 0
    x = np.zeros((M + 2 * PAD, K), np.float32)
    x[PAD:PAD + M] = y
    inp["x"], inp["w"] = x, w
    big = case.lattice == "L0"          # L1 has ~6 bits of head-room in all: its addends stay below one
    if case.has("bias"):
        inp["bias"] = ints(rng, (N,), 512 if big else 64, -8)
    if case.has("seq_bias"):
        inp["row_seq"] = rng.integers(0, 3, M).astype(np.int32)
        inp["seq_bias"] = ints(rng, (3, N), 256, -7)
    if case.has("res16"):
        inp["res"] = ints(rng, (M, N), 255, -7).astype(np.float16)
    if case.has("res32"):
        inp["res"] = ints(rng, (M, N), 4095 if big else 255, -8)
    if case.has("acc32"):
        inp["acc32"] = ints(rng, (M, N), 4095 if big else 255, -9)
    if case.has("add16"):
        inp["add16"] = (ints(rng, (M, N), 255, -8).astype(np.float16), ints(rng, (M, N), 255, -8).astype(np.float16))
    for key in ("respl", "accpl"):          # [PAD + M + PAD][N] activations whose plane sets the launch reads (invalid and slack rows zero)
        if case.has(key):
            a = ints(rng, (M, N), 8, -2) if big else two_level(rng, (M, N), 32, -4, case.density)
            if vb is not None:
                a[~inp["vrow"]] = 0
            inp[key] = np.zeros((M + 2 * PAD, N), np.float32)
            inp[key][PAD:PAD + M] = a
    return inp


def from_planes(a):
    """what a consumer reads back from the plane set of a: fp16 hi + Q4(lo) (the host quantiser's; lossless on both lattices) -> fp64"""
    hi, lo = mxfp4.split_hi_lo(a)
    return hi.astype(np.float64) + mxfp4.dequantize(*mxfp4.quantize(lo, 32), 32).astype(np.float64)


def plane_addends(case, inp, rows):
    """-> (residual from planes: the inverse leaky-relu of the stored activation, addend from a partial plane set), None where the case has none"""
    res = acc = None
    if case.has("respl"):
        a = from_planes(inp["respl"])[PAD + rows]
        res = np.where(a >= 0, a, a / case.slope)
    if case.has("accpl"):
        acc = from_planes(inp["accpl"])[PAD + rows]
    return res, acc


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the reference
def quantum(a):
    """largest power of two that divides every nonzero element (inf for an all-zero array)"""
    a = np.abs(np.asarray(a, np.float64)).ravel()
    a = a[a > 0]
    if a.size == 0:
        return np.inf
    m, e = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64)
    return float(np.ldexp((mi & -mi).astype(np.float64), e - 53).min())


def conv(xfull, w, taps, dil, center, rows):
    """sum over taps of shifted x @ w_t.T in fp64 for the output rows ``rows`` -> [len(rows)][N]"""
    xfull, w = np.asarray(xfull, np.float64), np.asarray(w, np.float64)
    out = np.zeros((len(rows), w.shape[0]))
    for t in range(taps):
        out += xfull[PAD + rows + (t - center) * dil] @ w[:, t, :].T
    return out


def w_block(K):
    return 128 if K % 128 == 0 else 32


def operand_parts(case, inp, w=None):
    """the operand pairs whose products the precision adds, as fp64 arrays: [(x part [PAD + M + PAD][K], w part [N][taps][K])]"""
    x = inp["x"]
    w = inp["w"] if w is None else w
    if case.has("pro"):
        x = lrelu(x, np.float32(case.slope)).astype(np.float32)          # (exact: dyadic slope)
    if case.dtype in (0, 1):
        if case.dtype == 0:
            assert np.array_equal(x.astype(np.float16).astype(np.float32), x) and np.array_equal(w.astype(np.float16).astype(np.float32), w)
        return [(x, w)]
    xh, xl = mxfp4.split_hi_lo(x)
    wh, wl = mxfp4.split_hi_lo(w)
    if case.dtype == 2:
        # the kernel's lo operands are fp16((v - hi) 2^11): exact on both lattices, so 2^-11 (xh.wl' + xl'.wh) = xh.wl + xl.wh
        for lo in (xl, wl):
            s = lo * np.float32(2048.0)
            assert np.array_equal(s.astype(np.float16).astype(np.float32), s)
        return [(xh, wh), (xh, wl), (xl, wh)]
    q = lambda v, blk, rule: mxfp4.dequantize(*mxfp4.quantize(v, blk, rule), blk)          # noqa: E731
    bw = w_block(case.K)
    return [(xh, wh), (q(xh, 32, "ocp"), q(wl, bw, mxfp4.W_RULE)), (q(xl, 32, "ocp"), q(wh, bw, mxfp4.W_RULE))]


def epilogue(case, inp, v, rows):
    """the documented order on the exact conv value v [len(rows)][N] -> (value stored to out32, value stored to out16 / emitted as planes)"""
    s = case.slope
    if case.has("bias"):
        v = v + inp["bias"].astype(np.float64)
    if case.has("relu"):
        v = np.maximum(v, 0.0)
    if case.has("lrelu"):
        v = lrelu(v, s)
    if case.has("seq_bias"):
        v = v + inp["seq_bias"].astype(np.float64)[inp["row_seq"][rows]]
    if case.has("res16") or case.has("res32"):
        v = v + inp["res"][rows].astype(np.float64)
    res_pl, acc_pl = plane_addends(case, inp, rows)
    if res_pl is not None:
        v = v + res_pl
    if case.has("scale"):
        v = v * case.scale
    if acc_pl is not None:
        v = v + acc_pl
    if case.has("acc32"):
        v = v + inp["acc32"][rows].astype(np.float64)
    if case.has("add16"):
        v = v + inp["add16"][0][rows].astype(np.float64) + inp["add16"][1][rows].astype(np.float64)
    post = lrelu(v, s) if case.has("post") else v
    if case.mask:
        m = inp["vrow"][rows]
        v = np.where(m[:, None], v, 0.0)
        post = np.where(m[:, None], post, 0.0)
    return (v if case.has("before_post") else post), post


def expected(case, inp, rows=None, *, dil=None, center=None, w=None):
    """-> dict(out32 fp32, out16 fp16 = round-to-nearest-even of the exact value) for the output rows ``rows`` (default: all).  dil / center / w override
    the case's own (the negative controls evaluate a deliberately different problem)."""
    rows = np.arange(case.M) if rows is None else np.asarray(rows)
    dil = case.dil if dil is None else dil
    center = case.center if center is None else center
    v = sum(conv(xp, wp, case.taps, dil, center, rows) for xp, wp in operand_parts(case, inp, w))
    v32, v16 = epilogue(case, inp, v, rows)
    o32 = v32.astype(np.float32)
    assert np.array_equal(o32.astype(np.float64), v32), "the exact value is not an fp32 number: the budget does not hold"
    return dict(out32=o32, out16=v16.astype(np.float16), exact=v16)


def plane_set(v, slope=1.0):
    """mxfp4 on the exact value after the consumer's slope -> (fp16 hi, codes hi, codes lo, scale bytes hi, scale bytes lo), block 32"""
    a = lrelu(np.asarray(v, np.float64), slope).astype(np.float32)
    hi, lo = mxfp4.split_hi_lo(a)
    ch, sh = mxfp4.quantize(hi, 32)
    cl, sl = mxfp4.quantize(lo, 32)
    return hi.astype(np.float16), ch, cl, sh, sl


def budget(case, inp, exact_flop_limit=4e10):
    """bits of  (sum of |every term the kernel adds| / smallest quantum among them), the worst output element.  Below LIMIT_BITS every partial sum in any
    order is an integer below 2^24 times the quantum: exact in fp32.  Per element where that is affordable; otherwise the per-column bound
    sum_k |w[n, t, k]| max_rows |x[:, k]| (an upper bound of every element of the column)."""
    parts = operand_parts(case, inp)
    q = min(quantum(xp) * quantum(wp) for xp, wp in parts)
    rows = np.arange(case.M)
    if 2.0 * case.M * case.N * case.K * case.taps * len(parts) <= exact_flop_limit:
        mag = sum(conv(np.abs(xp), np.abs(wp), case.taps, case.dil, case.center, rows) for xp, wp in parts)
    else:
        mag = sum(np.abs(wp).astype(np.float64).sum(1) @ np.abs(xp).max(0).astype(np.float64) for xp, wp in parts)[None, :]
    res_pl, acc_pl = plane_addends(case, inp, rows)
    for name in ("bias", "seq_bias", "res", "respl", "scale", "acc32", "accpl", "add16"):
        if name in ("respl", "accpl"):
            t = res_pl if name == "respl" else acc_pl
            if t is not None:
                mag, q = mag + np.abs(t), min(q, quantum(t))
        elif name == "scale" and case.has("scale"):
            mag, q = mag * case.scale, q * case.scale
        elif name == "add16" and case.has("add16"):
            a, b = inp["add16"]
            mag = mag + np.abs(a.astype(np.float64)) + np.abs(b.astype(np.float64))
            q = min(q, quantum(a), quantum(b))
        elif name == "seq_bias" and case.has("seq_bias"):
            mag, q = mag + np.abs(inp["seq_bias"]).max(0).astype(np.float64), min(q, quantum(inp["seq_bias"]))
        elif name in ("bias", "res", "acc32") and (case.has(name) or (name == "res" and (case.has("res16") or case.has("res32")))):
            t = np.abs(inp[name].astype(np.float64))
            mag, q = mag + (t if t.ndim == 2 else t[None, :]), min(q, quantum(t))
    if case.has("lrelu"):
        q *= case.slope
    if case.has("post"):
        q *= case.slope
    if not np.isfinite(q):
        return 0.0
    return float(np.log2(max(mag.max(), q) / q))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# comparison
def _codes(packed):
    """packed fp4 bytes -> one code per element, -0 (code 8) folded onto +0"""
    p = np.asarray(packed, np.uint8)
    c = np.empty(p.shape[:-1] + (p.shape[-1] * 2,), np.uint8)
    c[..., 0::2] = p & 15
    c[..., 1::2] = p >> 4
    return np.where(c == 8, 0, c)


def mismatches(got, want, kind="value"):
    """-> (count, message).  kind "value": numeric equality on every element (+-0 equal), everything finite; "codes": packed fp4 bytes, code 8 == code 0;
    "bytes": plain byte equality (scale bytes)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if kind == "codes":
        got, want = _codes(got), _codes(want)
    if kind == "value":
        g, w_ = got.astype(np.float64), want.astype(np.float64)
        bad = ~(np.isfinite(g) & (g == w_))
    else:
        bad = got != want
    n = int(bad.sum())
    if n == 0:
        return 0, ""
    bad2 = bad.reshape(bad.shape[0], -1) if bad.ndim > 1 else bad.reshape(-1, 1)
    g2, w2 = got.reshape(bad2.shape), want.reshape(bad2.shape)
    idx = np.argwhere(bad2)
    first = ["(%d, %d) got %r want %r" % (r, c, g2[r, c].item(), w2[r, c].item()) for r, c in idx[:6]]
    msg = "%d of %d elements differ (%d rows, %d columns); first: %s; rows mod 256: %s; columns mod 128: %s" % (
        n, bad.size, len(np.unique(idx[:, 0])), len(np.unique(idx[:, 1])), "; ".join(first),
        sorted(set((idx[:, 0] % 256).tolist()))[:16], sorted(set((idx[:, 1] % 128).tolist()))[:16])
    return n, msg


def compare(got, want, kind="value", what=""):
    n, msg = mismatches(got, want, kind)
    assert n == 0, "%s: %s" % (what, msg)
    return int(np.asarray(want).size)
