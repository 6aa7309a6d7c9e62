"""Every activation quantiser of the device against emotivoice_amd/mxfp4.py where its decisions are close (MI355X): byte equality, no tolerance.

The inputs are the probe blocks of tests/quant_probes.py (block maxima at every mantissa that could move the scale, elements on every rounding threshold of
the fp4 grid and on both representable neighbours, the fp16 split at its ties, E5M2 at its ties; domain: finite, |v| < 65520, v == 0 or |v| >= 2^-100).
Each site is reached through its entry point at the smallest shape its launcher takes, by a route on which the probes arrive EXACTLY -- zero weights and the
probes as the fp32 residual / addend, gamma = 0 and the probes as beta, the probes as the input itself, a routing weight of exactly 1.0 -- and every route's
precondition is asserted on the CPU before the launch.  Compared: the fp16 hi plane by value, the fp4 codes with code 8 (-0) folded onto code 0 (as
exact_lattice.mismatches does), the scale bytes plain, slack rows and sentinels untouched.  quant_edges_report.json, written next to parity_report.json,
records per site the kernel, the delivery route, the probe blocks run, the probes dropped, the thresholds covered and the mismatches.

What each route reaches is the whole probe set except:
  conv_gemm_mx_up_kernel   has no fp32 addend: its value is hi + Q4(lo) of an input plane set.  The hi plane is free (every hi-plane probe block, each with an
                           fp4-grid remainder underneath), the remainder plane is on the fp4 grid (pin mantissas 1 and 1.5; nothing rounds there).
  the fused C = 32 pairs   take non-negative activations only (their leaky-relu slope 0.1 is not dyadic) and show their two quantisers only through out32; see
                           the section at the end of the file and quant_probes.pair_expected."""
import ctypes as C

import numpy as np
import pytest

import exact_lattice as EL
import quant_probes as QP
from exact_lattice import PAD, Case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_exact import _KEEP, _host_planes, _sync_or_stop, build_desc      # noqa: E402
from test_gpu_ops import _PlaneSet, lib      # noqa: E402, F401  (lib: the module-scoped library fixture)
from test_gpu_parity import _report as write_report      # noqa: E402

REPORT = {}
SLOPES = (1.0, 0.125)          # the consumer's slope of an emitted plane set: none, and a dyadic one (the probes' pre-image goes in)


def tile_blocks(M, K, blocks=None):
    """the probe blocks as an [M][K] fp32 tensor, block j in row j // (K / 32), the rest zero -> (tensor, blocks placed)"""
    blocks = QP.BLOCKS if blocks is None else blocks
    per = K // 32
    n = min(len(blocks), M * per)
    v = np.zeros((M * per, 32), np.float32)
    v[:n] = blocks[:n]
    return v.reshape(M, K), n


def preimage(v, slope):
    """w with lrelu(w, slope) == v exactly (slope dyadic: the division and the kernel's multiplication are exact inside the domain)"""
    w = np.where(np.signbit(v), v / np.float32(slope), v).astype(np.float32)
    back = np.where(w > 0, w, w * np.float32(slope)).astype(np.float32)
    assert np.array_equal(back.view(np.uint32), v.view(np.uint32)) and np.isfinite(w).all()
    return w


def padded(a):
    x = np.zeros((a.shape[0] + 2 * PAD, a.shape[1]), a.dtype)
    x[PAD:PAD + a.shape[0]] = a
    return x


def same_bits_or_zero(got, want):
    """bitwise equality of two fp32 arrays; a zero may have either sign (0 + -0 = +0 in the epilogue's sums)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0))))


def host_plane_set(v):
    """mxfp4.py on v [rows][C] -> (fp16 hi, packed codes hi, packed codes lo, scale bytes hi [rows][C / 32], scale bytes lo)"""
    return EL.plane_set(v, 1.0)


def plane_mismatches(got, v, what):
    """got = (h [rows][C] fp16, [codes hi, codes lo] packed, [scales hi, scales lo] [rows][C / 32]) as numpy arrays -> (count, messages)"""
    h16, ch, cl, sh, sl = host_plane_set(v)
    n_bad, msgs = 0, []
    for name, g, w, kind in (("h", got[0], h16, "value"), ("q4[0]", got[1][0], ch, "codes"), ("q4[1]", got[1][1], cl, "codes"),
                             ("qs[0]", got[2][0], sh, "bytes"), ("qs[1]", got[2][1], sl, "bytes")):
        n, msg = EL.mismatches(g, w, kind)
        n_bad += n
        if n:
            msgs.append("%s plane %s: %s" % (what, name, msg))
    return n_bad, msgs


def read_plane_set(ps, rows, Cc):
    """the valid rows of a _PlaneSet as numpy, after asserting that its slack rows kept their sentinels"""
    assert bool((ps.h[:PAD] == 3.0).all()) and bool((ps.h[PAD + rows:] == 3.0).all()), "hi-plane slack rows written"
    for i in range(2):
        assert bool((ps.q4[i][:PAD] == 0x77).all()) and bool((ps.q4[i][PAD + rows:] == 0x77).all()), "code-plane slack rows written"
        assert bool((ps.qs[i][:, :PAD] == 130).all()) and bool((ps.qs[i][:, PAD + rows:] == 130).all()), "scale-plane slack rows written"
    if Cc == 64:
        qs = [ps.qs[i][0, PAD:PAD + rows, :2].cpu().numpy() for i in range(2)]
    else:
        qs = [ps.qs[i][:, PAD:PAD + rows].permute(1, 0, 2).reshape(rows, Cc // 32).cpu().numpy() for i in range(2)]
    return ps.h[PAD:PAD + rows].cpu().numpy(), [ps.q4[i][PAD:PAD + rows].cpu().numpy() for i in range(2)], qs


def covered(n_blocks, blocks_idx=None):
    """the (plane, threshold) pairs whose on-tie probe is among the first n_blocks probe blocks (or the given ones), as strings for the report"""
    idx = np.arange(n_blocks) if blocks_idx is None else np.asarray(blocks_idx)
    out = []
    for plane in (0, 1):
        for t in range(8):
            if ((QP.PLANE[idx] == plane)[:, None] & (QP.THR[idx] == t) & ((QP.SIDE[idx] == 0) | (t == QP.SAT))).any():
                out.append("%s:%s" % ("hi" if plane == 0 else "lo", "sat" if t == QP.SAT else QP.THRESHOLDS[t]))
    return out


def record(site, kernel, route, n_blocks, dropped, thresholds, n_bad):
    write_report(site, dict(kernel=kernel, route=route, probe_blocks=int(n_blocks), probes_dropped=int(dropped), thresholds_covered=thresholds,
                            mismatches=int(n_bad)), "quant_edges_report.json", REPORT)


def launch(lib, d, what):
    torch.cuda.synchronize()
    rc = lib.ev_op_conv_gemm(C.byref(d), None)
    _sync_or_stop(what)
    assert rc == 0, (what, rc)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# mx_planes_kernel: the probes are the fp32 input; the planes are read from mx_scratch through ev_op_mx_scratch_planes
def scratch_planes(lib, scratch, M, K):
    """views of the plane set that a dtype-3 launch with an fp32 [M][K] input leaves in its scratch (the layout is the library's: ev_op_mx_scratch_planes)
    -> (h, [codes], [scales [M][K / 32]], bool mask of the scratch bytes that belong to rows 0 .. M of a plane)"""
    out = (C.c_uint64 * 6)()
    assert lib.ev_op_mx_scratch_planes(scratch.data_ptr(), M, K, out) == 0
    base, nb = scratch.data_ptr(), scratch.numel()
    off = [int(a) - base for a in out[:5]]
    stride = int(out[5])
    assert all(0 <= o < nb for o in off) and stride % 4 == 0 and stride // 4 >= M
    mine = torch.zeros(nb, dtype=torch.bool, device="cuda")
    h = scratch[off[0]:off[0] + M * K * 2].view(torch.float16).reshape(M, K)
    mine[off[0]:off[0] + M * K * 2] = True
    q4, qs = [], []
    for i in range(2):
        q4.append(scratch[off[1 + i]:off[1 + i] + M * K // 2].reshape(M, K // 2))
        mine[off[1 + i]:off[1 + i] + M * K // 2] = True
        chunks = []
        for c in range(K // 128):
            o = off[3 + i] + c * stride
            assert o + M * 4 <= nb
            chunks.append(scratch[o:o + M * 4].reshape(M, 4))
            mine[o:o + M * 4] = True
        qs.append(torch.cat(chunks, 1))
    return h, q4, qs, mine


def run_planes_kernel(lib, v, slope):
    """v [M][K] through ev_op_conv_gemm (dtype 3, fp32 A, zero weights) -> (plane set in the scratch as numpy, out32)"""
    M, K = v.shape
    case = Case("planes_%d_%g" % (K, slope), "mx_planes_kernel", 3, M, K, 128, 3, epi=("pro",) if slope != 1.0 else (), outs="32", slope=slope if slope != 1.0 else 0.5)
    inp = dict(x=padded(preimage(v, slope)), w=np.zeros((128, 3, K), np.float32))
    d, outs = build_desc(lib, case, inp)
    nb = lib.ev_op_mx_scratch_bytes(M, K)
    scratch = torch.full((nb,), 0x5a, dtype=torch.uint8, device="cuda")          # (finite everywhere: 0x5a5a is an fp16 number, 0x5a an E8M0 scale)
    d.mx_scratch, d.mx_scratch_size = scratch.data_ptr(), nb
    launch(lib, d, case.name)
    h, q4, qs, mine = scratch_planes(lib, scratch, M, K)
    assert bool((scratch[~mine] == 0x5a).all()), "mx_planes_kernel wrote outside rows 0 .. M of its planes"
    got = (h.cpu().numpy(), [q.cpu().numpy() for q in q4], [s.cpu().numpy() for s in qs])
    assert not outs["out32"][PAD:PAD + M].any(), "zero weights: the conv output is zero"
    del _KEEP[:]
    return got


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("slope", SLOPES)
def test_mx_planes_kernel(lib, K, slope):
    """mx_planes_kernel (software codes: mx_fp4_code / mx_scale_byte), M 256, K 128 / 256, without and with the leaky-relu prologue"""
    v, n = tile_blocks(256, K)
    assert n == len(QP.BLOCKS) and QP.in_domain(v)
    got = run_planes_kernel(lib, v, slope)
    n_bad, msgs = plane_mismatches(got, v, "mx_planes_kernel K=%d slope=%g" % (K, slope))
    record("mx_planes_kernel:K%d:slope%g" % (K, slope), "mx_planes_kernel", "the probes are the fp32 input" + (" (pre-image of the prologue's leaky-relu)" if slope != 1 else ""),
           n, 0, covered(n), n_bad)
    assert n_bad == 0, "\n".join(msgs)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# mx_quant8 behind the conv-GEMM plane epilogues: zero weights, zero input planes, no bias, out_scale 1, the probes as the fp32 residual or addend
def run_epilogue(lib, v, slope, taps, Cc, via, r0=0):
    """v [M][Cc] as res32 (via "res32") or acc32 (via "acc32", the residual then zero) of a zero conv -> the emitted plane set as numpy"""
    M = v.shape[0]
    w = preimage(v, slope)
    epi = ("res32",) if via == "res32" else ("res32", "acc32")
    case = Case("epi_%s" % via, "", 3, M, Cc, Cc, taps, epi=epi, outs="32", extra=("planes_in", "mxo") + (("r0=%d" % r0,) if r0 else ()))
    inp = dict(x=np.zeros((M + 2 * PAD, Cc), np.float32), w=np.zeros((Cc, taps, Cc), np.float32))
    if via == "res32":
        inp["res"] = w
    else:
        inp["res"], inp["acc32"] = np.zeros_like(w), w
    d, outs = build_desc(lib, case, inp)
    assert d.out_scale == 1.0 and not d.bias
    d.mxo_slope = slope
    launch(lib, d, "%s C=%d taps=%d r0=%d" % (via, Cc, taps, r0))
    assert same_bits_or_zero(outs["out32"][PAD:PAD + M].cpu().numpy(), w), "out32 is not the addend: the probes did not arrive exactly"
    assert bool((outs["out32"][:PAD] == 7.0).all()) and bool((outs["out32"][PAD + M:] == 7.0).all())
    got = read_plane_set(outs["ps_out"], M, Cc)
    del _KEEP[:]
    return got


EPILOGUE_SITES = [
    # site, kernel, C, taps, reserved0
    ("conv_gemm_mx_kernel<3>", "conv_gemm_mx_kernel<3, EPI_RES32|[ACC32|]O32|MXP> (mx_quant8)", 128, 3, 0),
    ("conv_gemm_mx_kernel<7>", "conv_gemm_mx_kernel<7, EPI_RES32|[ACC32|]O32|MXP> (mx_quant8)", 128, 7, 0),
    ("conv_c64_mx2_kernel<3>", "conv_c64_mx2_kernel<3, 1 / 2>", 64, 3, 0),
    ("conv_c64_mx2_kernel<7>", "conv_c64_mx2_kernel<7, 1 / 2> (reserved0 8)", 64, 7, 8),
    ("conv_c64_mx_kernel<3>", "conv_c64_mx_kernel<3, 1 / 2> (reserved0 12)", 64, 3, 12),
    ("conv_c64_mx_kernel<7>", "conv_c64_mx_kernel<7, 1 / 2> (reserved0 12)", 64, 7, 12),
    ("conv_gemm_mx64_kernel<7>", "conv_gemm_mx64_kernel<7, EPI_RES32|[ACC32|]O32|MXP>", 64, 7, 0),
]


@pytest.mark.parametrize("site", EPILOGUE_SITES, ids=[s[0] for s in EPILOGUE_SITES])
@pytest.mark.parametrize("via", ["res32", "acc32"])
def test_plane_epilogues(lib, site, via):
    """the plane-set epilogue of every conv-GEMM family at M 256 (K = N = 128 / 64): the probes as res32 and as acc32, consumer slopes 1 and 0.125"""
    name, kernel, Cc, taps, r0 = site
    v, n = tile_blocks(256, Cc)
    assert n == len(QP.BLOCKS)
    for slope in SLOPES:
        got = run_epilogue(lib, v, slope, taps, Cc, via, r0)
        n_bad, msgs = plane_mismatches(got, v, "%s %s slope=%g" % (name, via, slope))
        record("%s:%s:slope%g" % (name, via, slope), kernel, "zero weights and input planes, the probes as %s%s" % (via, " (pre-image of the consumer's leaky-relu)" if slope != 1 else ""),
               n, 0, covered(n), n_bad)
        assert n_bad == 0, "\n".join(msgs)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# conv_gemm_mx_up_kernel: no fp32 addend.  Plane-set input written by the test, a routing weight of exactly 1.0 in a tap the phase multiplies
UP_S, UP_COUT = 4, 128
UP_TAP = (0, 1, 1, 2)          # phases 0, 1 multiply taps 0 and 1, phases 2, 3 taps 1 and 2


def up_probe_values():
    """the hi-plane probe blocks, each with a remainder on the fp4 grid underneath -> (v [n][32] fp32, fp16 hi, remainder codes [n][32], remainder scale bytes [n])
    The remainder of element e is c_e 2^(E - 20), E = the binade of the block's largest hi part, c_e running through the fp4 grid (the largest-magnitude
    element gets 4 or 6): below half an ulp of every nonzero hi part of the block, zero where the hi part is zero."""
    from emotivoice_amd import mxfp4
    idx = np.flatnonzero(QP.PLANE == 0)
    hi = QP.BLOCKS[idx].astype(np.float64)
    n = len(idx)
    E = np.frexp(np.abs(hi).max(1))[1] - 1
    sb = (E - 20 + 127).astype(np.uint8)
    codes = np.zeros((n, 32), np.uint8)
    for b in range(n):
        nz = np.flatnonzero(hi[b])
        top = 6 if b % 2 else 7          # the block's largest remainder: 4 or 6 times the scale (mantissa 1 / 1.5)
        codes[b, nz] = [(1 + (j % top)) | (8 if (j // top) % 2 else 0) for j in range(len(nz))]
        codes[b, QP.PINPOS[idx[b]]] = top
    lo = mxfp4.decode_fp4(codes).astype(np.float64) * np.ldexp(1.0, E - 20)[:, None]
    v = (hi + lo).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), hi + lo)
    h, l_ = mxfp4.split_hi_lo(v)
    assert np.array_equal(h.astype(np.float64), hi) and np.array_equal(l_.astype(np.float64), lo)          # the split of v IS (hi, remainder)
    return v, hi.astype(np.float16), codes, sb, idx


def test_up_kernel(lib):
    """conv_gemm_mx_up_kernel<EPI_O32|EPI_MXP> (the mxo_logC geometry), M 256, K 128, N 512, polyphase_cout 128"""
    from emotivoice_amd import _ffi, mxfp4
    M, K, N = 256, 128, UP_S * UP_COUT
    v, h16, codes, sb, idx = up_probe_values()
    vt, n = tile_blocks(M, K, v)
    assert n == len(v) and QP.in_domain(vt)
    ht, _ = tile_blocks(M, K, h16.astype(np.float32))
    ct, _ = tile_blocks(M, K, codes.astype(np.float32))
    st = np.ones((M * K // 32,), np.uint8)
    st[:n] = sb
    ps = _PlaneSet(M, K)          # the input plane set: hi plane and remainder planes as above; hi codes zero (they meet the zero remainder of the weight)
    ps.h.zero_()
    ps.h[PAD:PAD + M] = torch.from_numpy(ht.astype(np.float16)).cuda()
    c8 = ct.astype(np.uint8)
    for i in range(2):
        ps.q4[i].zero_()
        ps.qs[i].fill_(1)
    ps.q4[1][PAD:PAD + M] = torch.from_numpy((c8[:, 0::2] | (c8[:, 1::2] << 4)).astype(np.uint8)).cuda()
    ps.qs[1][0, PAD:PAD + M] = torch.from_numpy(st.reshape(M, 4)).cuda()
    w = np.zeros((N, 3, K), np.float32)
    for ph in range(UP_S):
        for c in range(UP_COUT):
            w[ph * UP_COUT + c, UP_TAP[ph], c] = 1.0
    assert not w[:N // 2, 2].any() and not w[N // 2:, 0].any()          # the zero tap of every phase really is zero
    ql, qh = mxfp4.weight_planes_dequant(mxfp4.pack_weight_planes(w), N, 3, K)
    assert np.array_equal(qh, w) and not ql.any()          # 1.0 is exact in the weight planes under W_RULE
    case = Case("up", "conv_gemm_mx_up_kernel", 3, M, K, N, 3, epi=(), outs="32", extra=("planes_in", "mxo", "up4"))
    inp = dict(x=np.zeros((M + 2 * PAD, K), np.float32), w=w, up=(UP_S, UP_COUT))
    for slope in SLOPES:
        # (the value is fixed by the input planes: with a slope the negative probes arrive divided by it -- still hi + grid remainder, so the planes are of
        #  lrelu(v / slope) = v only where v >= 0; the expected planes are therefore computed from what arrives, lrelu(value, slope))
        d, outs = build_desc(lib, case, inp, ps)
        d.mxo_slope = slope
        launch(lib, d, "up slope=%g" % slope)
        want = np.zeros((M + 2, K), np.float32)          # output row m s + ph = input row m + UP_TAP[ph] - 1
        want[1:M + 1] = vt
        exp = np.stack([want[UP_TAP[ph]:UP_TAP[ph] + M] for ph in range(UP_S)], 1).reshape(M * UP_S, UP_COUT)
        got32 = outs["out32"][PAD:PAD + M].cpu().numpy().reshape(M * UP_S, UP_COUT)
        assert same_bits_or_zero(got32, exp), "out32 is not hi + Q4(lo) of the input planes: the probes did not arrive exactly"
        arrived = np.where(exp > 0, exp, exp * np.float32(slope)).astype(np.float32)
        got = read_plane_set(outs["ps_out"], M * UP_S, UP_COUT)
        n_bad, msgs = plane_mismatches(got, arrived, "up slope=%g" % slope)
        record("conv_gemm_mx_up_kernel:slope%g" % slope, "conv_gemm_mx_up_kernel<EPI_O32|EPI_MXP>",
               "plane-set input written by the test, routing weight 1.0: hi plane free (every hi-plane block), remainder plane on the fp4 grid (lossless; pins 1 and 1.5)",
               n, 0, [c for c in covered(0, idx) if c.startswith("hi")], n_bad)
        assert n_bad == 0, "\n".join(msgs)
        del _KEEP[:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# resblock_pair_c64_mx_kernel<true>: zero weights, biases and input planes, the probes as acc32
class _UnitScale:
    """the library with the pair entry points' out_scale set to 1 (the harness classes of test_gpu_pair_long.py fix 1 / 3)"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ev_op_resblock_pair"):
            return fn

        def call(ref, stream):
            ref._obj.epi.out_scale = 1.0
            return fn(ref, stream)
        return call


class _AllValid:
    """what the pair harness classes read of a layout: every row valid"""

    def __init__(self, M):
        self.M, self.vrow = M, torch.ones(M, dtype=torch.bool)
        self.vrow_d = self.vrow.cuda()
        self.valid = torch.ones(M // 8, dtype=torch.uint8, device="cuda")


def test_pair_c64_planes(lib):
    """resblock_pair_c64_mx_kernel<true> (ev_op_resblock_pair_c64_mx, M 256, planes + out32): everything zero but the fp32 accumulate-in"""
    import test_gpu_pair_long as PL
    from emotivoice_amd import mxfp4
    M, Cc = 256, 64
    v, n = tile_blocks(M, Cc)
    assert n == len(QP.BLOCKS)
    L = _AllValid(M)
    z = np.zeros((Cc, 3, Cc), np.float32)
    wset = (torch.zeros(Cc, 3, Cc, dtype=torch.float16, device="cuda"), None, torch.from_numpy(mxfp4.pack_c64_weight_planes(z)).cuda())
    ps_in = _host_planes(np.zeros((M + 2 * PAD, Cc), np.float32))
    for slope in SLOPES:
        w = preimage(v, slope)
        inp = dict(L=L, w1=wset, w2=wset, b1=torch.zeros(Cc, device="cuda"), b2=torch.zeros(Cc, device="cuda"), acc=torch.from_numpy(w).cuda())
        K = PL._C64Mx(_UnitScale(lib), inp, 1, "acc+o32+planes", slope=slope)
        torch.cuda.synchronize()
        out, ps = K.fused(ps_in, L.valid, 0, M)
        _sync_or_stop("pair c64")
        assert same_bits_or_zero(out[PAD:PAD + M].cpu().numpy(), w), "out32 is not acc32: the probes did not arrive exactly"
        assert bool((out[:PAD] == 7.0).all()) and bool((out[PAD + M:] == 7.0).all())
        got = read_plane_set(ps, M, Cc)
        n_bad, msgs = plane_mismatches(got, v, "pair c64 slope=%g" % slope)
        record("resblock_pair_c64_mx_kernel:slope%g" % slope, "resblock_pair_c64_mx_kernel<true>", "zero weights, biases and input planes, the probes as acc32",
               n, 0, covered(n), n_bad)
        assert n_bad == 0, "\n".join(msgs)
    del _KEEP[:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm planes: gamma = 0, so y = beta
def run_layernorm(lib, beta, rows=8):
    """-> (plane set as numpy, the kernel's fp32 output from ev_op_layernorm on the same inputs)"""
    Cc = beta.size
    x = torch.linspace(-1.0, 2.0, rows * Cc, device="cuda").reshape(rows, Cc).contiguous()
    g, b = torch.zeros(Cc, device="cuda"), torch.from_numpy(beta).cuda()
    valid = torch.ones(rows, dtype=torch.uint8, device="cuda")
    y = torch.full((rows, Cc), 9.0, device="cuda")
    assert lib.ev_op_layernorm(x.data_ptr(), rows, Cc, g.data_ptr(), b.data_ptr(), 1e-12, valid.data_ptr(), None, y.data_ptr(), None, 0.0, None, None) == 0
    ps = _PlaneSet(rows, Cc)
    assert lib.ev_op_layernorm_planes(x.data_ptr(), rows, Cc, g.data_ptr(), b.data_ptr(), 1e-12, valid.data_ptr(), ps.h[PAD:].data_ptr(), ps.q4[0][PAD:].data_ptr(),
                                      ps.q4[1][PAD:].data_ptr(), ps.qs[0][0, PAD:].data_ptr(), ps.qs[1][0, PAD:].data_ptr(), ps.R * 4, None) == 0
    _sync_or_stop("layernorm planes")
    return read_plane_set(ps, rows, Cc), y.cpu().numpy()


@pytest.mark.parametrize("Cc", [128, 512])
def test_layernorm_planes(lib, Cc):
    """the LayerNorm plane epilogue (software codes, ev_misc.hip) at C 128 / 512, 8 rows: gamma = 0, beta = C / 32 probe blocks per launch, every row the same"""
    per = Cc // 32
    nb = len(QP.BLOCKS)
    n_bad, msgs = 0, []
    for first in range(0, nb, per):
        blk = np.zeros((per, 32), np.float32)
        chunk = QP.BLOCKS[first:first + per]
        blk[:len(chunk)] = chunk
        beta = blk.reshape(-1)
        got, y = run_layernorm(lib, beta)
        v = np.tile(beta, (8, 1))
        assert same_bits_or_zero(y, v), "LayerNorm with gamma = 0 is not beta: the probes did not arrive exactly"
        n, m = plane_mismatches(got, v, "layernorm C=%d blocks %d.." % (Cc, first))
        n_bad += n
        msgs += m
    record("layernorm_planes:C%d" % Cc, "layernorm_kernel<4, true> (mx_fp4_code / mx_scale_byte)", "gamma = 0, the probes as beta", nb, 0, covered(nb), n_bad)
    assert n_bad == 0, "\n".join(msgs[:8])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_site_gives_one_plane_set(lib):
    """the same fp32 probe tensor through mx_planes_kernel, the res32 route of conv_gemm_mx_kernel<3>, LayerNorm with gamma = 0 (its first 16 blocks) and the host
    quantiser: one plane set (the "same bits from either input form" guarantee of the engine)"""
    v, n = tile_blocks(256, 128)
    a = run_planes_kernel(lib, v, 1.0)
    b = run_epilogue(lib, v, 1.0, 3, 128, "res32")
    h16, ch, cl, sh, sl = host_plane_set(v)
    fold = EL._codes
    n_bad = 0
    for x in (a, b):
        n_bad += int((x[0].astype(np.float32) != h16.astype(np.float32)).sum())
        n_bad += int((fold(x[1][0]) != fold(ch)).sum() + (fold(x[1][1]) != fold(cl)).sum() + (x[2][0] != sh).sum() + (x[2][1] != sl).sum())
    n_bad += int((a[0].astype(np.float32) != b[0].astype(np.float32)).sum() + sum((fold(a[1][i]) != fold(b[1][i])).sum() + (a[2][i] != b[2][i]).sum() for i in range(2)))
    beta = v.reshape(-1)[:512]          # the first 16 blocks = the first four rows of the tensor
    c, y = run_layernorm(lib, beta)
    assert same_bits_or_zero(y, np.tile(beta, (8, 1)))
    row = beta.reshape(4, 128)
    for r in range(4):
        for x in (a, b):
            n_bad += int((c[0][0, 128 * r:128 * r + 128].astype(np.float32) != x[0][r].astype(np.float32)).sum())
            for i in range(2):
                n_bad += int((fold(c[1][i][0, 64 * r:64 * r + 64]) != fold(x[1][i][r])).sum() + (c[2][i][0, 4 * r:4 * r + 4] != x[2][i][r]).sum())
    assert row.any()
    record("cross-site", "mx_planes_kernel / conv_gemm_mx_kernel<3> res32 / layernorm_kernel<4, true> / mxfp4.py", "one fp32 probe tensor through every site", n, 0, covered(n), n_bad)
    assert n_bad == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The fused C = 32 pairs: resblock_pair_c32_e5_kernel (reserved0 32), resblock_pair_c32_mx2_kernel (16), resblock_pair_c32_mx_kernel (16 | 4), k 3 and 7.
# Their quantisers -- of the fp32 input x and of the intermediate xt in LDS -- show only through out32.  The convs are identities at the centre tap whose
# weights (1 + 2^-13, 1.0, -1.0) are exact in the weight planes (tests/test_quant_probes.py), b2 = 0, out_scale 1, no acc32, so that every output element is
# a short exact sum of the host functions' values for ONE operand element (quant_probes.pair_expected, in fp64; elements whose sum is not an fp32 number at
# every step are dropped and counted, and test_quant_probes.py holds the drop and coverage conditions on the CPU):
#   intermediate quantiser   x = 0, b1 = one probe block (C = 32 is exactly one scale block), conv2 = 1 + 2^-13: one launch per block, M 256
#   input quantiser          x = the probe blocks, one per row (M 1024), b1 = 0, conv2 = -1.0 and conv1 = 1.0 (reads the remainder plane) / 1 + 2^-13 (the hi plane)
# The kernels take their residual from x itself (epi.res is documented as "= x" and not read), hence conv2 = MINUS the identity on the input routes: the
# residual cancels the hi part and the result stays an fp32 number.  Non-negative probes only: the same restriction test_gpu_exact.py states for its pair cases.
PAIR_KERNELS = [("e5m2", 32, "resblock_pair_c32_e5_kernel"), ("fp4", 16, "resblock_pair_c32_mx2_kernel"), ("fp4", 16 | 4, "resblock_pair_c32_mx_kernel")]
_PAIR_PROBES = {}


def pair_probes(fmt):
    """-> {route: (rows fed [n][32] fp32 >= 0, expected fp32, compared mask, survival record)}, computed once per format"""
    if fmt not in _PAIR_PROBES:
        rows = QP.BLOCKS[QP.NONNEG] if fmt == "fp4" else QP.e5_rows()[0]
        per = {}
        for route in QP.PAIR_ROUTES:
            u = QP.pair_feed(rows, fmt, route)          # (an element whose intermediate would leave the domain is fed as zero and counted as dropped)
            assert QP.in_domain(u) and not np.signbit(u).any()
            want, ok = QP.pair_expected(u, fmt, route)
            w32 = np.where(ok, want, 0.0).astype(np.float32)
            assert np.array_equal(w32.astype(np.float64)[ok], want[ok])          # the expected value IS an fp32 number wherever it is compared
            per[route] = (np.ascontiguousarray(u), w32, ok, QP.pair_survival(fmt, route))
        _PAIR_PROBES[fmt] = per
    return _PAIR_PROBES[fmt]


def make_pair(lib, M, k, dil, w1, w2):
    """test_gpu_pair_long._MxPair with the given GEMM-layout weights, zero biases, out_scale 1"""
    import test_gpu_pair_long as PL
    from emotivoice_amd import mxfp4
    for w in (w1, w2):          # the precondition: hi part and remainder of the routing weights are exact in the planes the kernel multiplies
        hi, lo = mxfp4.split_hi_lo(w)
        ql, qh = mxfp4.pair_weight_planes_dequant(mxfp4.pack_pair_weight_planes(w), k)
        assert np.array_equal(ql, lo) and np.array_equal(qh, hi)
    P = PL._MxPair(_UnitScale(lib), _AllValid(M), k, dil, False, 1)
    P.b1, P.b2 = torch.zeros(32, device="cuda"), torch.zeros(32, device="cuda")
    P.w1h, P.w2h = (torch.from_numpy(w.astype(np.float16)).cuda() for w in (w1, w2))
    P.w1m, P.w2m = (torch.from_numpy(mxfp4.pack_pair_weight_planes(w)).cuda() for w in (w1, w2))
    return P


def pair_record(site, kernel, route, fmt, surv, n_blocks, n_bad):
    keys = sorted("%s:%s" % (("hi", "lo")[k[0]] if fmt == "fp4" else k[0], QP.THRESHOLDS[k[1]] if fmt == "fp4" else "/".join(str(x) for x in k[1:]))
                  for k, n in surv["thresholds"].items() if n > 0)
    record(site, kernel, route, n_blocks, surv["dropped_elements"], keys, n_bad)


@pytest.mark.parametrize("k,dil", [(3, 1), (7, 3)])
@pytest.mark.parametrize("kern", PAIR_KERNELS, ids=[p[2] for p in PAIR_KERNELS])
def test_pair_c32_intermediate_quantiser(lib, kern, k, dil):
    """the quantiser of xt: x = 0, b1 = a probe block, conv2 = the identity of weight 1 + 2^-13; every row of out32 is u_h + 2^-13 Q(u_h) + Q(u_l)"""
    fmt, r0, kernel = kern
    M = 256
    u, want, ok, surv = pair_probes(fmt)["intermediate"]
    P = make_pair(lib, M, k, dil, QP.pair_identity(k, 1.0), QP.pair_identity(k, 1.0 + 2.0 ** -13))
    x = torch.zeros(M + 2 * PAD, 32, device="cuda")
    u_d, want_d, ok_d = torch.from_numpy(u).cuda(), torch.from_numpy(want).cuda(), torch.from_numpy(ok).cuda()
    bad = torch.zeros(len(u), 32, dtype=torch.int64, device="cuda")          # per block and channel: rows that differ
    guard = torch.zeros((), dtype=torch.int64, device="cuda")
    for b in range(len(u)):
        P.b1 = u_d[b]
        out = P.run(x, P.L.valid, 0, M, r0)
        bad[b] = ((out[PAD:PAD + M] != want_d[b]) & ok_d[b]).sum(0)
        guard += (out[:PAD] != 7.0).sum() + (out[PAD + M:] != 7.0).sum()
    _sync_or_stop("pair c32 intermediate")
    assert int(guard) == 0, "guard rows written"
    bad = bad.cpu().numpy()
    n_bad = int(bad.sum())
    first = ["block %d element %d (u = %r, want %r): %d rows differ" % (b, c, float(u[b, c]), float(want[b, c]), bad[b, c]) for b, c in np.argwhere(bad)[:6]]
    pair_record("%s:k%d:intermediate" % (kernel, k), "%s<%d>" % (kernel, k), "x = 0, b1 = one probe block per launch, conv2 = identity (1 + 2^-13)", fmt, surv, len(u), n_bad)
    assert n_bad == 0, (kernel, k, n_bad, first)


@pytest.mark.parametrize("k,dil", [(3, 1), (7, 3)])
@pytest.mark.parametrize("kern", PAIR_KERNELS, ids=[p[2] for p in PAIR_KERNELS])
def test_pair_c32_input_quantiser(lib, kern, k, dil):
    """the quantiser of x: x = the probe blocks, one per row; conv2 = -1.0; conv1 = 1.0 shows u_l - Q(u_l), conv1 = 1 + 2^-13 shows -2^-13 Q(u_h) under fp16 probes"""
    fmt, r0, kernel = kern
    M = 1024
    for route, w1 in (("input_lo", 1.0), ("input_hi", 1.0 + 2.0 ** -13)):
        u, want, ok, surv = pair_probes(fmt)[route]
        assert len(u) <= M
        x = torch.zeros(M + 2 * PAD, 32, device="cuda")
        x[PAD:PAD + len(u)] = torch.from_numpy(u).cuda()
        P = make_pair(lib, M, k, dil, QP.pair_identity(k, w1), QP.pair_identity(k, -1.0))
        out = P.run(x, P.L.valid, 0, M, r0)
        _sync_or_stop("pair c32 input")
        assert bool((out[:PAD] == 7.0).all()) and bool((out[PAD + M:] == 7.0).all()), "guard rows written"
        got = out[PAD:PAD + M].cpu().numpy()
        assert not got[len(u):].any(), "zero rows of x give zero rows"
        bad = (got[:len(u)] != want) & ok
        n_bad = int(bad.sum())
        pair_record("%s:k%d:%s" % (kernel, k, route), "%s<%d>" % (kernel, k), "x = the probe blocks, conv1 = identity (%s), conv2 = -identity, residual x" %
                    ("1.0" if route == "input_lo" else "1 + 2^-13"), fmt, surv, len(u), n_bad)
        first = ["row %d element %d: got %r want %r (u = %r)" % (r, c, float(got[r, c]), float(want[r, c]), float(u[r, c])) for r, c in np.argwhere(bad)[:6]]
        assert n_bad == 0, (kernel, k, route, n_bad, first)
