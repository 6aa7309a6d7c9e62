"""The fused ResBlock pair kernels past one tile per block (MI355X).

Every pair kernel is persistent: a block walks tiles at a stride of the grid, and the grid is capped by the CU count.  The per-kernel tests of
test_gpu_ops.py stay below one tile per block, so everything that lives in the second and later iterations -- the prefetch of the next slab and
row-valid byte, the double-buffer flip, the row mask carried forward, the clamped last prefetch, stores draining under the next conv1, the two-block
variant's scratch aliased onto a live slab -- runs only in whole-engine tests whose whole-signal norms cannot see a few wrong rows.  Here each
kernel runs 2-3 (or more) iterations per block, on the engine's gap layout, and is held to three things:

  1. bit-identity with single-iteration launches of the same rows (the batch-invariance promise: groups of segments launched on their own, every
     block one tile, the regime the existing tests hold to the torch reference; a group's origin is a multiple of 1024 rows, not of the tile);
  2. the CPU reference per TILE (the tile's rows + 64 on each side; relative norm over the tile's own valid rows), at the bounds of the existing
     single-iteration tests -- on tiles of every iteration, the last full / partial tile and around an all-gap run;
  3. exact zeros in every invalid row (all-gap tiles included) and untouched slack rows around every output.

Row counts derive from the device's CU count; every case asserts its iteration-count condition before launching."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_ops import (PAD, _PlaneSet, _conv64, _e5_act_parts, _host_plane_set, _launch, _lrelu, _mx_act_parts,      # noqa: E402
                          _ref_conv, _rel, lib)      # noqa: E402, F401  (lib: the module-scoped library fixture)

PITCH = 1024          # rows per segment slot
VSHIFT = 3            # one row_valid byte per 8 rows


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Layout:
    """S independent segments at a pitch of 1024 rows, valid lengths in [600, 992] in steps of 8 (gaps of >= 32 rows: wider than conv1's + conv2's
    halo, <= 30 rows), one run of three segments entirely invalid (all-gap tiles), the last segment ending 40 rows short of M."""

    def __init__(self, S, seed=2024):
        g = torch.Generator().manual_seed(seed)
        lens = 600 + 8 * torch.randint(0, 50, (S,), generator=g)
        d0 = S // 3
        lens[d0:d0 + 3] = 0
        lens[-1] = 984
        self.S, self.M, self.lens, self.dead = S, S * PITCH, lens, (d0, d0 + 3)
        self.vrow = (torch.arange(PITCH)[None, :] < lens[:, None]).reshape(-1)                  # [M] bool, cpu
        self.vrow_d = self.vrow.cuda()
        self.valid = self.vrow.view(-1, 1 << VSHIFT)[:, 0].to(torch.uint8).cuda()               # row_valid bytes
        z = torch.zeros(PAD, dtype=torch.bool)
        self.vpad = torch.cat([z, self.vrow, z])                                                # vpad[i] = validity of row i - PAD

    def groups(self, max_seg):
        """consecutive segments in groups of at most max_seg, as even as possible -> [(first row, last row + 1)]"""
        n = -(-self.S // max_seg)
        per = -(-self.S // n)
        return [(s * PITCH, min(s + per, self.S) * PITCH) for s in range(0, self.S, per)]

    def pick_tiles(self, bmo, T):
        """T = tiles the whole grid takes per iteration.  -> (ntiles, >= 12 tile indices): the first two tiles, the first tile of iteration 2 and its
        neighbours, the last tile of a block that takes two, the first tiles of iteration 3, the last full and the partial last tile (the last one taken by
        a block that takes three), the all-gap tile before the first valid row after the dead run and the tile after it."""
        nt = -(-self.M // bmo)
        t_after = (self.dead[1] * PITCH) // bmo
        assert not bool(self.vrow[(t_after - 1) * bmo:t_after * bmo].any()) and bool(self.vrow[t_after * bmo:(t_after + 1) * bmo].any())
        tiles = sorted({0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, nt - 2, nt - 1, t_after - 1, t_after})
        assert len(tiles) >= 12 and nt * bmo > self.M and tiles[-1] == nt - 1
        return nt, tiles


def _big_segments(n_cu):
    """ntiles in (2 n_cu, 3 n_cu) for the 256-row kernels (246-254 output rows per tile): 160 segments on 256 CUs"""
    return 5 * n_cu // 8


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _zeros_and_slack(buf, M, vrow_d, sentinel):
    """assertion 3 on a [PAD + M + PAD][C] output buffer"""
    assert int(torch.count_nonzero(buf[PAD:PAD + M][~vrow_d])) == 0
    assert bool((buf[:PAD] == sentinel).all()) and bool((buf[PAD + M:] == sentinel).all())
    assert float(buf[PAD:PAD + M].float().abs().max()) > 0.1


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# fp16 pairs: resblock_pair_c32_kernel<K, ACC, TWOB>, resblock_pair_c64_kernel<3, ACC>
class _F16Pair:
    def __init__(self, lib, L, Cc, k, dil, accmode, seed):
        self.lib, self.L, self.Cc, self.k, self.dil, self.accmode = lib, L, Cc, k, dil, accmode
        M = L.M
        torch.manual_seed(seed)
        self.full = torch.randn(M + 2 * PAD, Cc, device="cuda").half()
        self.full[:PAD] = 0
        self.full[PAD + M:] = 0
        self.x = self.full[PAD:PAD + M]
        self.x[~L.vrow_d] = 0                          # the engine's invariant: invalid rows of every tensor are exact zeros
        self.w1 = (torch.randn(Cc, Cc, k, device="cuda") / math.sqrt(Cc * k)).half()
        self.w2 = (torch.randn(Cc, Cc, k, device="cuda") / math.sqrt(Cc * k)).half()
        self.b1, self.b2 = torch.randn(Cc, device="cuda") * 0.1, torch.randn(Cc, device="cuda") * 0.1
        self.w1g, self.w2g = self.w1.permute(0, 2, 1).contiguous(), self.w2.permute(0, 2, 1).contiguous()
        self.acc = torch.randn(M, Cc, device="cuda") if accmode == "acc32" else None
        if accmode == "add16":
            self.a16, self.b16 = torch.randn(M, Cc, device="cuda").half(), torch.randn(M, Cc, device="cuda").half()

    def run(self, full_x, valid, a0, M, reserved0=0, gmax=0):
        """launch on rows [0, M) of full_x[PAD:], the addends taken from row a0 on -> (out16, out32) with 64 sentinel rows on both sides"""
        from emotivoice_amd import _ffi
        Cc = self.Cc
        o16 = torch.full((M + 2 * PAD, Cc), 7.0, device="cuda", dtype=torch.float16)
        o32 = torch.full((M + 2 * PAD, Cc), 7.0, device="cuda")
        xp = full_x[PAD:].data_ptr()
        d = _ffi.ev_res_pair_desc()
        d.x, d.ldx, d.w1, d.b1, d.w2, d.M, d.k, d.dil = xp, Cc, self.w1g.data_ptr(), self.b1.data_ptr(), self.w2g.data_ptr(), M, self.k, self.dil
        d.gmax = gmax
        e = d.epi
        e.bias, e.res, e.res_dtype, e.ldres = self.b2.data_ptr(), xp, 0, Cc
        e.row_valid, e.valid_shift, e.out_scale = valid.data_ptr(), VSHIFT, 1.0 / 3.0
        if self.accmode == "acc32":
            e.acc32, e.ldacc = self.acc[a0:].data_ptr(), Cc
        elif self.accmode == "add16":
            e.add16_a, e.add16_b, e.ldadd = self.a16[a0:].data_ptr(), self.b16[a0:].data_ptr(), Cc
        e.post_lrelu, e.post_slope, e.out16, e.out32, e.ldo, e.out32_before_post = 1, 0.01, o16[PAD:].data_ptr(), o32[PAD:].data_ptr(), Cc, 1
        e.reserved0 = reserved0
        torch.cuda.synchronize()
        assert (self.lib.ev_op_resblock_pair_c32 if Cc == 32 else self.lib.ev_op_resblock_pair_c64)(C.byref(d), None) == 0
        torch.cuda.synchronize()
        return o16, o32

    def check_groups(self, o16, o32, max_tiles, bmo):
        """assertion 1: every group of segments alone, one tile per block, gives the bits of the big launch"""
        L, Cc = self.L, self.Cc
        for g0, g1 in L.groups(max_tiles * bmo // PITCH):
            Mg = g1 - g0
            assert -(-Mg // bmo) <= max_tiles
            xg = torch.zeros(Mg + 2 * PAD, Cc, device="cuda", dtype=torch.float16)
            xg[PAD:PAD + Mg] = self.x[g0:g1]
            vg = L.valid[g0 >> VSHIFT:g1 >> VSHIFT].clone()
            p16, p32 = self.run(xg, vg, g0, Mg)
            assert _same(p32[PAD:PAD + Mg], o32[PAD + g0:PAD + g1]), (g0, g1)
            assert _same(p16[PAD:PAD + Mg], o16[PAD + g0:PAD + g1]), (g0, g1)
            for p in (p16, p32):
                _zeros_and_slack(p, Mg, L.vrow_d[g0:g1], 7.0)

    def check_tiles(self, o16, o32, tiles, bmo, name):
        """assertion 2: the fp16-intermediate torch emulation of test_fused_resblock_pair per tile: 1e-4 on out32, 6e-4 on out16"""
        L, k, dil, M = self.L, self.k, self.dil, self.L.M
        h2 = (k - 1) // 2
        full_c, o16_c, o32_c = self.full.cpu(), o16[PAD:PAD + M].cpu(), o32[PAD:PAD + M].cpu()
        w1, w2, b1, b2 = self.w1.cpu(), self.w2.cpu(), self.b1.cpu(), self.b2.cpu()
        addend = self.acc.cpu() if self.accmode == "acc32" else (self.a16.float().cpu() + self.b16.float().cpu() if self.accmode == "add16" else None)
        worst = [0.0, 0.0]
        for t in tiles:
            m0, m1 = t * bmo, min((t + 1) * bmo, M)
            v = L.vrow[m0:m1]
            if not bool(v.any()):
                continue                                # (an all-gap tile: exact zeros, assertion 3)
            xw = full_c[m0:m1 + 2 * PAD].float()        # rows [m0 - PAD, m1 + PAD)
            vw = L.vpad[m0:m1 + 2 * PAD]
            xin = _lrelu(xw, 0.1).half().float()
            xt = _lrelu(_ref_conv(xin, w1, b1, dil, h2, k), 0.1)
            xt[~vw] = 0
            xt = xt.half().float()                      # the intermediate lives in LDS as fp16
            ref = ((_ref_conv(xt, w2, b2, 1, h2, k) + xw) * (1.0 / 3.0))[PAD:PAD + m1 - m0]
            if addend is not None:
                ref = ref + addend[m0:m1]
            r32, r16 = _rel(o32_c[m0:m1][v], ref[v]), _rel(o16_c[m0:m1][v].float(), _lrelu(ref, 0.01)[v])
            worst = [max(worst[0], r32), max(worst[1], r16)]
            assert r32 < 1e-4 and r16 < 6e-4, (name, t, r32, r16)
        print("pair-long %s: worst tile of %d  out32 %.2e (bound 1e-4)  out16 %.2e (bound 6e-4)" % (name, len(tiles), worst[0], worst[1]))


def _f16_case(lib, Cc, k, dil, accmode, twob=False):
    n_cu = _n_cu()
    h2 = (k - 1) // 2
    bmo = 256 - 2 * h2
    S = -(-4 * n_cu * bmo // PITCH) + 2 if twob else _big_segments(n_cu)          # (two-block variant: 256 segments on 256 CUs)
    L = _Layout(S)
    M = L.M
    ntiles = -(-M // bmo)
    # the launcher's rule (launch_resblock_pair_c32): two blocks per CU at C = 32, k = 3 from 4 tiles per CU on, on a grid of 2 x CUs
    assert (Cc == 32 and k == 3 and ntiles >= 4 * n_cu) == twob
    T = min(ntiles, 2 * n_cu if twob else n_cu)
    assert ntiles > 2 * T and (twob or ntiles < 3 * T), (ntiles, T)      # every block takes >= 2 tiles, some take 3
    P = _F16Pair(lib, L, Cc, k, dil, accmode, 100 + k + dil + Cc)
    name = "f16 C=%d k=%d dil=%d %s%s" % (Cc, k, dil, accmode, " two-block" if twob else "")
    o16, o32 = P.run(P.full, L.valid, 0, M)
    for o in (o16, o32):
        _zeros_and_slack(o, M, L.vrow_d, 7.0)
    if twob:
        # epi.reserved0 bit 2 = the one-block kernel on the same launch: the same bits; and run to run (the variant's transposing scratch is a live slab)
        q16, q32 = P.run(P.full, L.valid, 0, M, reserved0=4)
        assert _same(q32, o32) and _same(q16, o16)
        q16, q32 = P.run(P.full, L.valid, 0, M)
        assert _same(q32, o32) and _same(q16, o16)
        del q16, q32
    P.check_groups(o16, o32, n_cu, bmo)
    _, tiles = L.pick_tiles(bmo, T)
    P.check_tiles(o16, o32, tiles, bmo, name)
    return P, o16, o32


@pytest.mark.parametrize("k,dil,accmode", [(3, 5, "add16"), (7, 3, "acc32"), (11, 5, "none"), (11, 1, "add16")])
def test_pair_c32_long(lib, k, dil, accmode):
    """resblock_pair_c32_kernel<K, ACC, false>, 2-3 tiles per block (645-667 tiles on 256 CUs).  Worst tile of 12 against the fp16-intermediate torch
    emulation, measured on an MI355X (256 CUs), against the bounds of test_fused_resblock_pair (out32 < 1e-4, out16 < 6e-4):
      (3, 5, add16)   out32 1.96e-05  out16 2.17e-04        (7, 3, acc32)   out32 2.18e-05  out16 2.14e-04
      (11, 5, none)   out32 6.15e-05  out16 2.21e-04        (11, 1, add16)  out32 1.64e-05  out16 2.11e-04"""
    _f16_case(lib, 32, k, dil, accmode)


@pytest.mark.parametrize("dil,accmode", [(1, "add16"), (3, "acc32")])
def test_pair_c32_two_block_long(lib, dil, accmode):
    """resblock_pair_c32_kernel<3, ACC, true> (ntiles >= 4 x CUs: 1033 tiles on a grid of 512 on 256 CUs; its own 320-row slab, per-tap weight reads and
    the transposing scratch aliased onto the slab of the tile being finished), against the one-block kernel on the same launch (reserved0 bit 2), run to
    run, against single-iteration launches and the per-tile reference.  Worst tile of 12, measured on an MI355X, against the bounds out32 < 1e-4, out16 < 6e-4:
      (3, 1, add16)   out32 1.70e-05  out16 2.14e-04        (3, 3, acc32)   out32 1.97e-05  out16 2.12e-04"""
    _f16_case(lib, 32, 3, dil, accmode, twob=True)


@pytest.mark.parametrize("dil,accmode", [(1, "none"), (5, "add16"), (1, "add16"), (5, "none"), (3, "acc32")])
def test_pair_c64_long(lib, dil, accmode):
    """resblock_pair_c64_kernel<3, ACC>, 2-3 tiles per block; the transposing scratch aliases the slab buffer of the tile being finished.  Worst tile of 12,
    measured on an MI355X, against the bounds out32 < 1e-4, out16 < 6e-4:
      (1, none)   out32 6.91e-05  out16 2.19e-04        (5, add16)  out32 1.63e-05  out16 2.10e-04        (1, add16)  out32 1.81e-05  out16 2.12e-04
      (5, none)   out32 6.30e-05  out16 2.22e-04        (3, acc32)  out32 2.37e-05  out16 2.15e-04"""
    _f16_case(lib, 64, 3, dil, accmode)


def test_pair_c32_gmax_below_m(lib):
    """gmax < M (the only sub-range form left: the engine passes gmax = rows_out, gmin = 0), cutting a segment: rows [gmax, M) are exact zeros, rows below
    gmax have the bits of a launch with M = gmax.  x is zero above gmax, as the engine's arena is."""
    n_cu = _n_cu()
    k, dil, bmo = 7, 3, 250
    L = _Layout(_big_segments(n_cu))
    M = L.M
    gmax = (L.S - 2) * PITCH + 504
    assert -(-gmax // bmo) > 2 * n_cu and bool(L.vrow[gmax]) and bool(L.vrow[gmax - 1])
    P = _F16Pair(lib, L, 32, k, dil, "acc32", 77)
    P.full[PAD + gmax:] = 0
    o16, o32 = P.run(P.full, L.valid, 0, M, gmax=gmax)
    xs = torch.zeros(gmax + 2 * PAD, 32, device="cuda", dtype=torch.float16)
    xs[PAD:PAD + gmax] = P.x[:gmax]
    p16, p32 = P.run(xs, L.valid, 0, gmax)
    vr = L.vrow_d.clone()
    vr[gmax:] = False
    for o, p in ((o16, p16), (o32, p32)):
        _zeros_and_slack(o, M, vr, 7.0)
        assert _same(o[PAD:PAD + gmax], p[PAD:PAD + gmax])
        assert float(o[PAD + gmax - 8:PAD + gmax].float().abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The C = 32 MX pairs: resblock_pair_c32_e5_kernel (128-row tiles, two per block and iteration), resblock_pair_c32_mx2_kernel (the same schedule, fp4),
# resblock_pair_c32_mx_kernel (lock-step, 256-row tiles)
class _MxPair:
    def __init__(self, lib, L, k, dil, acc_in, seed):
        from emotivoice_amd import mxfp4
        self.lib, self.L, self.k, self.dil, self.acc_in = lib, L, k, dil, acc_in
        M, Cc = L.M, 32
        torch.manual_seed(seed)
        self.full = torch.randn(M + 2 * PAD, Cc, device="cuda") * torch.exp(0.7 * torch.randn(M + 2 * PAD, 1, device="cuda"))
        self.full[:PAD] = 0
        self.full[PAD + M:] = 0
        self.x = self.full[PAD:PAD + M]
        self.x[~L.vrow_d] = 0
        w1 = torch.randn(Cc, Cc, k, device="cuda") / math.sqrt(Cc * k)
        w2 = torch.randn(Cc, Cc, k, device="cuda") / math.sqrt(Cc * k)
        self.b1, self.b2 = torch.randn(Cc, device="cuda") * 0.1, torch.randn(Cc, device="cuda") * 0.1
        self.acc = torch.randn(M, Cc, device="cuda")

        def wparts(w):
            wg = w.permute(0, 2, 1).contiguous().cpu().numpy()            # [N][taps][K]
            planes = mxfp4.pack_pair_weight_planes(wg)
            ql, qh = mxfp4.pair_weight_planes_dequant(planes, k)
            hi = wg.astype(np.float16)
            t = lambda z: torch.from_numpy(np.asarray(z, np.float64))      # noqa: E731
            return torch.from_numpy(hi).cuda(), torch.from_numpy(planes).cuda(), (t(hi), t(ql), t(qh), t(wg))
        self.w1h, self.w1m, self.w1p = wparts(w1)
        self.w2h, self.w2m, self.w2p = wparts(w2)

    def run(self, full_x, valid, a0, M, reserved0, gmax=0):
        from emotivoice_amd import _ffi
        Cc = 32
        out = torch.full((M + 2 * PAD, Cc), 7.0, device="cuda")
        if self.acc_in:
            out[PAD:PAD + M] = self.acc[a0:a0 + M]
        xp, op = full_x[PAD:].data_ptr(), out[PAD:].data_ptr()
        d = _ffi.ev_res_pair_desc()
        d.x, d.ldx, d.w1, d.b1, d.w2, d.M, d.k, d.dil = xp, Cc, self.w1h.data_ptr(), self.b1.data_ptr(), self.w2h.data_ptr(), M, self.k, self.dil
        d.w1_mx, d.w2_mx, d.gmax = self.w1m.data_ptr(), self.w2m.data_ptr(), gmax
        e = d.epi
        e.bias, e.res, e.res_dtype, e.ldres = self.b2.data_ptr(), xp, 1, Cc
        e.row_valid, e.valid_shift, e.out_scale = valid.data_ptr(), VSHIFT, 1.0 / 3.0
        if self.acc_in:
            e.acc32, e.ldacc = op, Cc               # in place: the engine's running MRF sum
        e.out32, e.ldo = op, Cc
        e.reserved0 = reserved0
        torch.cuda.synchronize()
        assert self.lib.ev_op_resblock_pair_c32_mx(C.byref(d), None) == 0
        torch.cuda.synchronize()
        return out

    def check_groups(self, out, reserved0, max_tiles, bmo):
        L = self.L
        for g0, g1 in L.groups(max_tiles * bmo // PITCH):
            Mg = g1 - g0
            assert -(-Mg // bmo) <= max_tiles
            xg = torch.zeros(Mg + 2 * PAD, 32, device="cuda")
            xg[PAD:PAD + Mg] = self.x[g0:g1]
            vg = L.valid[g0 >> VSHIFT:g1 >> VSHIFT].clone()
            p = self.run(xg, vg, g0, Mg, reserved0)
            assert _same(p[PAD:PAD + Mg], out[PAD + g0:PAD + g1]), (reserved0, g0, g1)
            _zeros_and_slack(p, Mg, L.vrow_d[g0:g1], 7.0)

    def check_tiles(self, out, fmt, tiles, bmo, name):
        """the references of test_fused_mx_resblock_pair per tile, in fp64: the same arithmetic with the host quantiser (5e-5), the exact convs (2e-4)"""
        L, k, dil, M = self.L, self.k, self.dil, self.L.M
        h2 = (k - 1) // 2
        h1 = h2 * dil
        full_c, out_c, acc_c = self.full.cpu(), out[PAD:PAD + M].cpu().double(), self.acc.cpu().double()
        b1, b2 = self.b1.double().cpu(), self.b2.double().cpu()
        parts = _e5_act_parts if fmt == "e5m2" else _mx_act_parts

        def mxconv(a_rows, wp, dd):
            ah, qah, qal, _ = parts(a_rows.float())
            return _conv64(ah, wp[0], dd, k) + _conv64(qah, wp[1], dd, k) + _conv64(qal, wp[2], dd, k)
        worst = {"emu": 0.0, "exact": 0.0}
        for t in tiles:
            m0, m1 = t * bmo, min((t + 1) * bmo, M)
            v = L.vrow[m0:m1]
            if not bool(v.any()):
                continue
            xw = full_c[m0:m1 + 2 * PAD]                # rows [m0 - PAD, m1 + PAD)
            a0 = _lrelu(xw, 0.1)
            vm1 = L.vpad[m0 + h1:m1 + 2 * PAD - h1]     # validity of conv1's output rows [m0 - PAD + h1, m1 + PAD - h1)
            off = PAD - h1 - h2
            for rname, conv in (("emu", lambda a, i, dd: mxconv(a, self.w1p if i == 0 else self.w2p, dd)),
                                ("exact", lambda a, i, dd: _conv64(a.double(), (self.w1p if i == 0 else self.w2p)[3], dd, k))):
                xt = _lrelu(conv(a0, 0, dil) + b1, 0.1)
                xt[~vm1] = 0
                y = conv(xt.float() if rname == "emu" else xt, 1, 1)[off:off + m1 - m0]
                y = (y + b2 + xw[PAD:PAD + m1 - m0].double()) / 3.0
                if self.acc_in:
                    y = y + acc_c[m0:m1]
                r = _rel(out_c[m0:m1][v], y[v])
                worst[rname] = max(worst[rname], r)
                assert r < (5e-5 if rname == "emu" else 2e-4), (name, rname, t, r)
        print("pair-long %s: worst tile of %d  vs emulation %.2e (bound 5e-5)  vs exact %.2e (bound 2e-4)" % (name, len(tiles), worst["emu"], worst["exact"]))


@pytest.mark.parametrize("k,dil,acc_in", [(3, 5, True), (7, 1, False), (11, 5, True)])
def test_pair_c32_mx_long(lib, k, dil, acc_in):
    """The three C = 32 MX pair kernels at 2.5-2.7 iterations per block: the E5M2 kernel (reserved0 = 32; at k = 3 also the launcher's own choice, the same
    bits), the two-group fp4 kernel (16) and the lock-step fp4 kernel (16 | 4), the two fp4 kernels bit-identical.  Worst tile of 12 against the fp64
    references of test_fused_mx_resblock_pair, measured on an MI355X, against the bounds < 5e-5 (host-quantiser emulation) and < 2e-4 (exact convs):
      (3, 5, acc-in)    E5M2 1.18e-06 / 1.47e-05   fp4 two-group 6.10e-07 / 1.98e-05   fp4 lock-step 1.33e-06 / 1.92e-05
      (7, 1, no acc)    E5M2 1.36e-06 / 2.89e-05   fp4 two-group 1.78e-06 / 3.65e-05   fp4 lock-step 1.86e-06 / 3.48e-05
      (11, 5, acc-in)   E5M2 8.05e-07 / 1.42e-05   fp4 two-group 2.10e-06 / 1.90e-05   fp4 lock-step 8.57e-07 / 1.89e-05
    (the two fp4 kernels have different tile heights, so their twelve tiles are different rows; their outputs are the same bits)"""
    n_cu = _n_cu()
    h2 = (k - 1) // 2
    L = _Layout(_big_segments(n_cu))
    M = L.M
    P = _MxPair(lib, L, k, dil, acc_in, 300 + k + dil)
    outs = {}
    # (reserved0, format, rows per tile, tiles per block and iteration)
    for r0, fmt, gr, per in ((32, "e5m2", 128, 2), (16, "fp4", 128, 2), (16 | 4, "fp4", 256, 1)):
        bmo = gr - 2 * h2
        ntiles = -(-M // bmo)
        T = min(-(-ntiles // per), n_cu) * per          # the launchers' grids (launch_resblock_pair_c32_mx)
        assert ntiles > 2 * T, (ntiles, T)              # >= 3 iterations for some blocks, >= 2 for all
        name = "mx C=32 k=%d dil=%d %s %s reserved0=%d" % (k, dil, "acc-in" if acc_in else "no-acc", fmt, r0)
        out = P.run(P.full, L.valid, 0, M, r0)
        _zeros_and_slack(out, M, L.vrow_d, 7.0)          # (acc-in, in place: the invalid rows held the addend and are written as zeros)
        P.check_groups(out, r0, n_cu * per, bmo)
        _, tiles = L.pick_tiles(bmo, T)
        P.check_tiles(out, fmt, tiles, bmo, name)
        outs[r0] = out
    assert _same(outs[16], outs[16 | 4])
    assert not _same(outs[16], outs[32])
    if k == 3:
        assert _same(P.run(P.full, L.valid, 0, M, 0), outs[32])


def test_pair_c32_e5_gmax_below_m(lib):
    """gmax < M on the E5M2 kernel with the in-place accumulate-in: rows [gmax, M) are written as exact zeros, rows below gmax have the bits of a launch with
    M = gmax."""
    n_cu = _n_cu()
    k, dil, bmo = 3, 5, 126
    L = _Layout(_big_segments(n_cu))
    M = L.M
    gmax = (L.S - 2) * PITCH + 504
    assert -(-gmax // bmo) > 4 * n_cu and bool(L.vrow[gmax]) and bool(L.vrow[gmax - 1])
    P = _MxPair(lib, L, k, dil, True, 78)
    P.full[PAD + gmax:] = 0
    out = P.run(P.full, L.valid, 0, M, 32, gmax=gmax)
    xs = torch.zeros(gmax + 2 * PAD, 32, device="cuda")
    xs[PAD:PAD + gmax] = P.x[:gmax]
    p = P.run(xs, L.valid, 0, gmax, 32)
    vr = L.vrow_d.clone()
    vr[gmax:] = False
    _zeros_and_slack(out, M, vr, 7.0)
    assert _same(out[PAD:PAD + gmax], p[PAD:PAD + gmax])
    assert float(out[PAD + gmax - 8:PAD + gmax].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# resblock_pair_c64_mx_kernel<acc>: plane sets in / out, 126 output rows per tile, one tile per block and iteration
@pytest.fixture(scope="module")
def c64_input(lib):
    """the layout, the input plane set (host quantiser) and the weights, shared by the C = 64 MX cases and left unchanged"""
    from emotivoice_amd import mxfp4
    n_cu = _n_cu()
    L = _Layout(_big_segments(n_cu))
    M, Cc, k = L.M, 64, 3
    g = torch.Generator().manual_seed(640)
    x = torch.randn(M + 2 * PAD, Cc, generator=g) * torch.exp(0.5 * torch.randn(M + 2 * PAD, 1, generator=g))
    x[:PAD] = 0
    x[PAD + M:] = 0
    x[PAD:PAD + M][~L.vrow] = 0
    ps_x, _ = _host_plane_set(_lrelu(x, 0.1).float())

    def wset(seed):
        gw = torch.Generator().manual_seed(seed)
        wg = (torch.randn(Cc, k, Cc, generator=gw) / math.sqrt(Cc * k)).numpy()
        hi = wg.astype(np.float16)
        lo16 = ((wg - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
        return torch.from_numpy(hi).cuda(), torch.from_numpy(lo16).cuda(), torch.from_numpy(mxfp4.pack_c64_weight_planes(wg)).cuda()
    b1, b2 = torch.randn(Cc, generator=g).cuda() * 0.1, torch.randn(Cc, generator=g).cuda() * 0.1
    acc = torch.randn(M, Cc, generator=g).cuda()
    return dict(L=L, ps_x=ps_x, w1=wset(1), w2=wset(2), b1=b1, b2=b2, acc=acc)


def _ps_rows(ps_big, g0, g1):
    """rows [g0, g1) of a plane set as a plane set of their own; its slack rows hold the planes of zero rows (the big set's own slack)"""
    Mg = g1 - g0
    ps = _PlaneSet(Mg, ps_big.C)
    pairs = [(ps.h, ps_big.h)] + [(ps.q4[i], ps_big.q4[i]) for i in range(2)] + [(ps.qs[i][0], ps_big.qs[i][0]) for i in range(2)]
    for dst, src in pairs:
        dst[:PAD] = src[:PAD]
        dst[PAD + Mg:] = src[:PAD]
        dst[PAD:PAD + Mg] = src[PAD + g0:PAD + g1]
    return ps


class _C64Mx:
    def __init__(self, lib, inp, dil, mode, slope=0.1, partial=0):
        self.lib, self.inp, self.dil, self.slope, self.partial = lib, inp, dil, slope, partial
        self.want32, self.planes_out, self.acc_in = "o32" in mode, "planes" in mode, mode.startswith("acc")

    def epi_fields(self, e, valid, a0, out, ps_o):
        inp = self.inp
        e.bias, e.row_valid, e.valid_shift, e.out_scale, e.ldo = inp["b2"].data_ptr(), valid.data_ptr(), VSHIFT, 1.0 / 3.0, 64
        e.res_inv_slope = 10.0
        if self.acc_in:
            e.acc32, e.ldacc = inp["acc"][a0:].data_ptr(), 64
        if self.want32:
            e.out32 = out[PAD:].data_ptr()
        if self.planes_out:
            ps_o.out_fields(e, self.slope)
            e.mxo_logC, e.mxo_partial = 6, self.partial

    def fused(self, ps_in, valid, a0, M, twice=False):
        from emotivoice_amd import _ffi
        inp = self.inp
        out, ps_o = torch.full((M + 2 * PAD, 64), 7.0, device="cuda"), _PlaneSet(M, 64)
        dp = _ffi.ev_res_pair_desc()
        dp.x, dp.ldx, dp.w1, dp.b1, dp.w2, dp.M, dp.k, dp.dil = ps_in.h[PAD:].data_ptr(), 64, inp["w1"][0].data_ptr(), inp["b1"].data_ptr(), inp["w2"][0].data_ptr(), M, 3, self.dil
        dp.w1_mx, dp.w2_mx = inp["w1"][2].data_ptr(), inp["w2"][2].data_ptr()
        e = dp.epi
        e.mx_x4[0], e.mx_x4[1] = ps_in.q4[0][PAD:].data_ptr(), ps_in.q4[1][PAD:].data_ptr()
        e.mx_xs[0], e.mx_xs[1], e.mx_xs_stride = ps_in.qs[0][0, PAD:].data_ptr(), ps_in.qs[1][0, PAD:].data_ptr(), ps_in.R * 4
        self.epi_fields(e, valid, a0, out, ps_o)
        for _ in range(2 if twice else 1):
            torch.cuda.synchronize()
            assert self.lib.ev_op_resblock_pair_c64_mx(C.byref(dp), None) == 0
            torch.cuda.synchronize()
        return out, ps_o

    def layerwise(self, ps_in, valid, M):
        """the two ev_op_conv_gemm launches the fused kernel replaces (conv_c64_mx_kernel, covered by test_conv_c64_mx)"""
        from emotivoice_amd import _ffi
        inp = self.inp
        ps_t = _PlaneSet(M, 64)
        ps_t.h.zero_()
        for i in range(2):
            ps_t.q4[i].zero_()
            ps_t.qs[i].fill_(1)                       # (the engine's plane buffers have zero slack rows)
        w1h, w1l, w1m = inp["w1"]
        w2h, w2l, w2m = inp["w2"]
        d1 = _ffi.ev_conv_gemm_desc()
        d1.dtype, d1.W, d1.W_lo, d1.W_mx = 3, w1h.data_ptr(), w1l.data_ptr(), w1m.data_ptr()
        ps_in.in_fields(d1)
        d1.bias, d1.M, d1.N, d1.K, d1.taps, d1.dil, d1.center, d1.out_scale, d1.ldo = inp["b1"].data_ptr(), M, 64, 64, 3, self.dil, 1, 1.0, 64
        d1.row_valid, d1.valid_shift, d1.act, d1.act_slope = valid.data_ptr(), VSHIFT, 3, 0.1
        ps_t.out_fields(d1, 1.0)
        d1.mxo_logC = 6
        _launch(self.lib, d1)
        out, ps_o = torch.full((M + 2 * PAD, 64), 7.0, device="cuda"), _PlaneSet(M, 64)
        d2 = _ffi.ev_conv_gemm_desc()
        d2.dtype, d2.W, d2.W_lo, d2.W_mx = 3, w2h.data_ptr(), w2l.data_ptr(), w2m.data_ptr()
        ps_t.in_fields(d2)
        d2.M, d2.N, d2.K, d2.taps, d2.dil, d2.center = M, 64, 64, 3, 1, 1
        d2.res, d2.res_dtype, d2.ldres = ps_in.h[PAD:].data_ptr(), 3, 64
        d2.res_x4, d2.res_xs, d2.res_xs_stride = ps_in.q4[1][PAD:].data_ptr(), ps_in.qs[1][0, PAD:].data_ptr(), ps_in.R * 4
        self.epi_fields(d2, valid, 0, out, ps_o)
        d2.mxo_partial = 0
        _launch(self.lib, d2)
        return out, ps_o

    def same_outputs(self, a, b, ra, rb, what):
        """rows ra of (out, planes) a == rows rb of b, bit for bit; a partial set: the hi plane, the remainder's codes and scales"""
        (oa, pa), (ob, pb) = a, b
        if self.want32:
            assert _same(oa[ra], ob[rb]), what
        if self.planes_out:
            assert _same(pa.h[ra], pb.h[rb]), what
            for i in ((1,) if self.partial else (0, 1)):
                assert _same(pa.q4[i][ra], pb.q4[i][rb]), (what, i)
                assert _same(pa.qs[i][0, ra, :2], pb.qs[i][0, rb, :2]), (what, i)

    def zeros_and_slack(self, o, M, vrow_d):
        out, ps = o
        if self.want32:
            _zeros_and_slack(out, M, vrow_d, 7.0)
        else:
            assert bool((out == 7.0).all())
        if self.planes_out:
            _zeros_and_slack(ps.h, M, vrow_d, 3.0)
            for i in range(2):
                untouched = self.partial and i == 0          # a partial set leaves the hi codes / hi scales alone
                assert bool((ps.q4[i] == 0x77).all()) if untouched else int(torch.count_nonzero(ps.q4[i][PAD:PAD + M][~vrow_d] & 0x77)) == 0
                assert bool((ps.qs[i] == 130).all()) if untouched else not bool((ps.q4[i][PAD:PAD + M] == 0x77).all())
                assert bool((ps.q4[i][:PAD] == 0x77).all()) and bool((ps.q4[i][PAD + M:] == 0x77).all())
                assert bool((ps.qs[i][0, :PAD] == 130).all()) and bool((ps.qs[i][0, PAD + M:] == 130).all())
        else:
            assert bool((ps.h == 3.0).all())


def _c64_mx_case(lib, inp, dil, mode, slope=0.1, partial=0):
    n_cu = _n_cu()
    L, ps_x = inp["L"], inp["ps_x"]
    M, bmo = L.M, 126                                     # Pair64MxGeom::BMO
    ntiles = -(-M // bmo)
    T = min(ntiles, n_cu)
    assert ntiles > 2 * T, (ntiles, T)
    K = _C64Mx(lib, inp, dil, mode, slope, partial)
    big = K.fused(ps_x, L.valid, 0, M, twice=True)
    K.zeros_and_slack(big, M, L.vrow_d)
    for g0, g1 in L.groups(n_cu * bmo // PITCH):
        Mg = g1 - g0
        assert -(-Mg // bmo) <= n_cu
        vg = L.valid[g0 >> VSHIFT:g1 >> VSHIFT].clone()
        small = K.fused(_ps_rows(ps_x, g0, g1), vg, g0, Mg)
        K.same_outputs(small, big, slice(PAD, PAD + Mg), slice(PAD + g0, PAD + g1), (dil, mode, g0, g1))
        K.zeros_and_slack(small, Mg, L.vrow_d[g0:g1])
    return K, big


@pytest.mark.parametrize("dil,mode", [(1, "planes"), (5, "acc+o32+planes"), (3, "o32")])
def test_pair_c64_mx_long(lib, c64_input, dil, mode):
    """resblock_pair_c64_mx_kernel at 5 tiles per block (1301 tiles on 256 CUs), launched twice: bit for bit the two layer-wise launches it replaces at the
    same M over all rows (the reference of test_fused_mx_resblock_pair_c64: no tolerance), and the single-iteration launches of the same rows."""
    K, big = _c64_mx_case(lib, c64_input, dil, mode)
    L = c64_input["L"]
    ref = K.layerwise(c64_input["ps_x"], L.valid, L.M)
    rows = slice(PAD, PAD + L.M)
    K.same_outputs(big, ref, rows, rows, (dil, mode, "layer-wise"))


def test_pair_c64_mx_partial_out_long(lib, c64_input):
    """The partial plane-set output (mxo_partial) at dil 5 and 5 tiles per block: the hi / remainder planes of the full set at slope 1 (itself bit for bit the
    layer-wise launches), the hi codes / hi scales untouched."""
    L = c64_input["L"]
    Kf, full = _c64_mx_case(lib, c64_input, 5, "planes", slope=1.0)
    Kp, part = _c64_mx_case(lib, c64_input, 5, "planes", slope=1.0, partial=1)
    rows = slice(PAD, PAD + L.M)
    Kp.same_outputs(part, full, rows, rows, "partial vs full")
    Kf.same_outputs(full, Kf.layerwise(c64_input["ps_x"], L.valid, L.M), rows, rows, "full vs layer-wise")
