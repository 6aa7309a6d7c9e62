"""The grouped three-conv MX launch at its edges (MI355X): conv_gemm_mx_group3_kernel through ev_op_conv_gemm_group3.

The kernel's whole contract is "the results are those of the three launches, bit for bit", so the oracle is the same three descriptors issued one by one through
ev_op_conv_gemm (conv_gemm_mx_kernel, held to the fp64 references by test_gpu_ops.py), each into its own sentinel-filled plane set.  Every output plane of every
problem is compared over its WHOLE allocation (fp16 hi plane, both code planes, both scale planes, slack rows included): the same valid rows, the same zeros on
invalid rows, no byte outside the tensor touched, each problem's result in its own plane set.  What is specific to the grouped path and chosen here:

  * tile counts = (M / 256) (N / 128) for the padding of every problem to a multiple of eight blocks and the XCD remap that runs on the padded count for the
    k = 11 and k = 7 problems and on the unpadded one for k = 3: 1, 7, 8, 9, 17 tiles at C = 128 and 6, 8, 10 at C = 256 (two column tiles per row block) --
    fewer than one round of XCDs, exact multiples (no padding blocks), residues 1 / 2 / 6 / 7, more than two rounds;
  * both epilogue forms the launcher accepts (conv1 of a pair: planes only; conv2 inside a ResBlock: residual from a plane set, planes only);
  * one input (and residual) plane set for all three problems, and three of their own;
  * all six orders of the tap counts {3, 7, 11} in the descriptor array;
  * the engine's dilations (conv1 1 / 3 / 5, conv2 1) and triples whose members differ, k = 11 at dil 5 (span 50 of 64) among them;
  * row masks (valid_shift 2 / 3) with invalid first and last rows, invalid runs across 256-row tile boundaries, an all-gap tile, and launches that are all gap;
  * three grouped launches into fresh outputs: the same bits;
  * two small cases against the fp64 evaluation of the MX arithmetic (the reference and bound of test_mx_residual_from_planes), so that a single and a grouped
    launch cannot be wrong in the same way unnoticed;
  * everything the launcher must refuse (-1, nothing launched) and what the entry point itself refuses (-2)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_ops import (PAD, _PlaneSet, _conv64, _host_plane_set, _launch, _lrelu, _mx_act_parts, _mx_weights, _rel, lib)      # noqa: E402, F401  (lib: the library fixture)

SENT_H, SENT_Q4, SENT_QS = 3.0, 0x77, 130          # what _PlaneSet fills its planes with


def _mask(M, vshift, j, allgap=False):
    """row validity of problem variant j -> [M] bool (cpu), constant over groups of 2^vshift rows: the first and last 8 (j + 1) rows invalid; one tile: an
    interior run; three tiles and more: an invalid run from 40 rows before an all-gap tile to 24 rows after it (both tile boundaries crossed), seven and more:
    a second run across the boundary of tiles 5 | 6"""
    v = torch.ones(M, dtype=torch.bool)
    mt = M // 256
    v[:8 * (j + 1)] = False
    v[M - 8 * (j + 1):] = False
    if mt < 3:
        v[96 + 8 * j:136 + 8 * j] = False
    else:
        g = 1 + j % (mt - 2)
        v[g * 256 - 40:(g + 1) * 256 + 24] = False
        assert not bool(v[g * 256:(g + 1) * 256].any()) and bool(v[(g - 1) * 256:g * 256].any()) and bool(v[(g + 1) * 256:(g + 2) * 256].any())
    if mt >= 7:
        v[6 * 256 - 16:6 * 256 + 8] = False
    if allgap:
        v[:] = False
    grp = v.view(-1, 1 << vshift)
    assert bool((grp == grp[:, :1]).all())
    return v


class _Store:
    """inputs shared by the cases and left unchanged: weights per (N, K, k), plane sets per (kind, C, M, vshift, j), row masks"""

    def __init__(self):
        self.w, self.x, self.m = {}, {}, {}

    def weights(self, N, K, k):
        key = (N, K, k)
        if key not in self.w:
            g = torch.Generator().manual_seed(1000 * N + 10 * K + k)
            w = torch.randn(N, K, k, generator=g) / math.sqrt(K * k)
            bias = (torch.randn(N, generator=g) * 0.1).cuda()
            self.w[key] = (_mx_weights(w), bias)
        return self.w[key]

    def mask(self, M, vshift, j, allgap=False):
        """-> (row_valid bytes on the device, [M] bool on the cpu)"""
        key = (M, vshift, j, allgap)
        if key not in self.m:
            v = _mask(M, vshift, j, allgap)
            self.m[key] = (v.view(-1, 1 << vshift)[:, 0].to(torch.uint8).cuda(), v)
        return self.m[key]

    def planes(self, kind, Cc, M, vshift, j):
        """kind "x": the plane set of an activation (a conv's operand); "res": of lrelu(x, 0.1) (the residual a conv2 adds back).  Random rows with widely differing
        row scales, the engine's invariants: zero slack rows, exact zeros in the invalid rows of mask j.  -> (_PlaneSet, (hi, Q(hi), Q(lo)) in fp64)"""
        key = (kind, Cc, M, vshift, j)
        if key not in self.x:
            g = torch.Generator().manual_seed(7 * Cc + M + 131 * j + (5 if kind == "res" else 0) + vshift)
            R = M + 2 * PAD
            a = torch.randn(R, Cc, generator=g) * torch.exp(0.5 * torch.randn(R, 1, generator=g))
            a[:PAD] = 0
            a[PAD + M:] = 0
            a[PAD:PAD + M][~_mask(M, vshift, j)] = 0
            self.x[key] = _host_plane_set(_lrelu(a, 0.1).float() if kind == "res" else a)
        return self.x[key]


@pytest.fixture(scope="module")
def store(lib):
    return _Store()


def _fill(d, form, W, k, dil, M, N, K, x, res, out, valid, vshift):
    """one member of a triple: form "conv1" = planes in, only planes out (EPI_MXP); "conv2" = + the residual from a plane set, out_scale 1 / 3
    (EPI_RESPL | EPI_LEAN | EPI_MXP)"""
    wts, bias = W
    d.dtype, d.W, d.W_lo, d.W_mx = 3, wts["hi"].data_ptr(), wts["lo"].data_ptr(), wts["mx"].data_ptr()
    x.in_fields(d)
    d.bias, d.M, d.N, d.K, d.taps, d.dil, d.center = bias.data_ptr(), M, N, K, k, dil, (k - 1) // 2
    d.row_valid, d.valid_shift = valid.data_ptr(), vshift
    d.out_scale, d.ldo = 1.0, N
    if form == "conv2":
        d.res, d.res_dtype, d.ldres = res.h[PAD:].data_ptr(), 3, N
        d.res_x4, d.res_xs, d.res_xs_stride, d.res_inv_slope = res.q4[1][PAD:].data_ptr(), res.qs[1][0, PAD:].data_ptr(), res.R * 4, 10.0
        d.out_scale = 1.0 / 3.0
    out.out_fields(d, 0.1)


def _planes_of(ps):
    return [ps.h.view(torch.int16), ps.q4[0], ps.q4[1], ps.qs[0], ps.qs[1]]


def _same_set(a, b):
    """every plane of two plane sets over the whole allocation, bit for bit -> the names of the planes that differ"""
    return [n for n, p, q in zip(("h", "q4[0]", "q4[1]", "qs[0]", "qs[1]"), _planes_of(a), _planes_of(b)) if not torch.equal(p, q)]


def _untouched(ps, rows=None):
    """the sentinels of a _PlaneSet in `rows` (default: everywhere)"""
    r = slice(None) if rows is None else rows
    return bool((ps.h[r] == SENT_H).all()) and all(bool((ps.q4[i][r] == SENT_Q4).all()) and bool((ps.qs[i][:, r] == SENT_QS).all()) for i in range(2))


def _group(lib, arr, check_only=0):
    torch.cuda.synchronize()
    rc = lib.ev_op_conv_gemm_group3(arr, check_only, None)
    torch.cuda.synchronize()
    return rc


class _Triple:
    """three problems in descriptor order `order` (tap counts), member i at dilation dils[order[i]]"""

    def __init__(self, store, form, Cc, mt, share, order, dils, vshift, allgap=False):
        from emotivoice_amd import _ffi
        self.ffi, self.form, self.C, self.M, self.order, self.dils, self.vshift, self.allgap = _ffi, form, Cc, 256 * mt, order, dils, vshift, allgap
        M = self.M
        self.members = []
        for i, k in enumerate(order):
            j = 0 if share else i
            valid, vrow = store.mask(M, vshift, j, allgap)
            x, xparts = store.planes("x", Cc, M, vshift, j)
            res, rparts = store.planes("res", Cc, M, vshift, j) if form == "conv2" else (None, None)
            self.members.append(dict(k=k, dil=dils[k], W=store.weights(Cc, Cc, k), x=x, xparts=xparts, res=res, rparts=rparts, valid=valid, vrow=vrow))

    def fill(self, d, i, out):
        m = self.members[i]
        _fill(d, self.form, m["W"], m["k"], m["dil"], self.M, self.C, self.C, m["x"], m["res"], out, m["valid"], self.vshift)

    def singles(self, lib):
        outs = [_PlaneSet(self.M, self.C) for _ in range(3)]
        for i in range(3):
            d = self.ffi.ev_conv_gemm_desc()
            self.fill(d, i, outs[i])
            _launch(lib, d)
        return outs

    def grouped(self, lib):
        outs = [_PlaneSet(self.M, self.C) for _ in range(3)]
        arr = (self.ffi.ev_conv_gemm_desc * 3)()
        for i in range(3):
            self.fill(arr[i], i, outs[i])
        assert _group(lib, arr, 1) == 0
        assert all(_untouched(o) for o in outs), "check_only wrote"
        assert _group(lib, arr, 0) == 0
        return outs

    def check(self, lib):
        """grouped == single launches on every plane, three grouped launches agree, zeros / sentinels where they belong, not vacuous -> the grouped outputs"""
        M, name = self.M, (self.form, self.C, self.M, self.order, self.dils)
        runs = [self.grouped(lib) for _ in range(3)]
        ref = self.singles(lib)
        for r, outs in enumerate(runs):
            for i in range(3):
                assert _same_set(outs[i], ref[i]) == [], (name, "grouped run %d vs single launch, problem %d (k = %d)" % (r, i, self.order[i]))
        got = runs[0]
        for i, o in enumerate(got):
            vrow = self.members[i]["vrow"].cuda()
            body = slice(PAD, PAD + M)
            assert _untouched(o, slice(0, PAD)) and _untouched(o, slice(PAD + M, None)), (name, i, "slack rows")
            assert int(torch.count_nonzero(o.h[body][~vrow])) == 0 and all(int(torch.count_nonzero(o.q4[q][body][~vrow])) == 0 for q in range(2)), (name, i, "gap rows")
            assert not any(bool((o.q4[q][body] == SENT_Q4).all(dim=1).any()) for q in range(2)), (name, i, "a row of a code plane still holds the sentinel")
            if self.allgap:
                assert not bool(o.h[body].any())
            else:
                assert bool((o.h[body][vrow] != SENT_H).any(dim=1).all()), (name, i, "a valid row still holds the sentinel")
                assert float(o.h[body][vrow].float().abs().max()) > 0.1
        if not self.allgap:
            for a, b in ((0, 1), (0, 2), (1, 2)):
                assert not torch.equal(got[a].h, got[b].h), (name, "problems %d and %d have the same hi plane" % (a, b))
        return got

    def fp64_rel(self, i, out):
        """problem i: hi + dequantize(q4[1], qs[1]) of the output planes against lrelu(fp64 xh.wh + Q(xh).Q(wl) + Q(xl).Q(wh) + bias [+ residual, / 3], 0.1) --
        test_mx_residual_from_planes' planes-only comparison"""
        from emotivoice_amd import mxfp4
        m, M, Cc = self.members[i], self.M, self.C
        k, dil = m["k"], m["dil"]
        wts, bias = m["W"]
        th, tqh, tql = m["xparts"]
        h = dil * (k - 1) // 2
        rows = slice(PAD - h, PAD + M + h)
        ref = _conv64(th[rows], wts["wh"], dil, k) + _conv64(tqh[rows], wts["qwl"], dil, k) + _conv64(tql[rows], wts["qwh"], dil, k) + bias.double().cpu()
        if self.form == "conv2":
            xh, _, xql = m["rparts"]
            a_rec = xh + xql                                              # what the epilogue adds back: hi + Q4(lo), then the inverse leaky-relu
            ref = (ref + torch.where(a_rec >= 0, a_rec, a_rec * 10.0)[PAD:PAD + M]) / 3.0
        ref[~m["vrow"]] = 0
        sb = out.qs[1][:, PAD:PAD + M].permute(1, 0, 2).reshape(M, Cc // 32)
        lo_rec = mxfp4.dequantize(out.q4[1][PAD:PAD + M].cpu().numpy(), np.ascontiguousarray(sb.cpu().numpy()), 32)
        rec = out.h[PAD:PAD + M].float().cpu().double() + torch.from_numpy(lo_rec).double()
        return _rel(rec, _lrelu(ref, 0.1))


ORDERS = [(3, 7, 11), (3, 11, 7), (7, 3, 11), (7, 11, 3), (11, 3, 7), (11, 7, 3)]

# (form, C, M / 256, one shared input set, descriptor order, conv1 dilation, valid_shift): tiles = M / 256 at C = 128, 2 M / 256 at C = 256
ENGINE_CASES = [
    ("conv1", 128, 1, True, ORDERS[0], 1, 2), ("conv2", 128, 1, False, ORDERS[5], 1, 3),
    ("conv1", 128, 7, False, ORDERS[2], 3, 3), ("conv2", 128, 7, True, ORDERS[1], 1, 2),
    ("conv1", 128, 8, True, ORDERS[4], 5, 2), ("conv2", 128, 8, False, ORDERS[3], 1, 3),
    ("conv1", 128, 9, False, ORDERS[1], 1, 3), ("conv2", 128, 9, True, ORDERS[5], 1, 2),
    ("conv1", 128, 17, True, ORDERS[3], 3, 2), ("conv2", 128, 17, False, ORDERS[0], 1, 3),
    ("conv1", 256, 3, False, ORDERS[4], 5, 3), ("conv2", 256, 3, True, ORDERS[2], 1, 2),
    ("conv1", 256, 4, True, ORDERS[2], 1, 2), ("conv2", 256, 4, False, ORDERS[4], 1, 3),
    ("conv1", 256, 5, False, ORDERS[5], 3, 3), ("conv2", 256, 5, True, ORDERS[1], 1, 2),
]
assert {c[4] for c in ENGINE_CASES} == set(ORDERS)


def _id(c):
    return "%s-C%d-mt%d-%s-%s" % (c[0], c[1], c[2], "shared" if c[3] else "own", "".join(str(k) for k in c[4]))


@pytest.mark.parametrize("case", ENGINE_CASES, ids=[_id(c) for c in ENGINE_CASES])
def test_group3_equals_single_launches_engine_dilations(lib, store, case):
    """The engine's combinations: one dilation for the three conv1 of a level (1, 3 or 5), conv2 at 1; 1 / 7 / 8 / 9 / 17 tiles at C = 128 and 6 / 8 / 10 at C = 256;
    every one of the six descriptor orders; shared and separate input sets (separate ones carry masks of their own)."""
    form, Cc, mt, share, order, dil1, vshift = case
    assert form == "conv1" or dil1 == 1
    dil = dil1
    _Triple(store, form, Cc, mt, share, order, {3: dil, 7: dil, 11: dil}, vshift).check(lib)


MIXED_CASES = [
    ("conv1", 128, 9, False, ORDERS[3], {11: 5, 7: 3, 3: 1}, 3),
    ("conv2", 128, 7, True, ORDERS[4], {11: 5, 7: 1, 3: 3}, 2),
    ("conv1", 256, 5, True, ORDERS[0], {11: 1, 7: 5, 3: 5}, 2),
]


@pytest.mark.parametrize("case", MIXED_CASES, ids=[_id(c) for c in MIXED_CASES])
def test_group3_equals_single_launches_mixed_dilations(lib, store, case):
    """Members at different dilations (every tile takes the dilation of its own problem), k = 11 at dil 5 = span 50 of the 64 allowed."""
    form, Cc, mt, share, order, dils, vshift = case
    _Triple(store, form, Cc, mt, share, order, dils, vshift).check(lib)


ALLGAP_CASES = [("conv1", 128, 9, True, ORDERS[2], {11: 5, 7: 3, 3: 1}, 3), ("conv2", 256, 3, False, ORDERS[5], {11: 1, 7: 1, 3: 1}, 2)]


@pytest.mark.parametrize("case", ALLGAP_CASES, ids=[_id(c) for c in ALLGAP_CASES])
def test_group3_all_gap_launch(lib, store, case):
    """Every tile of the launch is gap (row_valid all zero over non-zero inputs): all-zero hi and code planes, the single launches' planes bit for bit.  (The
    non-vacuity assertions of the other cases have no valid row to look at here; that every row was written shows in the zeros over the sentinels.)"""
    form, Cc, mt, share, order, dils, vshift = case
    _Triple(store, form, Cc, mt, share, order, dils, vshift, allgap=True).check(lib)


@pytest.mark.parametrize("form", ["conv1", "conv2"])
def test_group3_against_fp64(lib, store, form):
    """C = 128, M = 768: the grouped launch's own output planes against the fp64 evaluation of the MX arithmetic with the host quantiser, the epilogue and the
    consumer's leaky-relu, at the planes-only bound of test_mx_residual_from_planes (1e-4: the fp4 step of the remainder plane).  Measured on an MI355X
    (problems in descriptor order k = 11, 3, 7 at dil 5, 3, 1):
      conv1   2.99e-05  3.01e-05  2.93e-05
      conv2   3.02e-05  2.96e-05  3.00e-05"""
    t = _Triple(store, form, 128, 3, False, ORDERS[4], {11: 5, 7: 1, 3: 3}, 3)
    got = t.check(lib)
    rels = [t.fp64_rel(i, got[i]) for i in range(3)]
    print("group3 %s vs fp64: k = %s  rel %s (bound 1e-4)" % (form, t.order, " ".join("%.2e" % r for r in rels)))
    assert max(rels) < 1e-4, (form, rels)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# what the launcher refuses (-1: "not such a triple", the caller launches one by one) and what the entry point refuses (-2)
REJECTS = ["same_taps", "other_M", "other_N", "other_K", "fp32_A", "out32_one", "out32_all", "acc32_one", "acc32_all", "mixed_forms", "reserved0"]


def _reject_triple(lib, store, what):
    """-> (descriptor array, output plane sets, [(tensor, sentinel)] that must stay as they are, objects to keep alive).  Every member is a descriptor
    ev_op_conv_gemm takes; the triple is not one the grouped kernel takes."""
    from emotivoice_amd import _ffi
    Cc, vshift = 128, 3
    Mbuf = 512 if what == "other_M" else 256
    forms = ["conv2"] * 3 if what in ("acc32_one", "acc32_all") else (["conv1", "conv2", "conv2"] if what == "mixed_forms" else ["conv1"] * 3)
    taps = [3, 3, 11] if what == "same_taps" else [3, 7, 11]
    valid, _ = store.mask(Mbuf, vshift, 0)
    x, _ = store.planes("x", Cc, Mbuf, vshift, 0)
    res, _ = store.planes("res", Cc, Mbuf, vshift, 0)
    arr = (_ffi.ev_conv_gemm_desc * 3)()
    outs, extra, keep = [], [], []
    for i in range(3):
        M, N, K, xi = Mbuf, Cc, Cc, x
        if i == 1 and what == "other_N":
            N = 256
        if i == 1 and what == "other_K":
            K = 256
            xi, _ = store.planes("x", 256, Mbuf, vshift, 0)
        if i == 2 and what == "other_M":
            M = 256
        out = _PlaneSet(Mbuf, N)
        outs.append(out)
        _fill(arr[i], forms[i], store.weights(N, K, taps[i]), taps[i], 1, M, N, K, xi, res, out, valid, vshift)
    if what == "fp32_A":          # member 0 reads an fp32 activation through mx_planes_kernel's scratch instead of a plane set
        xf = torch.randn(Mbuf + 2 * PAD, Cc, device="cuda")
        nb = lib.ev_op_mx_scratch_bytes(Mbuf, Cc)
        scratch = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        d = arr[0]
        d.A, d.lda = xf[PAD:].data_ptr(), Cc
        d.mx_x4[0], d.mx_x4[1], d.mx_xs[0], d.mx_xs[1], d.mx_xs_stride = None, None, None, None, 0
        d.mx_scratch, d.mx_scratch_size = scratch.data_ptr(), nb
        extra.append((scratch, 0))
        keep.append(xf)
    for i in {"out32_one": [2], "out32_all": [0, 1, 2]}.get(what, []):
        o32 = torch.full((Mbuf, Cc), 7.0, device="cuda")
        arr[i].out32 = o32.data_ptr()
        extra.append((o32, 7.0))
    for i in {"acc32_one": [1], "acc32_all": [0, 1, 2]}.get(what, []):
        acc = torch.randn(Mbuf, Cc, device="cuda")
        arr[i].acc32, arr[i].ldacc = acc.data_ptr(), Cc
        keep.append(acc)
    if what == "reserved0":
        arr[0].reserved0 = 1
    return arr, outs, extra, keep


@pytest.mark.parametrize("what", REJECTS)
def test_group3_refuses_what_is_not_a_triple(lib, store, what):
    """-1 with check_only 1 and with check_only 0, and after the latter every output still holds its sentinels: two members with one tap count; a member
    with another M / N / K; an fp32 A + scratch instead of a plane set; out32 beside the planes (one member: forms differ; all three: a form the grouped kernel
    is not built for); acc32 (likewise); one conv1 with two conv2; reserved0 != 0."""
    arr, outs, extra, keep = _reject_triple(lib, store, what)
    for check_only in (1, 0):
        assert _group(lib, arr, check_only) == -1, (what, check_only)
        assert all(_untouched(o) for o in outs), (what, check_only)
        assert all(bool((t == s).all()) for t, s in extra), (what, check_only)
    # (that -1 is the triple's fault, not a member's: every member alone is a launch ev_op_conv_gemm takes)
    for i in range(3):
        _launch(lib, arr[i])
        assert not _untouched(outs[i], slice(PAD, PAD + arr[i].M))


def test_group3_refuses_a_member_the_single_launch_refuses(lib, store):
    """-2 (not -1) for a member ev_op_conv_gemm itself refuses -- M not a multiple of the row alignment (256) -- in either mode, nothing written."""
    t = _Triple(store, "conv1", 128, 1, True, ORDERS[0], {3: 1, 7: 1, 11: 1}, 3)
    outs = [_PlaneSet(t.M, t.C) for _ in range(3)]
    arr = (t.ffi.ev_conv_gemm_desc * 3)()
    for i in range(3):
        t.fill(arr[i], i, outs[i])
    arr[1].M = 128
    torch.cuda.synchronize()
    assert lib.ev_op_conv_gemm(C.byref(arr[1]), None) == -2
    for check_only in (1, 0):
        assert _group(lib, arr, check_only) == -2
        assert all(_untouched(o) for o in outs)
    arr[1].M = t.M          # the same array with the member mended is a triple again
    assert _group(lib, arr, 1) == 0 and all(_untouched(o) for o in outs)
