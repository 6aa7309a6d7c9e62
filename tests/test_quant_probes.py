"""The probe set of tests/quant_probes.py on the CPU: mxfp4.py equals the independent reference on every probe, every deliberately wrong rule is caught by a
named probe (the probes discriminate), every (plane, threshold, side, sign) and pin mantissa is covered, every probe is inside the stated domain, and the
probes the fused C = 32 pairs can carry exactly (tests/test_gpu_quant_edges.py) still cover every threshold."""
import numpy as np
import pytest

import quant_probes as QP
from emotivoice_amd import mxfp4

B = QP.BLOCKS


def _unpack(packed):
    c = np.empty(packed.shape[:-1] + (packed.shape[-1] * 2,), np.uint8)
    c[..., 0::2] = packed & 15
    c[..., 1::2] = packed >> 4
    return c


def _host(blocks):
    """what mxfp4.py states for [n][32] fp32 blocks: every plane of the MX set and both E5M2 operands"""
    hi, lo = mxfp4.split_hi_lo(blocks)
    ch, sh = mxfp4.quantize(hi, 32, rule="ocp")
    cl, sl = mxfp4.quantize(lo, 32, rule="ocp")
    return dict(hi=hi, lo=lo, codes_hi=QP.fold_fp4(_unpack(ch)), scale_hi=sh[:, 0], codes_lo=QP.fold_fp4(_unpack(cl)), scale_lo=sl[:, 0],
                e5_hi=mxfp4.e5m2_hi_codes(hi), e5_lo=QP.fold_e5(mxfp4.e5m2_lo_codes(lo)))


def test_probes_are_inside_the_domain():
    assert QP.in_domain(B) and QP.in_domain(QP.E5_V) and QP.in_domain(QP.E5_HI.astype(np.float64))
    assert B.dtype == np.float32 and QP.E5_V.dtype == np.float32 and QP.E5_HI.dtype == np.float16
    assert not QP.in_domain(np.float32(65520.0)) and not QP.in_domain(np.float32(2.0 ** -101)) and not QP.in_domain(np.float32(np.inf))


def test_mxfp4_equals_the_independent_reference_on_every_probe():
    got = _host(B)
    rh, rl = QP.ref_split(B)
    assert np.array_equal(got["hi"].astype(np.float64), rh) and np.array_equal(np.signbit(got["hi"]), np.signbit(rh))
    assert np.array_equal(got["lo"].astype(np.float64), rl)
    for name, part in (("hi", rh), ("lo", rl)):
        codes, sb = QP.ref_quantize(part)
        assert np.array_equal(got["scale_" + name], sb), name
        bad = np.argwhere(got["codes_" + name] != QP.fold_fp4(codes))
        assert len(bad) == 0, (name, QP.describe(*bad[0]))
    assert np.array_equal(got["e5_hi"], QP.ref_e5m2_trunc(rh))
    assert np.array_equal(got["e5_lo"], QP.fold_e5(QP.ref_e5m2_lo(rl)))
    # the E5M2 probe lists
    assert np.array_equal(mxfp4.e5m2_hi_codes(QP.E5_HI), QP.ref_e5m2_trunc(QP.E5_HI.astype(np.float64)))
    vh, vl = QP.ref_split(QP.E5_V)
    h, lo = mxfp4.split_hi_lo(QP.E5_V)
    assert np.array_equal(h.astype(np.float64), vh) and np.array_equal(lo.astype(np.float64), vl)
    bad = np.flatnonzero(QP.fold_e5(mxfp4.e5m2_lo_codes(lo)) != QP.fold_e5(QP.ref_e5m2_lo(vl)))
    assert len(bad) == 0, [(float(QP.E5_V[i]), QP.E5_TAG[i]) for i in bad[:4]]
    assert np.array_equal(mxfp4.e5m2_hi_codes(h), QP.ref_e5m2_trunc(vh))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# mutants: deliberately wrong rules.  Each must disagree with mxfp4.py on at least one probe.
def _mutant_quantize(part, swap=None, exp_off=-2, nosat=False, group=32):
    """the OCP rule of mxfp4.quantize on [n][32] with one thing wrong -> (codes [n][32], folded; scale byte of the block's first element)"""
    p = np.ascontiguousarray(part, np.float32)
    n = p.shape[0]
    amax = np.repeat(np.abs(p).reshape(n, 32 // group, group).max(-1), group, axis=1)
    bits = np.ascontiguousarray(amax).view(np.uint32)
    e = ((bits >> 23) & 0xFF).astype(np.int32) + exp_off
    if nosat:
        e = e + ((bits >> 22) & 1).astype(np.int32)          # mantissa >= 1.5: the next scale up, nothing saturates
    e = np.clip(e, 1, 254)
    a = np.abs(p * np.ldexp(np.float32(1.0), 127 - e).astype(np.float32))
    c = np.zeros(p.shape, np.uint8)
    for i, t in enumerate(QP.THRESHOLDS):
        strict = (i % 2 == 0) != (swap == i)
        c += (a > np.float32(t)) if strict else (a >= np.float32(t))
    return QP.fold_fp4(c | (np.signbit(p).astype(np.uint8) << 3)), e[:, 0].astype(np.uint8)


def _planes(hi, lo, **kw):
    ch, sh = _mutant_quantize(hi, **kw)
    cl, sl = _mutant_quantize(lo, **kw)
    return dict(codes_hi=ch, scale_hi=sh, codes_lo=cl, scale_lo=sl)


def _trunc_split(v):
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    h = np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float32)
    return h, v - h


def _e5_lo_no_subnormals(lo):
    """mxfp4.e5m2_lo_codes without the clip at the smallest normal binade"""
    y = lo.astype(np.float64) * 2048.0
    a = np.abs(y)
    e = np.minimum(np.floor(np.log2(np.maximum(a, 1e-300))), 15)
    q = np.ldexp(1.0, (e - 2).astype(np.int64))
    r = np.minimum(np.rint(a / q) * q, 57344.0)
    return QP.fold_e5((np.where(np.signbit(y), -r, r).astype(np.float16).view(np.uint16) >> 8).astype(np.uint8))


def _mutants():
    hi, lo = mxfp4.split_hi_lo(B)
    m = {}
    for i, t in enumerate(QP.THRESHOLDS):
        m["threshold %g: > and >= swapped" % t] = lambda i=i: _planes(hi, lo, swap=i)
    m["scale exponent - 1"] = lambda: _planes(hi, lo, exp_off=-1)
    m["no-saturation scale rule"] = lambda: _planes(hi, lo, nosat=True)
    m["maximum over 8 elements"] = lambda: _planes(hi, lo, group=8)
    m["fp16 split by truncation"] = lambda: dict(zip(("hi", "lo"), _trunc_split(B)))
    m["E5M2 hi by rounding"] = lambda: dict(e5_hi=QP.ref_e5m2_nearest(hi.astype(np.float64)))
    m["E5M2 lo by truncation"] = lambda: dict(e5_lo=QP.fold_e5(QP.ref_e5m2_trunc(lo.astype(np.float64) * 2048.0)))
    m["E5M2 lo without the subnormal band"] = lambda: dict(e5_lo=_e5_lo_no_subnormals(lo))
    return m


MUTANTS = _mutants()


def test_the_unmutated_restatement_is_the_host_rule():
    """the mutants change ONE thing of a rule that is otherwise mxfp4.py's"""
    want = _host(B)
    hi, lo = mxfp4.split_hi_lo(B)
    for k, v in _planes(hi, lo).items():
        assert np.array_equal(v, want[k]), k


@pytest.mark.parametrize("name", list(MUTANTS), ids=[n.replace(" ", "_") for n in MUTANTS])
def test_every_mutant_is_caught_by_a_named_probe(name):
    want = _host(B)
    caught = []
    for key, got in MUTANTS[name]().items():
        bad = np.argwhere(np.asarray(got) != want[key])
        if len(bad):
            where = QP.describe(*bad[0]) if bad.shape[1] == 2 else QP.describe(bad[0][0])
            caught.append("%s: %d probes differ, first %s" % (key, len(bad), where))
    print(name, "->", "; ".join(caught))
    assert caught, "mutant '%s' agrees with mxfp4.py on every probe" % name


def test_e5m2_probe_lists_catch_their_mutants():
    """the E5_HI / E5_V lists (what the E5M2 pair kernel is fed) on their own"""
    assert (QP.ref_e5m2_nearest(QP.E5_HI.astype(np.float64)) != mxfp4.e5m2_hi_codes(QP.E5_HI)).any()
    _, lo = mxfp4.split_hi_lo(QP.E5_V)
    want = QP.fold_e5(mxfp4.e5m2_lo_codes(lo))
    assert (QP.fold_e5(QP.ref_e5m2_trunc(lo.astype(np.float64) * 2048.0)) != want).any()
    assert (_e5_lo_no_subnormals(lo) != want).any()
    for band in range(len(QP.E5_BANDS)):
        assert any(t[0] == band for t in QP.E5_TAG), QP.E5_BANDS[band]
    for band in range(5):          # every tie of a band with both neighbours and both remainder signs
        for tie in range(4):
            for side in (-1, 0, 1):
                for sign in (1, -1):
                    assert (band, tie, side, sign) in QP.E5_TAG, (QP.E5_BANDS[band], tie, side, sign)
    # the low byte of the hi parts: truncation against rounding
    low = QP.E5_HI.view(np.uint16) & 0xff
    assert set(low.tolist()) == {0x00, 0x7f, 0x80, 0xff}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# coverage
def _plane_values():
    rh, rl = QP.ref_split(B)
    return {0: rh, 1: rl}


def test_every_threshold_side_sign_and_pin_is_covered_and_means_what_its_tag_says():
    parts = _plane_values()
    for plane in (0, 1):
        sel = QP.PLANE == plane
        p = parts[plane]
        codes, sb = QP.ref_quantize(p)
        y = np.abs(p) / np.ldexp(1.0, sb.astype(np.int64) - 127)[:, None]
        mag = codes & 7
        for t in range(7):
            for side in (-1, 0, 1):
                for neg in (False, True):
                    hit = sel[:, None] & (QP.THR == t) & (QP.SIDE == side) & (np.signbit(p) == neg)
                    assert hit.any(), (plane, QP.THRESHOLDS[t], side, neg)
                    thr = QP.THRESHOLDS[t]
                    yy = y[hit]
                    assert np.all(yy == thr if side == 0 else (yy < thr if side < 0 else yy > thr)), (plane, thr, side)
                    lower, upper = t, t + 1
                    want = (lower if lower % 2 == 0 else upper) if side == 0 else (lower if side < 0 else upper)
                    assert np.all(mag[hit] == want), (plane, thr, side, want)
        sat = sel[:, None] & (QP.THR == QP.SAT)
        assert sat.any() and np.all((y[sat] >= 6) & (y[sat] < 8) & (mag[sat] == 7)) and (y[sat] > 6).any()
        for pi in range(len(QP.PIN_NAMES)):
            blocks = np.flatnonzero(sel & (QP.PIN == pi))
            assert len(blocks), (plane, QP.PIN_NAMES[pi])
            for b in blocks:          # the pin IS the block maximum of its plane, with the mantissa its name says
                a = np.abs(p[b])
                assert a[QP.PINPOS[b]] == a.max(), QP.describe(b)
                m = np.frexp(a.max())[0] * 2
                want = (1.0, None, None, 1.5, 1.75, None)[pi]
                assert (m == want) if want else {1: 1 < m < 1.01, 2: 1.49 < m < 1.5, 5: 1.99 < m < 2}[pi], (QP.describe(b), m)
        assert set(QP.PINPOS[sel].tolist()) >= {0, 7, 8, 31}
    assert "all zero" in QP.KIND and "only -pin" in QP.KIND and "split" in QP.KIND


def test_lo_plane_probes_split_as_intended():
    """every lo-plane probe is an fp32 number (asserted when the module builds it) whose fp16 hi part is the block's one H (or zero), the remainder strictly
    inside half an ulp: no probe of a code threshold depends on how the split breaks a tie"""
    rh, rl = QP.ref_split(B)
    for b in np.flatnonzero(QP.PLANE == 1):
        nz = B[b] != 0
        H = np.unique(np.abs(rh[b][nz]))
        assert len(H) == 1, QP.describe(b)
        if H[0] == 0:
            assert np.all(np.abs(B[b]) < 2.0 ** -25)
        else:
            q = np.ldexp(1.0, max(int(np.frexp(H[0])[1]) - 1, -14) - 10)
            assert np.all(np.abs(rl[b]) < q / 2), QP.describe(b)
        assert np.array_equal(B[b].astype(np.float16).astype(np.float64), rh[b])
    for b in np.flatnonzero(QP.PLANE == 0):
        assert not rl[b].any(), QP.describe(b)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the fused C = 32 pairs (tests/test_gpu_quant_edges.py): what their routes can carry exactly, and what they can see
@pytest.mark.parametrize("fmt", ["fp4", "e5m2"])
@pytest.mark.parametrize("route", QP.PAIR_ROUTES)
def test_pair_routes_keep_every_threshold(fmt, route):
    """a probe whose expected out32 is not an fp32 number at every step is dropped (a condition on the input, not a tolerance): at most a quarter of the
    probe blocks per site may lose an element, and every threshold of the plane(s) a route reads must keep an on-tie probe that is compared AND whose
    expected value changes when its code goes to the other neighbour"""
    s = QP.pair_survival(fmt, route)
    print(fmt, route, {k: v for k, v in s.items() if k != "thresholds"})
    assert 4 * s["dropped_blocks"] <= s["blocks"], s
    reads_hi, reads_lo = route != "input_lo", route != "input_hi"
    for key, n in s["thresholds"].items():
        is_hi = key[0] == (0 if fmt == "fp4" else "hi")
        if (is_hi and reads_hi) or (not is_hi and reads_lo):
            assert n > 0, (fmt, route, key)
    assert len(s["thresholds"]) == (14 if fmt == "fp4" else 24)


def test_pair_routing_weights_are_exact_in_the_weight_planes():
    """the identity at the centre tap with weights 1 + 2^-13, 1.0 and -1.0: hi part and remainder exact under W_RULE"""
    for k in (3, 7):
        for val in (1.0 + 2.0 ** -13, 1.0, -1.0):
            w = QP.pair_identity(k, val)
            hi, lo = mxfp4.split_hi_lo(w)
            ql, qh = mxfp4.pair_weight_planes_dequant(mxfp4.pack_pair_weight_planes(w), k)
            assert np.array_equal(ql, lo) and np.array_equal(qh, hi), (k, val)
            assert hi[5, (k - 1) // 2, 5] == np.float32(round(val)) and lo[5, (k - 1) // 2, 5] == np.float32(val - round(val))
