"""CPU checks of tests/exact_lattice.py: the lattices are what they claim, the budget precondition holds for every case of the GPU parametrisation
(tests/test_gpu_exact.py, imported without touching the GPU), an fp32 accumulation of a case's terms gives the expected bits in any order, and the
comparison flags the defects it exists for."""
import numpy as np
import pytest

import exact_lattice as EL
import test_gpu_exact as G
from emotivoice_amd import mxfp4


def _l1(block, p, density=0.3, shape=(96, 256), seed=3):
    return EL.two_level(np.random.default_rng(seed), shape, block, p, density)


@pytest.mark.parametrize("block,rule,p", [(32, "ocp", -2), (128, "best", -3), (32, "best", -3), (32, "ocp", 1), (128, "best", -6)])
def test_host_quantisers_are_lossless_on_l1(block, rule, p):
    v = _l1(block, p)
    hi, lo = mxfp4.split_hi_lo(v)
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), v.astype(np.float64)) and lo.any()
    a = np.round(np.ldexp(hi.astype(np.float64), -p))
    assert np.array_equal(np.ldexp(a, p), hi) and set(np.unique(np.abs(a))) <= {0.0, 4.0, 6.0}          # the hi part is the first level
    for part in (hi, lo):
        assert np.array_equal(mxfp4.dequantize(*mxfp4.quantize(part, block, rule), block), part)
    assert np.array_equal(mxfp4.e5m2_decode(mxfp4.e5m2_hi_codes(hi)), hi)
    assert np.array_equal(mxfp4.e5m2_lo_decode(mxfp4.e5m2_lo_codes(lo)), lo)
    s = lo * np.float32(2048.0)          # the split-precision kernel's lo operand
    assert np.array_equal(s.astype(np.float16).astype(np.float32), s)


def test_l1_offset_13_is_the_smallest():
    """with offset 12 the fp16 split already fails: 4 - 6 2^-12 rounds into the lower binade"""
    x = np.float32(4.0 - 6.0 * 2.0 ** -12)
    assert mxfp4.split_hi_lo(np.array([x]))[0][0] != 4.0
    assert mxfp4.split_hi_lo(np.array([np.float32(4.0 - 6.0 * 2.0 ** -13)]))[0][0] == 4.0


def test_l0_has_no_lo_parts_and_dense():
    case = [c for c in G.ALL_CASES if c.name == "x3_L0_split64_o32"][0]
    inp = EL.make_inputs(case)
    for v in (inp["x"], inp["w"]):
        assert not mxfp4.split_hi_lo(v)[1].any()
    assert (inp["w"] != 0).mean() > 0.9 and (inp["x"][EL.PAD:-EL.PAD] != 0).mean() > 0.9


def test_mx_value_equals_split_precision_value_on_l1():
    """on L1 the host quantiser is lossless, so what dtype 3 promises is what dtype 2 promises"""
    import dataclasses
    case = [c for c in G.MX_CASES if c.name == "mx_L1_k7_f32in"][0]
    inp = EL.make_inputs(case)
    a = EL.expected(case, inp)["out32"]
    b = EL.expected(dataclasses.replace(case, dtype=2), inp)["out32"]
    assert np.array_equal(a, b)
    hi_only = EL.conv(mxfp4.split_hi_lo(EL.lrelu(inp["x"], np.float32(case.slope)))[0], mxfp4.split_hi_lo(inp["w"])[0], case.taps, case.dil, case.center, np.arange(case.M))
    assert (EL.expected(dataclasses.replace(case, epi=("pro",), mask=0), inp)["out32"] != hi_only.astype(np.float32)).mean() > 0.5          # the cross terms are there


@pytest.mark.parametrize("case", G.ALL_CASES, ids=G._ids(G.ALL_CASES))
def test_budget_holds_for_every_gpu_case(case):
    inp = G.case_inputs(case)
    bits = EL.budget(case, inp)
    assert bits < EL.LIMIT_BITS, (case.name, bits)
    if case.lattice == "L1":
        assert bits > 16, (case.name, bits)          # the two levels are both in play
    live = inp["x"][EL.PAD:EL.PAD + case.M]
    assert not inp["x"][:EL.PAD].any() and not inp["x"][EL.PAD + case.M:].any() and live.any()
    if case.mask:
        assert not live[~inp["vrow"]].any() and inp["vrow"].any() and not inp["vrow"].all()          # masked rows are zero in the input


ORDER_CASES = [c for c in G.ALL_CASES if c.name in ("epi_generic_acc32", "x3_L1_split64_generic", "x3_L1_splitk_s3", "mx_L1_k11_f32in", "f32_256x32_k7")]


@pytest.mark.parametrize("case", ORDER_CASES, ids=G._ids(ORDER_CASES))
def test_fp32_accumulation_is_order_independent(case):
    """the terms of some output elements, accumulated in fp32 in several random orders and chunkings (partial sums added at the end, as split-K and the two
    accumulators of the split precision do): always the bits of the fp64 reference"""
    assert len(ORDER_CASES) == 5
    inp = EL.make_inputs(case)
    rng = np.random.default_rng(11)
    rows = rng.choice(np.nonzero(inp.get("vrow", np.ones(case.M, bool)))[0], 6, replace=False)
    plain = EL.Case(case.name, case.kernel, case.dtype, case.M, case.K, case.N, case.taps, case.dil, lattice=case.lattice, epi=("pro",) if case.has("pro") else ())
    want = EL.expected(plain, inp, rows)["out32"]
    parts = EL.operand_parts(plain, inp)
    for ri, r in enumerate(rows):
        for n in rng.choice(case.N, 4, replace=False):
            terms = np.concatenate([(np.asarray(xp, np.float32)[EL.PAD + r + (t - case.center) * case.dil] * np.asarray(wp, np.float32)[n, t]) for xp, wp in parts
                                    for t in range(case.taps)]).astype(np.float32)
            terms = terms[terms != 0]
            for trial in range(6):
                perm = rng.permutation(terms)
                chunks = np.array_split(perm, [1, 2, 3, 5, 8, 16][trial])
                partial = []
                for ch in chunks:
                    acc = np.float32(0.0)
                    for v in ch:
                        acc = np.float32(acc + v)
                    partial.append(acc)
                acc = np.float32(0.0)
                for v in partial:
                    acc = np.float32(acc + v)
                assert acc == want[ri, n], (case.name, r, n, trial)


def _good():
    case = [c for c in G.ALL_CASES if c.name == "epi_generic_acc32"][0]
    inp = EL.make_inputs(case)
    return case, inp, EL.expected(case, inp)


def test_compare_flags_the_defects_it_exists_for():
    case, inp, want = _good()
    o32, o16, exact = want["out32"], want["out16"], want["exact"]
    assert EL.compare(o32.copy(), o32) == o32.size and EL.compare(o16.copy(), o16) == o16.size
    assert EL.mismatches(-np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32))[0] == 0          # +-0 are equal
    r = int(np.nonzero(inp["vrow"])[0][40])
    # one flipped ulp in one element
    bad = o32.copy()
    bad[r, 5] = np.nextafter(bad[r, 5], np.float32(np.inf))
    n, msg = EL.mismatches(bad, o32)
    assert n == 1 and "(%d, 5)" % r in msg and "rows mod 256" in msg and "columns mod 128" in msg
    with pytest.raises(AssertionError):
        EL.compare(bad, o32, what="ulp")
    # one element taken from the neighbouring row
    bad = o32.copy()
    bad[r, 9] = o32[r + 1, 9]
    assert o32[r, 9] != o32[r + 1, 9] and EL.mismatches(bad, o32)[0] == 1
    # two taps swapped in one column
    w2 = inp["w"].copy()
    w2[17, [0, 2]] = w2[17, [2, 0]]
    n, msg = EL.mismatches(EL.expected(case, inp, w=w2)["out32"], o32)
    assert n > case.M // 4 and "1 columns" in msg
    # a truncated instead of rounded fp16
    trunc = (np.abs(exact).astype(np.float32).view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32).astype(np.float16) * np.sign(exact).astype(np.float16)
    assert EL.mismatches(trunc, o16)[0] > o16.size // 8          # (the lattice does reach below fp16's quantum: the rounding is exercised)
    # non-finite values never pass
    bad = o32.copy()
    bad[3, 3] = np.nan
    assert EL.mismatches(bad, bad)[0] == 1
    # planes: a scale byte off by one; fp4 code 8 is code 0, any other code change is reported
    h16, ch, cl, sh, sl = EL.plane_set(exact, 0.125)
    bad = sh.copy()
    bad[r, 1] += 1
    assert EL.mismatches(bad, sh, "bytes")[0] == 1
    neg0 = np.where((ch & 15) == 0, ch | 8, ch)
    assert (neg0 != ch).any() and EL.mismatches(neg0, ch, "codes")[0] == 0
    bad = ch.copy()
    bad[r, 0] ^= 0x10
    assert EL.mismatches(bad, ch, "codes")[0] == 1


def test_expected_epilogue_order_matches_the_documented_one():
    """a hand evaluation of one element of the full epilogue"""
    case, inp, want = _good()
    r = int(np.nonzero(inp["vrow"])[0][7])
    n = 3
    x = EL.lrelu(inp["x"].astype(np.float64), case.slope)
    v = sum(float(x[EL.PAD + r + (t - case.center) * case.dil] @ inp["w"][n, t].astype(np.float64)) for t in range(case.taps))
    v = ((v + float(inp["bias"][n])) + float(inp["res"][r, n])) * case.scale + float(inp["acc32"][r, n])
    assert want["out32"][r, n] == np.float32(v) and want["out16"][r, n] == np.float16(v if v > 0 else v * case.slope)
    assert not want["out32"][~inp["vrow"]].any() and not want["out16"][~inp["vrow"]].any()


@pytest.mark.parametrize("pc", G.PAIR_CASES, ids=[c[0] for c in G.PAIR_CASES])
def test_budget_holds_for_the_pair_cases(pc):
    """both convs of a fused pair (the GPU test asserts the same on its own row count, which follows the device's CU count; here: an eighth of it), and the
    inputs keep every leaky-relu of the fixed slope 0.1 inactive"""
    p = G.pair_inputs(pc, n_cu=32)
    assert p["x"].min() >= 0 and not p["x"][EL.PAD:-EL.PAD][~p["vrow"]].any() and ((p["w1"] < 0).any() or (p["w2"] < 0).any())
    for fmt in {"f16": ["f16"], "mx32": ["e5m2", "fp4"], "mx64": ["fp4"]}[pc[2]]:
        v32, v16, bits = G.pair_reference(p, fmt, "cpu")
        assert bits < EL.LIMIT_BITS, (pc[0], fmt, bits)
        assert float(v32.abs().max()) > 1.0 and not bool(v32[~G.torch.from_numpy(p["vrow"])].any())
        if fmt == "f16":          # the fp16 store of the intermediate does round: the reference without it differs
            assert float((v16.half().double() != v16).double().mean()) > 0.05
