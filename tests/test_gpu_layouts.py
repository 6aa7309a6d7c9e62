"""MI355X: the generator and the acoustic model at accepted layouts other than the default (tests/layout_cases.py).

ev_create accepts a family of layouts and make_voc_plan turns one into a schedule through a dozen layout-dependent decisions; every other GPU
test runs EVShapes().  Here each listed layout, chosen for the planner arm it reaches, produces waveforms that are held to a float64 CPU
reference, shows by its launch records that the arm was taken, and keeps the project's same-bits claims.

Bounds (none of them taken from what the device gives):
  strict  TOL_STRICT on every waveform and every stage tap: a rounding-class bound, and no listed layout is deeper than the default it was set for
  fast    m * fp16_level(layout, mel), m = FAST_ZDC / fp16_level(default, the 37-frame mel): the margin the project grants its fp16 mode over its
          measured level, carried to the level a CPU emulation of fp16 weights / operands / storage predicts for this layout and mel
  mx      fp16_level(layout, mel) with no margin (every mx data path is the fp16 hi x hi product plus correction terms, stored finer than fp16);
          TOL_MX too on the default layout
Every figure goes to layouts_report.json, next to the other GPU files' reports, before it is asserted.
"""
import numpy as np
import pytest

import layout_cases as L

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

REPORT = {}
PRECS = ("strict", "mx", "fast")


def _report(key, val):
    """into layouts_report.json, next to the other GPU files' reports (test_gpu_parity keeps the report directory)"""
    from test_gpu_parity import _report as write_report
    write_report(key, val, "layouts_report.json", REPORT)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


class _Guarded:
    """an engine whose HIP errors end the session: once a device call has failed nothing more is started on that GPU"""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if not callable(attr):
            return attr

        def call(*a, **kw):
            from emotivoice_amd.engine import EVError
            try:
                return attr(*a, **kw)
            except EVError as e:
                if " failed: " in str(e) and "hip" in str(e).lower():          # HIPCHK's message: "<call> failed: <hipGetErrorString> (file:line)"
                    pytest.exit("device error, nothing more is run: %s" % e, returncode=3)
                raise
        return call


class _Engines:
    """the engines of one layout: one per (precision, switches), made on first use, closed when the layout's tests end"""

    def __init__(self, case):
        self.case, self.engines, self.outs = case, {}, {}

    def get(self, prec, **kw):
        from emotivoice_amd.engine import EVEngine
        key = (prec,) + tuple(sorted(kw.items()))
        if key not in self.engines:
            assert L.accepted(self.case.shapes) == "ok"
            eng = _Guarded(EVEngine(shapes=self.case.shapes, precision=prec, **kw))          # (ev_create agrees with accepted(), or this raises)
            eng.load_blob(self.case.blob, self.case.manifest_json)
            self.engines[key] = eng
        return self.engines[key]

    def ragged(self, prec):
        """the three short mels as one ragged batch on the precision's plain engine (shared by the tests of that precision)"""
        if prec not in self.outs:
            self.outs[prec] = self.get(prec).vocoder(self.case.mels[:3], want_int16=True)
        return self.outs[prec]

    def close(self):
        for e in self.engines.values():
            e.close()
        self.engines, self.outs = {}, {}


@pytest.fixture(scope="module", params=list(L.LAYOUTS))
def case(request, gpu):
    return L.build_case(request.param)


@pytest.fixture(scope="module")
def engines(case):
    e = _Engines(case)
    yield e
    e.close()


_DEFAULT = {}


def _default_case():
    if "case" not in _DEFAULT:
        _DEFAULT["case"] = L.build_case("default")
    return _DEFAULT["case"]


def _margin(case):
    """m: FAST_ZDC over the emulated fp16 level of the default layout on the 37-frame mel"""
    if "m" not in _DEFAULT:
        c = case if case.name == "default" else _default_case()
        _DEFAULT["m"] = L.FAST_ZDC / c.fp16_levels()[2]
    return _DEFAULT["m"]


# ---------------------------------------------------------------------------------------------------------------- waveforms against the reference
@pytest.mark.parametrize("prec", PRECS)
def test_waveforms_against_float64_reference(case, engines, prec):
    out = engines.ragged(prec)
    up = case.shapes.upsample_factor
    assert [len(w) for w in out["wav_list"]] == [n * up for n in L.MEL_LENS] and out["wav"].shape[0] == sum(L.MEL_LENS) * up
    errs = [dict(wav=L.rel_l2(w, r), wav_ac=L.rel_l2_ac(w, r)) for w, r in zip(out["wav_list"], case.refs)]
    levels, m = case.fp16_levels(), _margin(case)
    bound = {"strict": [L.TOL_STRICT] * 3, "mx": levels[:3], "fast": [m * v for v in levels[:3]]}[prec]
    rep = dict(errs=errs, fp16_level=levels[:3], m=m, bound=bound, frames=list(L.MEL_LENS))
    if prec == "mx":
        rep["above_half_fp16_level"] = [n for n, e, v in zip(L.MEL_LENS, errs, levels) if e["wav_ac"] > 0.5 * v]      # reported, not asserted
    _report("wave/%s/%s" % (case.name, prec), rep)
    print("wave", case.name, prec, rep)
    for n, e, b in zip(L.MEL_LENS, errs, bound):
        assert np.isfinite(e["wav_ac"]) and e["wav"] <= b and e["wav_ac"] <= b, (case.name, prec, "%d frames" % n, e, "bound %.3e" % b)
        if prec == "mx" and case.name == "default":
            assert e["wav_ac"] <= L.TOL_MX, (n, e)


# ---------------------------------------------------------------------------------------------------------------- stage taps (keep_stages: a second data flow)
@pytest.mark.parametrize("prec", ("strict", "mx"))
def test_stage_taps_against_float64_reference(case, engines, prec):
    """keep_stages changes the plan (no partial-plane MRF, no streams, no grouping, fp32 copies beside the planes): the 37-frame mel alone, every
    generator tap against the float64 oracle's.  strict: TOL_STRICT per tap; mx: the waveform rule on the last tap and on the waveform."""
    n_up = len(case.shapes.up_rates)
    taps = {}
    L.oracle64(case.sd, case.mels[2], case.shapes, taps)
    eng = engines.get(prec, keep_stages=True)
    out = eng.vocoder([case.mels[2]])
    names = ["voc_pre"] + [t % i for i in range(n_up) for t in ("voc_up%d", "voc_mrf%d")]
    errs = {}
    for name in names:
        r = taps[name].numpy().T          # the oracle keeps (C, L), the engine is channels-last
        errs[name] = L.rel_l2(eng.get_stage(name).reshape(r.shape), r)
    errs["wav"], errs["wav_ac"] = L.rel_l2(out["wav"], case.refs[2]), L.rel_l2_ac(out["wav"], case.refs[2])
    level = case.fp16_levels()[2]
    _report("taps/%s/%s" % (case.name, prec), dict(errs=errs, fp16_level=level))
    print("taps", case.name, prec, errs)
    if prec == "strict":
        for name, e in errs.items():
            assert e <= L.TOL_STRICT, (case.name, name, errs)
    else:
        last = "voc_mrf%d" % (n_up - 1)
        assert all(np.isfinite(e) for e in errs.values()), errs
        assert errs[last] <= level and errs["wav_ac"] <= level and errs["wav"] <= level, (case.name, last, errs, level)


# ---------------------------------------------------------------------------------------------------------------- the arm was taken
def _match(r, pat):
    return all((r[k] in v) if isinstance(v, (tuple, set, frozenset)) else r[k] == v for k, v in pat.items())


def has(recs, **pat):
    return any(_match(r, pat) for r in recs)


def count(recs, **pat):
    return sum(_match(r, pat) for r in recs)


def first(recs, **pat):
    return next((i for i, r in enumerate(recs) if _match(r, pat)), len(recs))


GM, C64, P64, P32, X3 = "voc_conv_gemm_mx", "voc_conv_c64_mx", "voc_resblock_pair_c64_mx", "voc_resblock_pair_c32_mx", "voc_conv_gemm_x3"
F16, F64, F32 = "voc_conv_gemm_f16", "voc_resblock_pair_c64", "voc_resblock_pair_c32"
RB64 = dict(N=64, K=64)
# name -> precision -> (what the launch records of one profiled call on the ragged batch must show).  Written from make_voc_plan; a profiled call
# takes no streams, so a layout with the kernel set {3, 7, 11} issues its >= 128-channel MX stages as grouped levels (one record per level: the three
# convs' taps summed, 21, and dil = 0).  Every layout but the default must show something the default's records do not (asserted below).
ARMS = {
    "default": {
        "mx": [("grouped levels at stages 0-1", lambda r: count(r, name=GM, taps=21, dil=0) == 10),
               ("k = 3 first at C = 64: fused pair, then conv_c64_mx", lambda r: count(r, name=P64, taps=3) == 3 and first(r, name=P64) < first(r, name=C64, taps=11)),
               ("the last up-conv on conv_c64_mx", lambda r: has(r, name=C64, taps=3, dil=1, **RB64)),
               ("every C = 32 pair fused", lambda r: count(r, name=P32) == 9),
               ("only conv_pre on the split kernel", lambda r: all(x["K"] == 96 for x in r if x["name"] == X3))],
        "fast": [("fused pairs at C = 32 and at C = 64, k = 3", lambda r: count(r, name=F32) == 9 and count(r, name=F64) == 3)],
    },
    "perm": {
        "mx": [("k = 3 is the second ResBlock at C = 64: its fused pair runs after the k = 11 convs (fp32 accumulate-in)",
                lambda r: count(r, name=P64, taps=3) == 3 and first(r, name=C64, taps=11, **RB64) < first(r, name=P64) < first(r, name=C64, taps=7)),
               ("stages 0-1 still grouped", lambda r: count(r, name=GM, taps=21, dil=0) == 10)],
        "fast": [("k = 3 pair at C = 64 after the k = 11 layers", lambda r: first(r, name=F16, taps=11, **RB64) < first(r, name=F64) < first(r, name=F16, taps=7, **RB64))],
    },
    "wide": {
        "mx": [("C = 64, k = 3, dil = 9 on conv_c64_mx, not the fused pair", lambda r: count(r, name=C64, taps=3, dil=9) == 1 and not has(r, name=P64, dil=9) and count(r, name=P64) == 2),
               ("C = 32, k = 11, dil = 6 falls out of the fused pair (70 > 64)", lambda r: has(r, name=X3, N=32, taps=11, dil=6) and not has(r, name=P32, taps=11, dil=6)),
               ("C = 32, k = 7, dil = 9 stays fused (60)", lambda r: has(r, name=P32, taps=7, dil=9) and count(r, name=P32) == 8),
               ("k = 7, dil = 9 inside the grouped levels' span", lambda r: count(r, name=GM, taps=21, dil=0) == 10)],
        "fast": [("C = 64, k = 3, dil = 9 layer by layer: the fused pair's slab holds dil <= 8", lambda r: not has(r, name=F64, dil=9) and has(r, name=F16, taps=3, dil=9, **RB64) and count(r, name=F64) == 2),
                 ("C = 32, k = 11, dil = 6 fused (384-row slab)", lambda r: has(r, name=F32, taps=11, dil=6) and count(r, name=F32) == 9)],
    },
    "two": {
        "mx": [("n_rb = 2: no grouped level, one launch per conv", lambda r: not has(r, name=GM, dil=0) and count(r, name=GM, N=256, K=256, taps=11) == 6),
               ("no 7-tap conv but conv_pre", lambda r: all(x["K"] == 96 for x in r if x["taps"] == 7)),
               ("fused pairs", lambda r: count(r, name=P64) == 3 and count(r, name=P32) == 6)],
        "fast": [("two ResBlocks of pairs", lambda r: count(r, name=F32) == 6 and count(r, name=F64) == 3 and not has(r, name=F64, taps=11))],
    },
    "one4": {
        "mx": [("four dilations of k = 7 on the MX kernels", lambda r: has(r, name=GM, N=256, taps=7, dil=8) and has(r, name=C64, taps=7, dil=8) and count(r, name=C64, taps=7) == 8),
               ("no fused C = 64 pair, four fused C = 32 pairs", lambda r: count(r, name=P64) == 0 and count(r, name=P32) == 4 and has(r, name=P32, taps=7, dil=8)),
               ("no grouped level", lambda r: not has(r, name=GM, dil=0))],
        "fast": [("four k = 7 pairs at C = 32, none at C = 64", lambda r: count(r, name=F32, taps=7) == 4 and count(r, name=F64) == 0 and has(r, name=F16, taps=7, dil=8, **RB64))],
    },
    "odd": {
        "mx": [("no MX launch at 5 or 9 taps", lambda r: not has(r, name=(GM, C64), taps=(5, 9))),
               ("up0 through the scratch is the only conv_gemm_mx launch; no MX stage", lambda r: count(r, name=GM) == 1 and has(r, name=GM, N=2048, K=512) and count(r, name=(C64, P64)) == 0),
               ("C = 32, k = 3 still fused beside split-kernel layers", lambda r: count(r, name=P32) == 2 and has(r, name=X3, N=32, taps=9, dil=3) and has(r, name=X3, N=32, taps=5, dil=2))],
        "fast": [("k = 5 / 9 layer by layer, k = 3 fused", lambda r: has(r, name=F16, taps=5, dil=2) and has(r, name=F16, taps=9, dil=3) and count(r, name=F32) == 2 and count(r, name=F64) == 2)],
    },
    "s4": {
        "mx": [("polyphase up-convs at s = 4 on conv_gemm_mx", lambda r: has(r, name=GM, N=1024, K=512, taps=3) and has(r, name=GM, N=512, K=256, taps=3) and has(r, name=GM, N=256, K=128, taps=3)),
               ("the last up-conv (N = 128, K = 64) has no planes: split kernel, not conv_c64_mx", lambda r: has(r, name=X3, N=128, K=64, taps=3) and not has(r, name=C64, taps=3)),
               ("C = 64 stage still MX", lambda r: count(r, name=P64) == 3 and count(r, name=C64, taps=(7, 11)) == 12)],
        "fast": [("up-convs at s = 4", lambda r: has(r, name=F16, N=128, K=64, taps=3) and has(r, name=F16, N=1024, K=512, taps=3))],
    },
    "up3": {
        "mx": [("three stages from 256 channels", lambda r: not has(r, K=512) and has(r, name=GM, N=1024, K=256, taps=3) and has(r, name=GM, N=256, K=128, taps=3)),
               ("one grouped stage only", lambda r: count(r, name=GM, taps=21, dil=0) == 5),
               ("C = 64 at stage 1, its next up-conv (N = 128, K = 64) on the split kernel", lambda r: count(r, name=P64) == 3 and has(r, name=X3, N=128, K=64, taps=3) and count(r, name=P32) == 9)],
        "fast": [("three stages", lambda r: not has(r, K=512) and has(r, name=F16, N=1024, K=256, taps=3) and count(r, name=F32) == 9)],
    },
    "up1": {
        "mx": [("no MX launch but the C = 32 pairs", lambda r: {x["name"] for x in r if x["name"].endswith("_mx")} == {P32} and count(r, name=P32) == 9),
               ("conv_pre to 64 channels, one up-conv at s = 16", lambda r: has(r, name=X3, N=64, K=96, taps=7) and has(r, name=X3, N=512, K=64, taps=3) and count(r, name=X3) == 2)],
        "fast": [("one stage", lambda r: count(r, name=F16) == 2 and has(r, name=F16, N=512, K=64, taps=3) and count(r, name=F32) == 9 and count(r, name=F64) == 0)],
    },
}


def _profiled(eng, mels):
    eng.set_profiling(True)
    try:
        out = eng.vocoder(mels)
        return out, eng.launch_records()
    finally:
        eng.set_profiling(False)


def _default_records(prec):
    if ("recs", prec) not in _DEFAULT:
        from emotivoice_amd.engine import EVEngine
        c = _default_case()
        eng = EVEngine(shapes=c.shapes, precision=prec)
        eng.load_blob(c.blob, c.manifest_json)
        _DEFAULT["recs", prec] = _profiled(eng, c.mels[:3])[1]
        eng.close()
    return _DEFAULT["recs", prec]


@pytest.mark.parametrize("prec", ("mx", "fast"))
def test_the_arm_was_taken(case, engines, prec):
    out, recs = _profiled(engines.get(prec), case.mels[:3])
    if case.name == "default":
        _DEFAULT["recs", prec] = recs
    names = sorted({r["name"] for r in recs})
    shown = {text: bool(pred(recs)) for text, pred in ARMS[case.name][prec]}
    _report("arms/%s/%s" % (case.name, prec), dict(kernels=names, shown=shown,
                                                   launches=["%s N%d K%d t%d d%d" % (r["name"], r["N"], r["K"], r["taps"], r["dil"]) for r in recs if r["name"].startswith("voc_")]))
    print("arms", case.name, prec, shown)
    assert all(shown.values()), (case.name, prec, shown)
    assert np.array_equal(out["wav"], engines.ragged(prec)["wav"]), "the profiled call's bits differ"      # (no streams, grouped levels: the same bits)
    if case.name != "default":
        ref = _default_records(prec)
        novel = [text for text, pred in ARMS[case.name][prec] if not pred(ref)]
        assert novel, (case.name, prec, "every expectation also holds on the default layout's records")


# ---------------------------------------------------------------------------------------------------------------- the same bits
@pytest.mark.parametrize("prec", ("mx", "fast"))
def test_same_bits_small_batch(case, engines, prec):
    from oracle.jets_oracle import wav_to_int16
    eng, batch = engines.get(prec), engines.ragged(prec)
    assert np.array_equal(batch["wav_i16"], wav_to_int16(batch["wav"]))
    for b, mel in enumerate(case.mels[:3]):
        solo = eng.vocoder([mel])
        assert np.array_equal(solo["wav"], batch["wav_list"][b]), (case.name, prec, "alone vs in the ragged batch", L.MEL_LENS[b])
    one = engines.get(prec, vocoder_streams=1).vocoder(case.mels[:3])
    assert np.array_equal(one["wav"], batch["wav"]), (case.name, prec, "vocoder_streams = 1")


@pytest.mark.parametrize("prec", ("mx", "fast"))
def test_same_bits_large_batch(case, engines, prec):
    """the 230-frame mel alone (256 frame rows: the small-batch, stream-eligible path) and nine copies in one call (2304 rows > 2048: grouped levels
    where the kernel set is {3, 7, 11}, else ResBlock after ResBlock)"""
    eng, mel = engines.get(prec), case.mels[3]
    up = case.shapes.upsample_factor
    solo = eng.vocoder([mel])["wav"]
    big = eng.vocoder([mel] * L.BIG_COPIES)
    assert solo.shape[0] == L.BIG_LEN * up and [len(w) for w in big["wav_list"]] == [L.BIG_LEN * up] * L.BIG_COPIES
    e = dict(wav=L.rel_l2(solo, case.refs[3]), wav_ac=L.rel_l2_ac(solo, case.refs[3]))
    for b, w in enumerate(big["wav_list"]):
        assert np.array_equal(w, solo), (case.name, prec, "copy %d of the large batch vs alone" % b)
    assert np.array_equal(engines.get(prec, vocoder_streams=1).vocoder([mel])["wav"], solo), (case.name, prec, "vocoder_streams = 1")
    ng = engines.get(prec, mx_group=False).vocoder([mel] * L.BIG_COPIES)
    assert np.array_equal(ng["wav"], big["wav"]), (case.name, prec, "mx_group = False")
    # the long waveform against the reference, by the rule of the ragged batch at this mel's own emulated level
    level = case.fp16_level_big()
    bound = level * (_margin(case) if prec == "fast" else 1.0)
    _report("big/%s/%s" % (case.name, prec), dict(e, fp16_level=level, bound=bound))
    assert e["wav_ac"] <= bound and e["wav"] <= bound, (case.name, prec, e, bound)


# ---------------------------------------------------------------------------------------------------------------- acoustic-model layouts
DUR = np.array([0, 3, 0, 0, 7, 1, 2, 0, 5, 4, 0, 0, 0, 6, 2, 2, 1, 0, 9, 3], np.int64)      # test_forced_durations_and_zero_duration_guard's


@pytest.fixture(scope="module", params=list(L.AM_LAYOUTS))
def am_case(request, gpu):
    from oracle import am_forward, synth_inputs
    c = L.build_case(request.param)
    c.utt = synth_inputs(51, [20], [9], shapes=c.shapes)[0]
    with torch.no_grad():
        c.am_ref = am_forward(c.sd, torch.from_numpy(c.utt["ling"]), 9, torch.from_numpy(c.utt["style"]), torch.from_numpy(c.utt["content"]), c.shapes,
                              durations=torch.from_numpy(DUR))
    return c


@pytest.fixture(scope="module")
def am_engines(am_case):
    e = _Engines(am_case)
    yield e
    e.close()


@pytest.mark.parametrize("prec", PRECS)
def test_am_layout_mel(am_case, am_engines, prec):
    eng = am_engines.get(prec)
    eng.set_profiling(True)
    try:
        out = eng.synthesize([am_case.utt], forced_durations=DUR, vocoder=False)
        recs = eng.launch_records()
    finally:
        eng.set_profiling(False)
    ref = am_case.am_ref["dec_outputs"].numpy()
    assert out["mel"].shape == (int(DUR.sum()), 64) == ref.shape and int(out["mel_lens"][0]) == int(am_case.am_ref["mel_len"])
    err = L.rel_l2(out["mel"], ref)
    ffn = sorted({(r["name"], r["N"], r["K"], r["taps"]) for r in recs if r["taps"] == am_case.shapes.ffn_kernel})
    _report("am/%s/%s" % (am_case.name, prec), dict(mel=err, ffn_launches=["%s N%d K%d t%d" % x for x in ffn]))
    print("am", am_case.name, prec, err, ffn)
    assert err <= {"strict": L.TOL_STRICT, "mx": L.TOL_MX, "fast": L.TOL_OUT}[prec], (am_case.name, prec, err)
    assert np.array_equal(eng.synthesize([am_case.utt], forced_durations=DUR, vocoder=False)["mel"], out["mel"]), "the profiled call's bits differ"
    if prec == "mx":
        k = am_case.shapes.ffn_kernel
        mx_ffn = [r for r in recs if r["name"] == "dec_mx_gemm" and r["taps"] > 1]
        if am_case.name == "ffn5":          # a 5-tap conv-FFN has no planes: the split kernel, while QKV / output projections stay on the one-tap MX GEMM
            assert not mx_ffn and has(recs, name="dec_f32_gemm", N=1536, K=384, taps=5) and has(recs, name="dec_f32_gemm", N=384, K=1536, taps=5)
            assert has(recs, name="dec_mx_gemm", taps=1)
        else:
            assert len(mx_ffn) == 2 * am_case.shapes.dec_layers and has(mx_ffn, N=1536, K=384, taps=k) and has(mx_ffn, N=384, K=1536, taps=k)
    assert count(recs, name="enc_f32_gemm", N=384, K=1536, taps=am_case.shapes.ffn_kernel) == am_case.shapes.enc_layers


def test_am_layout_full_synthesis_mx(am_case, am_engines):
    """the whole path at n_mels = 64 (to_mel and voc.pre zero-padded to MEL_PAD): waveform against jets_forward under the mx waveform rule"""
    from oracle import jets_forward
    ref = jets_forward(am_case.sd, am_case.utt["ling"], 9, am_case.utt["style"], am_case.utt["content"], am_case.shapes, durations=torch.from_numpy(DUR))
    mel = ref["dec_outputs"].t().contiguous()
    level = L.fp16_level(am_case.sd, mel, am_case.shapes)
    out = am_engines.get("mx").synthesize([am_case.utt], forced_durations=DUR)
    want = ref["wav_predictions"].numpy()
    assert out["wav"].shape == want.shape == (int(DUR.sum()) * 256,)
    e = dict(mel=L.rel_l2(out["mel"], ref["dec_outputs"].numpy()), wav=L.rel_l2(out["wav"], want), wav_ac=L.rel_l2_ac(out["wav"], want), fp16_level=level)
    _report("am_full/%s/mx" % am_case.name, e)
    print("am_full", am_case.name, e)
    assert e["mel"] <= L.TOL_MX and e["wav"] <= level and e["wav_ac"] <= level, e


# ---------------------------------------------------------------------------------------------------------------- rejections
@pytest.mark.parametrize("name", list(L.NEAR_MISSES))
def test_near_misses_are_refused_by_ev_create(gpu, name):
    from emotivoice_amd.engine import EVEngine, EVError
    reason = L.accepted(L.NEAR_MISSES[name])
    assert reason != "ok"
    with pytest.raises(EVError) as ei:
        EVEngine(shapes=L.NEAR_MISSES[name])
    assert reason in str(ei.value), (reason, str(ei.value))
