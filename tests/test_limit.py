"""CPU checks of ev_limit's host half (include/evhip.h) and of its numpy restatement (tests/limit_oracle.py): the smoothing window and the
interpolator's taps against the library's, the meter's known answers, the limiter's properties on the tests' voiced signal, LimiterConfig, the
pre-gain rule, and the serving functions' and the CLI's pass-through."""
import ctypes as C
import math

import numpy as np
import pytest

import limit_oracle as mo
import loudness_oracle as lo

from emotivoice_amd import _ffi

CEILING = float(mo.DEFAULT_CEILING)
CASES = ((0, 0), (16, 0), (5, 37), (80, 800))
GAINS = (1.0, 2.5, 6.0)
WORST_OVERSHOOT, MARGIN = mo.WORST_OVERSHOOT, mo.MARGIN      # tests/limit_oracle.py records how they were measured


@pytest.fixture(scope="module")
def runs():
    """The oracle on the voiced signal (8000 samples, peak 0.5) at every (gain, L, Hd): computed once, read by several tests."""
    x = mo.voiced_half()
    assert x.size == 8000 and np.abs(x).max() == np.float32(0.5)
    return x, {(g, L, Hd): mo.limit(x, g, L=L, Hd=Hd) for g in GAINS for L, Hd in CASES}


def test_window_equals_the_library_and_sums_to_at_most_one():
    from emotivoice_amd.limiter import window
    for L in (0, 1, 2, 80, 1024):
        w = window(L)
        assert w.dtype == np.float32 and w.shape == (L + 1,) and np.array_equal(w.view(np.uint32), mo.window(L).view(np.uint32)), L
        acc = 0.0
        for v in w:
            acc += float(v)
        assert acc <= 1.0 and acc > 1.0 - 1e-6 and (w > 0).all(), (L, acc)
    assert window(0).tolist() == [1.0] and window(1).tolist() == [0.5, 0.5]
    lib = _ffi.lib()
    buf = np.zeros(2000, np.float32)
    for bad in (-1, 1025):
        assert lib.ev_limit_design(bad, buf.ctypes.data_as(C.c_void_p)) == -1 and not buf.any()
        with pytest.raises(ValueError, match="lookahead"):
            window(bad)
    assert lib.ev_limit_design(4, None) == -1


def test_interpolator_is_the_resampler_design_with_up_4():
    """The library's taps match the Python design to one fp32 ulp (as tests/test_resample.py holds every design); each phase has unit DC gain."""
    from emotivoice_amd.limiter import interpolator
    h, want = interpolator(), mo.taps()
    assert h.shape == (129,) and np.array_equal(h, h[::-1])
    assert (np.abs(h.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(h), np.abs(want)))).all()
    for q in range(4):
        assert abs(h.astype(np.float64)[q::4].sum() - 1.0) < 1e-4, q


def test_known_answers_of_the_meter():
    """A sine at fs / 4 with phase pi / 4 and amplitude 0.98 has samples of +-0.693 only; its true peak is 0.98.  Measured on the oracle, over
    the interior (the segment's ends are transients of the zero padding): a relative error of -1.03e-5.  A full-scale 997 Hz sine at 16 kHz:
    +2.6e-6.  Both are held to five times that."""
    n = np.arange(4000)
    x = (0.98 * np.sin(2 * np.pi * n / 4 + np.pi / 4)).astype(np.float32)
    m = mo.meter(x)
    assert abs(float(m["sample_peak"]) - 0.98 * math.sqrt(0.5)) < 1e-6 and m["nonfinite"] == 0
    rel = float(m["p"][100:-100].max()) / 0.98 - 1.0
    print("fs / 4: true peak error %.3g" % rel)
    assert abs(rel) <= 5 * 1.03e-5
    x = lo.sine(997.0, 1.0, 16000)
    rel = float(mo.meter(x)["p"][100:-100].max()) - 1.0
    print("997 Hz: true peak error %.3g" % rel)
    assert abs(rel) <= 5 * 2.6e-6
    # phase 0 of v is the input low-passed at 0.47 fs (the voiced signal's noise floor above it is 0.002), and a non-finite sample enters as zero and is counted
    y = mo.voiced_half(2000)
    m = mo.meter(y)
    assert np.abs(m["v"][0::4] - y).max() < 0.01 and m["true_peak"] >= m["sample_peak"] == np.float32(np.abs(y).max())
    y[[5, 900]] = [np.nan, np.inf]
    m2 = mo.meter(y)
    assert m2["nonfinite"] == 2 and np.isfinite(m2["p"]).all() and np.isfinite(m2["true_peak"])


def test_erosion_and_gain_against_brute_force():
    """The oracle's doubling erosion and its vectorised gain against the definitions written as loops, at windows that are and are not powers of
    two; m before the segment's first sample is below 1 when a peak sits there."""
    rng = np.random.default_rng(0)
    r = rng.uniform(0.2, 1.0, 300).astype(np.float32)
    r[r > 0.6] = 1.0
    r[0] = r[-1] = 0.25
    ext = lambda k: r[k] if 0 <= k < r.size else np.float32(1.0)      # noqa: E731
    for L, Hd in ((0, 0), (1, 0), (3, 0), (5, 37), (2, 300), (7, 8)):
        m = mo.erode(r, L, Hd)
        want = np.array([min(ext(j) for j in range(k - Hd, k + L + 1)) for k in range(-L, r.size)], np.float32)
        assert np.array_equal(m, want), (L, Hd)
        if L:
            assert m[0] == 0.25      # m[-L] covers sample 0
        w = mo.window(L)
        s = mo.gain(m, w, L)
        for n in (0, 1, 150, r.size - 1):
            ms = [m[n - j + L] for j in range(L + 1)]
            acc = 0.0
            for j in range(L + 1):
                acc += float(w[j]) * float(ms[j])
            assert s[n] == (np.float32(1.0) if all(v == 1.0 for v in ms) else np.float32(acc)), (L, Hd, n)
        assert (s <= r).all(), (L, Hd)


def test_limiter_properties_on_the_voiced_signal(runs):
    """s <= r at every sample, the output's sample peak within one rounding of the ceiling, and at gain 1 (peak 0.5, below the ceiling) the
    input's bits."""
    x, res = runs
    for (g, L, Hd), o in res.items():
        assert (o["s"] <= o["r"]).all() and (o["s"] > 0).all(), (g, L, Hd)
        assert float(o["sample_peak_out"]) <= CEILING * (1.0 + 2.0 ** -22), (g, L, Hd, o["sample_peak_out"])
        assert o["min_gain"] == o["s"].min() <= o["r"].min() and o["limited"] == int((o["s"] < 1).sum())
        if g == 1.0:
            assert np.array_equal(o["wav"].view(np.uint32), x.view(np.uint32)) and o["limited"] == 0 and o["min_gain"] == 1.0
        else:
            assert o["limited"] > 0 and float(o["true_peak_in"]) > CEILING
            # the gain is one away from the peaks: more than L + Hd + L samples from any sample that asks for a gain
            far = mo.sliding_min(np.concatenate([np.ones(2 * L + Hd, np.float32), o["r"], np.ones(2 * L + Hd, np.float32)]), 4 * L + 2 * Hd + 1) == 1.0
            assert (o["s"][far] == 1.0).all()
            assert np.array_equal(o["wav"][o["s"] == 1.0].view(np.uint32), o["u"][o["s"] == 1.0].view(np.uint32))


def test_output_true_peak_stays_within_the_margin(runs):
    x, res = runs
    worst = 0.0
    for (g, L, Hd), o in res.items():
        over = float(o["true_peak_out"]) / CEILING - 1.0
        print("gain %.1f L %d Hd %d: true peak out %.6f, overshoot %.3g" % (g, L, Hd, o["true_peak_out"], over))
        if L >= 5:
            worst = max(worst, over)
            assert float(o["true_peak_out"]) <= CEILING * (1.0 + MARGIN), (g, L, Hd, over)
    assert 0.5 * WORST_OVERSHOOT < worst <= 1.02 * WORST_OVERSHOOT, worst      # the recorded figure is the oracle's
    # L = 0, documented: the sample peak holds, the true peak does not
    assert float(res[(2.5, 0, 0)]["true_peak_out"]) > CEILING * 1.03 and float(res[(6.0, 0, 0)]["true_peak_out"]) > CEILING * 1.1


def test_output_rules_of_the_oracle():
    x = np.array([0.5, -1.0, 1.0, 0.2, -0.3, np.nan, np.inf, 3e-5], np.float32)
    o = mo.limit(x, 1.0, ceiling=1.0, L=0, Hd=0)
    assert o["nonfinite"] == 2 and o["sample_peak_in"] == 1.0 and np.isnan(o["wav"][5]) and o["wav_i16"][5] == 0
    assert (np.abs(o["wav"][[0, 1, 2, 3, 4, 7]]) <= 1.0).all() and np.abs(o["wav_i16"].astype(np.int32)).max() <= 32768
    i16 = np.array([-32768, 5, 32767, 0], np.int16)
    o16, of = mo.limit(i16, 2.0, L=2, Hd=3), mo.limit(i16.astype(np.float32) / np.float32(32768.0), 2.0, L=2, Hd=3)
    assert np.array_equal(o16["wav"].view(np.uint32), of["wav"].view(np.uint32)) and o16["sample_peak_in"] == 2.0
    assert o16["wav_i16"].min() >= -32768 and float(o16["sample_peak_out"]) <= CEILING * (1.0 + 2.0 ** -22)


def test_pre_gain_is_the_gain_rule_without_the_peak_step():
    from emotivoice_amd.limiter import pre_gain
    from emotivoice_amd.loudness import FLAG_BOOST_LIMITED, FLAG_PEAK_LIMITED, FLAG_UNDEFINED, LoudnessConfig, gain_for
    seen = set()
    for target in (float("nan"), -70.0, -23.0, -16.0, 0.0):
        for L in (-np.inf, -69.5, -40.0, -23.0, -16.0, -3.01, 2.5):
            for mg in (20.0, 0.0, 6.0):
                cfg = LoudnessConfig(target_lufs=target, max_gain_db=mg)
                g, f = pre_gain(L, cfg)
                wg, wf = gain_for(L, 0.0, cfg)      # a peak of 0 skips step 4
                assert g.dtype == np.float32 and g == wg and f == wf and not f & FLAG_PEAK_LIMITED, (target, L, mg)
                seen.add(f)
    assert seen == {0, FLAG_UNDEFINED, FLAG_BOOST_LIMITED}
    cfg = LoudnessConfig(target_lufs=-16.0)
    assert pre_gain(-46.0, cfg) == (np.float32(10.0), FLAG_BOOST_LIMITED) and gain_for(-46.0, 0.5, cfg)[0] < pre_gain(-46.0, cfg)[0]


def test_default_config_and_python_config_agree():
    from emotivoice_amd.limiter import MAX_HOLD, MAX_LOOKAHEAD, LimiterConfig, as_config
    c = _ffi.ev_limit_config()
    _ffi.lib().ev_default_limit_config(C.byref(c))
    assert (c.struct_size, c.sample_rate, c.ceiling, c.lookahead, c.hold, c.want_i16) == (C.sizeof(c), 16000, np.float32(10 ** (-1 / 20.0)), 80, 800, 0)
    d = LimiterConfig().validate().to_struct()
    assert (d.struct_size, d.sample_rate, d.ceiling, d.lookahead, d.hold, d.want_i16) == (c.struct_size, c.sample_rate, c.ceiling, c.lookahead, c.hold, c.want_i16)
    assert (_ffi.EV_LIMIT_MAX_SAMPLES, _ffi.EV_LIMIT_MAX_LOOKAHEAD, _ffi.EV_LIMIT_MAX_HOLD, _ffi.EV_LIMIT_TILE) == (1 << 30, MAX_LOOKAHEAD, MAX_HOLD, 4096) == (1 << 30, 1024, 8192, 4096)
    assert LimiterConfig(sample_rate=48000).samples() == (240, 2400) and LimiterConfig(sample_rate=22050, lookahead_ms=0.1, hold_ms=1.3).samples() == (2, 29)
    assert LimiterConfig(ceiling_dbtp=0.0).ceiling == 1.0
    for kw, needle in ((dict(sample_rate=11025), "sample_rate"), (dict(sample_rate=16000.5), "sample_rate"), (dict(ceiling_dbtp=0.5), "ceiling"),
                       (dict(ceiling_dbtp=float("nan")), "ceiling"), (dict(ceiling_dbtp=-float("inf")), "ceiling"), (dict(lookahead_ms=-1.0), "lookahead"),
                       (dict(lookahead_ms=64.1), "lookahead"), (dict(lookahead_ms=float("nan")), "lookahead"), (dict(hold_ms=-0.5), "hold"),
                       (dict(hold_ms=513.0), "hold"), (dict(sample_rate=48000, hold_ms=171.0), "hold")):
        with pytest.raises(ValueError, match=needle):
            LimiterConfig(**kw).validate()
    for sr in lo.SAMPLE_RATES:
        LimiterConfig(sample_rate=sr, ceiling_dbtp=0.0, lookahead_ms=0.0, hold_ms=0.0, want_int16=True).validate()
    # the limiter= argument of synthesize / synthesize_long
    a = as_config(True, 16000, want_int16=True)
    assert (a.sample_rate, a.ceiling_dbtp, a.want_int16, a.samples()) == (16000, -1.0, True, (80, 800))
    assert as_config(-2, 16000).ceiling_dbtp == -2.0 and not as_config(-2.0, 16000).want_int16
    given = LimiterConfig(hold_ms=10.0)
    assert as_config(given, 16000).hold_ms == 10.0
    for bad, needle in ((LimiterConfig(sample_rate=48000), "engine's"), (False, "limiter"), ("-1", "limiter"), (1.5, "ceiling")):
        with pytest.raises(ValueError, match=needle):
            as_config(bad, 16000)


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def synthesize(self, utts, **kw):
        self.calls.append(kw)
        n = len(utts)
        out = dict(wav_list=[np.full(4, b, np.float32) for b in range(n)])
        if "flac" in kw:
            out["flac_list"] = [b"fLaC%d" % b if m else None for b, m in enumerate(kw["flac"])]
        return out


def test_serving_synth_functions_pass_the_limiter_through():
    from emotivoice_amd.limiter import LimiterConfig
    from emotivoice_amd.prosody import Prosody
    from emotivoice_amd.serving import engine_flac_synth_fn, engine_prosody_synth_fn, engine_synth_fn
    utts = [dict(), dict()]
    eng = _FakeEngine()
    # without the setting synthesize is called exactly as before
    engine_synth_fn(eng)(utts, 1.25)
    engine_prosody_synth_fn(eng)(utts, [Prosody(), Prosody()])
    engine_flac_synth_fn(eng, loudness=-16.0)(utts, 0.8, [True, False])
    assert [sorted(c) for c in eng.calls] == [["alpha"], ["prosody"], ["alpha", "flac", "loudness"]]
    eng.calls.clear()
    cfg = LimiterConfig(ceiling_dbtp=-2.0)
    assert len(engine_synth_fn(eng, loudness=-16.0, limiter=-1.0)(utts, 1.25)) == 2
    engine_synth_fn(eng, limiter=True)(utts, 1.0)
    engine_prosody_synth_fn(eng, limiter=cfg)(utts, [Prosody(), Prosody()])
    got = engine_flac_synth_fn(eng, loudness=-16.0, limiter=cfg)(utts, [Prosody(), Prosody()], [False, True])
    assert eng.calls[0] == dict(alpha=1.25, loudness=-16.0, limiter=-1.0)
    assert eng.calls[1] == dict(alpha=1.0, limiter=True)
    assert eng.calls[2]["limiter"] is cfg and "loudness" not in eng.calls[2] and "alpha" not in eng.calls[2]
    assert eng.calls[3]["limiter"] is cfg and eng.calls[3]["loudness"] == -16.0 and eng.calls[3]["flac"] == [False, True] and "prosody" in eng.calls[3]
    assert isinstance(got[0], np.ndarray) and got[1] == b"fLaC1"


def test_cli_has_the_true_peak_flag():
    from emotivoice_amd.inference_tts import build_parser
    p = build_parser()
    assert p.parse_args(["-t", "x.txt"]).true_peak is None
    a = p.parse_args(["-t", "x.txt", "--loudness", "-16", "--true-peak", "-1"])
    assert a.true_peak == -1.0 and a.loudness == -16.0
