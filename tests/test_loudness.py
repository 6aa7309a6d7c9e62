"""CPU checks of ev_loudness's host half (include/evhip.h): the K-weighting design against the standard's table and against the oracle, the 997 Hz
known answer of the float64 restatement (tests/loudness_oracle.py), the gain rule, LoudnessConfig, and the serving synth functions' pass-through."""
import ctypes as C
import math

import numpy as np
import pytest

import loudness_oracle as lo

from emotivoice_amd import _ffi


def test_design_reproduces_the_standard_at_48_khz():
    c = lo.design(48000)
    got = np.concatenate([c[0:5], c[8:10]])
    assert np.abs(got - np.array(lo.STANDARD_48K)).max() < 1e-12
    assert c[5:8].tolist() == [1.0, -2.0, 1.0]


def test_the_library_design_equals_the_oracle_at_every_rate():
    lib = _ffi.lib()
    co = (C.c_double * 10)()
    for sr in lo.SAMPLE_RATES:
        assert lib.ev_loudness_design(sr, co) == 0, sr
        got, want = np.array(list(co)), lo.design(sr)
        assert np.abs(got / want - 1.0).max() < 1e-12, (sr, got, want)
    for sr in (0, -16000, 11025, 15999, 96000):
        assert lib.ev_loudness_design(sr, co) == -1, sr
    from emotivoice_amd.loudness import k_weighting
    shelf, hp = k_weighting(16000)
    want = lo.design(16000)
    assert np.array_equal(shelf, [want[0:3], [1.0, want[3], want[4]]]) and np.array_equal(hp, [want[5:8], [1.0, want[8], want[9]]])
    r = np.abs(np.roots(hp[1]))
    assert np.allclose(r, 0.98514, atol=2e-5)      # the high-pass's double pole at 16 kHz: a memory of thousands of samples
    with pytest.raises(ValueError, match="sample_rate"):
        k_weighting(12345)


@pytest.mark.parametrize("sr", [16000, 22050, 48000])
def test_full_scale_997_hz_sine_measures_minus_3_01_lufs(sr):
    """EBU Tech 3341's tolerance is 0.1 LU.  Measured: -2.970, -2.981, -3.010; the offset at the low rates is the bilinear warp."""
    m = lo.measure(lo.sine(997.0, 3.0, sr), sr)
    print("997 Hz at %d Hz: %.4f LUFS" % (sr, m["loudness"]))
    assert abs(m["loudness"] - (-3.01)) < 0.1
    assert m["block_ms"].size == 27 and (m["block_state"] == 2).all() and m["nonfinite"] == 0


def test_short_segments_blocks_and_gates_of_the_oracle():
    sr = 16000
    x = lo.voiced(6399, sr)
    m = lo.measure(x, sr)
    assert m["block_ms"].size == 1 and math.isfinite(m["loudness"])      # n < block: one block of all samples
    assert lo.measure(lo.voiced(6400, sr), sr)["block_ms"].size == 1 and lo.measure(lo.voiced(8000, sr), sr)["block_ms"].size == 2
    z = lo.measure(np.zeros(7000, np.float32), sr)
    assert z["loudness"] == -np.inf and z["rel_threshold"] == -np.inf and z["flags"] == lo.UNDEFINED and z["gain"] == 1.0 and z["peak"] == 0.0
    g = lo.measure(lo.gated_signal(sr), sr)
    assert g["block_ms"].size == 37 and (g["block_state"] == 0).sum() >= 1 and (g["block_state"] == 1).sum() >= 1
    y = x.copy()
    y[[3, 77]] = [np.nan, np.inf]
    n = lo.measure(y, sr)
    assert n["nonfinite"] == 2 and math.isfinite(n["loudness"]) and np.isfinite(n["peak"])
    i16 = np.array([-32768, 5, 32767], np.int16)
    assert lo.measure(i16, sr)["peak"] == 1.0 and np.array_equal(lo.to_f64(i16)[0], [-1.0, 5 / 32768.0, 32767 / 32768.0])


def test_output_rules_of_the_oracle():
    x = np.array([0.5, -1.0, 1.0, 0.99999, -0.3, np.nan, np.inf, -np.inf, 3e-5, -3e-5], np.float32)
    assert np.array_equal(lo.apply_gain(x, 1.0).view(np.uint32), x.view(np.uint32))      # the source bits
    out = lo.apply_gain(x, 1.5)
    assert np.array_equal(out[:5], x[:5] * np.float32(1.5))
    assert lo.to_i16(out).tolist() == [24576, -32768, 32767, 32767, -14745, 0, 32767, -32768, 1, -1]      # clamped, truncated toward zero, NaN -> 0
    assert lo.to_i16(lo.apply_gain(np.array([-32768, 16384], np.int16), 1.0)).tolist() == [-32768, 16384]


def test_gain_for_matches_the_rule_on_a_grid():
    from emotivoice_amd.loudness import FLAG_BOOST_LIMITED, FLAG_PEAK_LIMITED, FLAG_UNDEFINED, LoudnessConfig, gain_for
    assert (FLAG_UNDEFINED, FLAG_BOOST_LIMITED, FLAG_PEAK_LIMITED) == (lo.UNDEFINED, lo.BOOST_LIMITED, lo.PEAK_LIMITED) == (
        _ffi.EV_LOUDNESS_UNDEFINED, _ffi.EV_LOUDNESS_BOOST_LIMITED, _ffi.EV_LOUDNESS_PEAK_LIMITED)
    seen = set()
    for target in (float("nan"), -70.0, -23.0, -16.0, 0.0):
        for L in (-np.inf, -69.5, -40.0, -23.0, -16.0, -3.01, 2.5):
            for peak in (0.0, 1e-4, 0.25, 0.8912509, 1.0, 3.5):
                for mg, pc in ((20.0, np.float32(10 ** (-1 / 20.0))), (0.0, 1.0), (6.0, 0.5)):
                    cfg = LoudnessConfig(target_lufs=target, max_gain_db=mg, peak_ceiling=float(pc))
                    g, f = gain_for(L, peak, cfg)
                    wg, wf = lo.gain_for(L, np.float32(peak), target, mg, np.float32(pc))
                    assert g.dtype == np.float32 and g == wg and f == wf, (target, L, peak, mg, pc, g, wg, f, wf)
                    seen.add(f)
                    if math.isnan(target):
                        assert g == 1.0 and f == (FLAG_UNDEFINED if L == -np.inf else 0)
                    else:
                        assert g <= np.float32(10 ** (mg / 20.0)) and (peak == 0 or float(g) * peak <= float(np.float32(pc)) * (1 + 2e-7))
    assert seen >= {0, 1, 2, 4, 1 | 4, 2 | 4}
    # the four steps in the order written: the target, the boost limit, the peak limit, the rounding
    cfg = LoudnessConfig(target_lufs=-16.0)
    assert gain_for(-26.0, 0.1, cfg) == (np.float32(10.0 ** 0.5), 0)
    assert gain_for(-46.0, 0.01, cfg) == (np.float32(10.0), FLAG_BOOST_LIMITED)
    assert gain_for(-46.0, 0.5, cfg) == (np.float32(float(np.float32(cfg.peak_ceiling)) / 0.5), FLAG_BOOST_LIMITED | FLAG_PEAK_LIMITED)
    assert gain_for(-np.inf, 0.0, cfg) == (np.float32(1.0), FLAG_UNDEFINED)


def test_default_config_and_python_config_agree():
    from emotivoice_amd.loudness import DEFAULT_PEAK_CEILING, EXAMPLE_TARGET_LUFS, LoudnessConfig, as_config
    c = _ffi.ev_loudness_config()
    _ffi.lib().ev_default_loudness_config(C.byref(c))
    d = LoudnessConfig().validate().to_struct()
    assert (c.struct_size, c.sample_rate, c.max_gain_db, c.peak_ceiling, c.want_i16) == (C.sizeof(c), 16000, 20.0, np.float32(10 ** (-1 / 20.0)), 0)
    assert math.isnan(c.target_lufs) and math.isnan(d.target_lufs) and LoudnessConfig().measure_only
    assert (d.struct_size, d.sample_rate, d.max_gain_db, d.peak_ceiling, d.want_i16) == (c.struct_size, c.sample_rate, c.max_gain_db, c.peak_ceiling, c.want_i16)
    assert c.peak_ceiling == DEFAULT_PEAK_CEILING and EXAMPLE_TARGET_LUFS == -16.0
    assert (_ffi.EV_LOUDNESS_MAX_SAMPLES, _ffi.EV_LOUDNESS_TILE) == (1 << 30, 4096)
    for kw, needle in ((dict(sample_rate=11025), "sample_rate"), (dict(sample_rate=16000.5), "sample_rate"), (dict(target_lufs=0.5), "target_lufs"),
                       (dict(target_lufs=-70.5), "target_lufs"), (dict(target_lufs=float("inf")), "target_lufs"), (dict(max_gain_db=-1.0), "max_gain_db"),
                       (dict(max_gain_db=float("nan")), "max_gain_db"), (dict(max_gain_db=float("inf")), "max_gain_db"), (dict(peak_ceiling=0.0), "peak_ceiling"),
                       (dict(peak_ceiling=1.0001), "peak_ceiling"), (dict(peak_ceiling=float("nan")), "peak_ceiling")):
        with pytest.raises(ValueError, match=needle):
            LoudnessConfig(**kw).validate()
    for sr in lo.SAMPLE_RATES:
        LoudnessConfig(sample_rate=sr, target_lufs=-16.0, peak_ceiling=1.0, max_gain_db=0.0, want_int16=True).validate()
    # the loudness= argument of synthesize / synthesize_long
    a = as_config(-20, 16000, want_int16=True)
    assert (a.sample_rate, a.target_lufs, a.want_int16, a.max_gain_db) == (16000, -20.0, True, 20.0)
    given = LoudnessConfig(target_lufs=-18.0, max_gain_db=6.0)
    assert as_config(given, 16000) is not None and as_config(given, 16000).max_gain_db == 6.0 and not as_config(given, 16000).want_int16
    for bad, needle in ((LoudnessConfig(sample_rate=48000, target_lufs=-16.0), "engine's"), (LoudnessConfig(), "target"), (True, "loudness"), ("-16", "loudness"),
                        (5.0, "target_lufs")):
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


def test_serving_synth_functions_pass_loudness_through():
    from emotivoice_amd.loudness import LoudnessConfig
    from emotivoice_amd.prosody import Prosody
    from emotivoice_amd.serving import engine_flac_synth_fn, engine_prosody_synth_fn, engine_synth_fn
    utts = [dict(), dict()]
    eng = _FakeEngine()
    # without the setting synthesize is called exactly as before
    engine_synth_fn(eng)(utts, 1.25)
    engine_prosody_synth_fn(eng)(utts, [Prosody(), Prosody()])
    engine_flac_synth_fn(eng)(utts, 0.8, [True, False])
    assert [sorted(c) for c in eng.calls] == [["alpha"], ["prosody"], ["alpha", "flac"]]
    eng.calls.clear()
    cfg = LoudnessConfig(target_lufs=-18.0)
    assert len(engine_synth_fn(eng, loudness=-16.0)(utts, 1.25)) == 2
    engine_prosody_synth_fn(eng, loudness=cfg)(utts, [Prosody(), Prosody()])
    got = engine_flac_synth_fn(eng, loudness=-16.0)(utts, [Prosody(), Prosody()], [False, True])
    assert eng.calls[0] == dict(alpha=1.25, loudness=-16.0)
    assert eng.calls[1]["loudness"] is cfg and "alpha" not in eng.calls[1]
    assert eng.calls[2]["loudness"] == -16.0 and eng.calls[2]["flac"] == [False, True] and "prosody" in eng.calls[2]
    assert isinstance(got[0], np.ndarray) and got[1] == b"fLaC1"


def test_cli_has_the_loudness_flag():
    from emotivoice_amd.inference_tts import build_parser
    p = build_parser()
    assert p.parse_args(["-t", "x.txt"]).loudness is None
    assert p.parse_args(["-t", "x.txt", "--loudness", "-16"]).loudness == -16.0
