"""ev_stretch without a GPU: the numpy restatement (tests/stretch_oracle.py) against the consequences of the rules, every deliberately wrong rule
caught by a named case, the host rule for the lengths against the library's ev_stretch_plan, the window, StretchConfig and synthesize_fit's
arithmetic."""
import ctypes as C

import numpy as np
import pytest

import stretch_oracle as so
from emotivoice_amd import _ffi
from emotivoice_amd.stretch import FRAME, HOP, LAGS, MAX_SAMPLES, StretchConfig, fit_alpha, plan_lengths, stretch_config

EDGE_LENGTHS = [(1, 1), (1, 2), (2, 1), (255, 300), (257, 129), (511, 1022), (513, 257)]


def noise(n, seed=0, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- consequences of the rules
def test_equal_lengths_return_finite_input_bit_for_bit():
    for n in (1, 255, 256, 257, 5000):
        x = noise(n, n)
        r = so.stretch(x, n)
        assert np.array_equal(bits(r["wav"]), bits(x)) and r["sum_dist"] == 0 and r["edge_frames"] == 0 and not r["deltas"].any()
    x16 = (noise(3000, 7) * 32768).astype(np.int16)
    assert np.array_equal(so.stretch(x16, 3000)["wav"], x16.astype(np.float32) / np.float32(32768))
    assert np.array_equal(so.stretch(x16, 3000)["wav_i16"], x16)


@pytest.mark.parametrize("P", [57, 80, 128])
def test_periodic_input_comes_out_periodic(P):
    """y[m] == x[m % P] for all m < L_out - 2304: the last 896 / 0.5 + 256 = 2048 outputs may read the zero extension, plus one hop of slack."""
    base = noise(P, P)
    x = np.tile(base, 20000 // P + 1)[:20000]
    for speed in (0.5, 0.8, 1.25, 1.37, 2.0):
        L_out = so.plan_length(20000, speed)
        y = so.stretch(x, L_out)["wav"]
        m = np.arange(L_out - 2304)
        assert np.array_equal(bits(y[m]), bits(base[m % P])), (P, speed)


def test_known_answers_at_the_edge_lengths():
    for L_in, L_out in EDGE_LENGTHS:
        r = so.stretch(noise(L_in, L_in), L_out)
        assert r["wav"].shape == (L_out,) and np.all(np.isfinite(r["wav"])) and r["deltas"][0] == 0
        assert r["frames"] == -(-L_out // HOP) == r["deltas"].size and r["nonfinite"] == 0
    # p_0 = 0, p_(-1) = -H: the first hop is the input itself wherever the input reaches
    x = noise(511, 511)
    assert np.array_equal(so.stretch(x, 1022)["wav"][:256], x[:256])
    assert so.stretch(noise(1, 1), 2)["wav"].tolist() == [float(noise(1, 1)[0]), 0.0]
    r = so.stretch(noise(255, 255), 300)
    assert r["frames"] == 2 and -128 <= int(r["deltas"][1]) <= 127


def test_nonfinite_samples_decide_as_zero_and_are_counted():
    x = noise(3000, 3)
    bad = x.copy()
    bad[[5, 700, 2999]] = [np.nan, np.inf, -np.inf]
    zeroed = np.where(np.isfinite(bad), bad, np.float32(0))
    a, b = so.stretch(bad, 2400), so.stretch(zeroed, 2400)
    assert a["nonfinite"] == 3 and b["nonfinite"] == 0
    assert np.array_equal(a["deltas"], b["deltas"]) and a["sum_dist"] == b["sum_dist"]
    ok = np.isfinite(a["wav"])
    assert not ok.all() and np.array_equal(a["wav"][ok], b["wav"][ok])
    nan = np.isnan(a["wav"])      # int16: NaN -> 0, an infinity clamps
    assert nan.any() and not a["wav_i16"][nan].any() and set(a["wav_i16"][~ok & ~nan].tolist()) <= {32767, -32768}
    assert np.array_equal(so.quantise(np.array([1.0, -1.0, 4.0, -4.0, 0.99976, 2.44140625e-4, 7.32421875e-4], np.float32)),
                          [2047, -2047, 2047, -2047, 2047, 0, 2])      # the clamp; ties to even at 0.5 and 1.5


# ---------------------------------------------------------------- every deliberately wrong rule is caught by a named case
def test_the_reversed_tie_rule_is_caught_by_silence():
    x = np.zeros(2000, np.float32)
    assert not so.stretch(x, 1600)["deltas"].any()
    assert so.stretch(x, 1600, so.Rules(tie_reversed=True))["deltas"][1:].tolist() == [-128] * 6
    # and by a periodic input, whose ties lie a period apart: the nearest one wins
    base = noise(80, 80)
    x = np.tile(base, 250)
    right, wrong = so.stretch(x, 16000)["deltas"], so.stretch(x, 16000, so.Rules(tie_reversed=True))["deltas"]
    assert not np.array_equal(right, wrong)
    assert np.abs(right[:-10]).max() <= 40 < np.abs(wrong[:-10]).max()      # away from the zero extension at the end


def test_the_truncated_read_position_is_caught_by_1000_to_777():
    x = noise(1000, 1000)
    right, wrong = so.stretch(x, 777), so.stretch(x, 777, so.Rules(a_truncated=True))
    assert (2 * 2 * HOP * 1000 + 777) // (2 * 777) == 659 and (2 * HOP * 1000) // 777 == 658      # frame 2 reads one sample later when rounded
    assert not np.array_equal(right["deltas"], wrong["deltas"])


def test_the_nominal_template_is_caught_by_noise_at_speed_1_1():
    x = noise(20011, 20011)
    L_out = so.plan_length(20011, 1.1)
    right, wrong = so.stretch(x, L_out), so.stretch(x, L_out, so.Rules(template_nominal=True))
    assert right["deltas"].any() and not np.array_equal(right["deltas"], wrong["deltas"])
    assert not np.array_equal(bits(right["wav"]), bits(wrong["wav"]))


def test_sixteen_bit_samples_with_wrapping_sums_are_caught_by_full_scale_noise():
    x = noise(6000, 6000, scale=1.5)      # beyond full scale: q clamps at 2047, and 512 squares of 16-bit differences leave int32
    right, wrong = so.stretch(x, 5000), so.stretch(x, 5000, so.Rules(q16_wrapping=True))
    assert np.abs(so.quantise(x)).max() == 2047 and 512 * 4094 ** 2 > 2 ** 32 > 128 * 4094 ** 2
    assert not np.array_equal(right["deltas"], wrong["deltas"]) and right["sum_dist"] != wrong["sum_dist"]


def test_a_window_off_the_lattice_is_caught_by_noise_at_speed_1_1():
    w = so.window()
    assert w[0] == 0 and w[128] == 0.5 and np.array_equal(w.astype(np.float64) * 2 ** 23, np.rint(w.astype(np.float64) * 2 ** 23))
    assert np.all((np.float32(1) - w).astype(np.float64) + w.astype(np.float64) == 1.0)
    off = so.window(so.Rules(window_float=True))
    assert not np.array_equal(off, w) and np.abs(off.astype(np.float64) - w.astype(np.float64)).max() <= 2.0 ** -24
    x = noise(20011, 20011)
    L_out = so.plan_length(20011, 1.1)
    right, wrong = so.stretch(x, L_out), so.stretch(x, L_out, so.Rules(window_float=True))
    assert np.array_equal(right["deltas"], wrong["deltas"]) and not np.array_equal(bits(right["wav"]), bits(wrong["wav"]))


# ---------------------------------------------------------------- the built library's host entry points (no GPU)
def lib_plan(lens, speeds=None, targets=None):
    lib = _ffi.lib()
    ln = np.ascontiguousarray(lens, np.int64)
    sp = None if speeds is None else np.ascontiguousarray(speeds, np.float64)
    tg = None if targets is None else np.ascontiguousarray([0 if t is None else t for t in targets], np.int64)
    out = np.zeros(ln.size, np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = lib.ev_stretch_plan(ln.size, p(ln), p(sp), p(tg), p(out))
    return (out, None) if rc == 0 else (None, lib.ev_last_error(None).decode())


def test_the_library_window_is_the_oracles():
    w = np.zeros(HOP, np.float32)
    assert _ffi.lib().ev_stretch_window(w.ctypes.data_as(C.c_void_p)) == HOP
    assert np.array_equal(bits(w), bits(so.window()))
    assert _ffi.lib().ev_stretch_window(None) == -1
    assert (FRAME, HOP, LAGS, MAX_SAMPLES) == (_ffi.EV_STRETCH_FRAME, _ffi.EV_STRETCH_HOP, _ffi.EV_STRETCH_LAGS, _ffi.EV_STRETCH_MAX_SAMPLES) == (so.N, so.H, so.LAGS, so.MAX_SAMPLES)


def test_plan_lengths_agrees_with_the_library_on_edges_and_rejections():
    accepted = [  # (L_in, speed, target)
        (5, 2.0, None), (7, 2.0, None), (3, 2.0, None), (1, 2.0, None), (1, 1000.0, None),      # 2.5 -> 2, 3.5 -> 4, 1.5 -> 2, 0.5 -> 0 -> 1
        (20011, 0.5, None), (20011, 0.9, None), (20011, 1.1, None), (20011, 2.0, None), (16000, 1.37, None), (16000, None, None),
        (1024, None, 512), (512, None, 1024), (1024, None, 511), (511, None, 5000), (5000, None, 1), (1 << 30, None, 1 << 30), (1 << 30, 2.0, None),
        (1 << 29, 0.5, None),
    ]
    for L_in, s, t in accepted:
        got, err = lib_plan([L_in], None if s is None else [s], None if t is None else [t])
        assert err is None, (L_in, s, t, err)
        want = plan_lengths([L_in], [s], [t])
        assert got.tolist() == want.tolist() == [so.plan_length(L_in, s, t)], (L_in, s, t)
    assert plan_lengths([5, 7, 3, 1], [2.0] * 4).tolist() == [2, 4, 2, 1]
    rejected = [
        (0, 1.0, None, "lens[1] = 0 < 1"), (100, None, -3, "lens_out[1] = -3 < 1"), (100, 0.0, None, "speeds[1]"), (100, float("nan"), None, "speeds[1]"),
        (100, float("inf"), None, "speeds[1]"), (100, -1.0, None, "speeds[1]"), ((1 << 30) + 1, None, 1 << 30, "lens[1] = 1073741825 > EV_STRETCH_MAX_SAMPLES"),
        (1 << 30, None, (1 << 30) + 1, "lens_out[1] = 1073741825 > EV_STRETCH_MAX_SAMPLES"), (1 << 30, 0.999, None, "lens_out[1]"),
        (1025, None, 512, "segment 1: 1025 -> 512 samples lies outside the ratios [0.5, 2]"), (512, None, 1025, "segment 1: 512 -> 1025"),
        (20011, 2.001, None, "segment 1"), (20011, 0.4999, None, "segment 1"), (100, 1e-300, None, "lens_out[1]"),
    ]
    for L_in, s, t, text in rejected:      # segment 1 of two: the message names it
        args = ([4000, L_in], None if s is None else [1.0, s], None if t is None else [None, t])
        got, err = lib_plan(*args)
        assert got is None and text in err and err.startswith("ev_stretch_plan: "), (L_in, s, t, err)
        with pytest.raises(ValueError) as e:
            plan_lengths(*args)
        assert text in str(e.value), (str(e.value), err)
        if not text.startswith("speeds"):      # the same sentence; a speed is printed by two different formatters
            assert err == "ev_stretch_plan: " + str(e.value)
    assert lib_plan([], None, None)[1] == "ev_stretch_plan: B = 0 outside [1, 65535]"


# ---------------------------------------------------------------- the Python configuration
def test_stretch_config_validation():
    assert stretch_config(None) is None and stretch_config(False) is None
    assert stretch_config(1.25).speed == 1.25 and stretch_config([1.25, 0.8]).speed == [1.25, 0.8]
    assert stretch_config(np.array([1.25, 0.8])).per_segment(2, 16000) == ([1.25, 0.8], [None, None])
    c = StretchConfig(samples=777)
    assert stretch_config(c) is c
    for bad in ("fast", True, {"speed": 2}):
        with pytest.raises(ValueError):
            stretch_config(bad)
    for kw in (dict(speed=0.0), dict(speed=-1.0), dict(speed=float("nan")), dict(speed=float("inf")), dict(seconds=0.0), dict(samples=0), dict(samples=2.5),
               dict(samples=True), dict(speed="2"), dict(speed=[1.0, "x"]), dict(speed=2.0, seconds=1.0), dict(seconds=1.0, samples=16000), dict(speed={1: 2})):
        with pytest.raises(ValueError):
            StretchConfig(**kw).validate()
    # one entry per segment; each segment at most one of the three; none = speed 1
    mixed = StretchConfig(speed=[2.0, None, None, None], seconds=[None, 2.5, None, None], samples=[None, None, 777, None])
    assert mixed.per_segment(4, 16000) == ([2.0, None, None, None], [None, 40000, 777, None])
    assert mixed.lengths([30000, 30000, 1000, 123]).tolist() == [15000, 40000, 777, 123]
    assert StretchConfig(seconds=0.25).per_segment(2, 8000)[1] == [2000, 2000]
    assert StretchConfig(seconds=[0.00003125, 0.00009375]).per_segment(2, 16000)[1] == [0, 2]      # 0.5 -> 0, 1.5 -> 2: ties to even
    with pytest.raises(ValueError, match="lens_out\\[0\\] = 0 < 1"):
        StretchConfig(seconds=0.00003125).lengths([100])
    with pytest.raises(ValueError, match="one entry per segment \\(3\\), got 2"):
        StretchConfig(speed=[1.0, 2.0]).per_segment(3, 16000)
    with pytest.raises(ValueError, match="segment 1: only one of speed, samples"):
        StretchConfig(speed=[None, 2.0], samples=[5, 5]).per_segment(2, 16000)
    with pytest.raises(ValueError, match="segment 0: 16000 -> 48000"):
        StretchConfig(seconds=3.0).lengths([16000])
    s = StretchConfig(want_int16=True).to_struct()
    assert (s.struct_size, s.want_int16) == (C.sizeof(_ffi.ev_stretch_config), 1) and StretchConfig().to_struct().want_int16 == 0


def test_fit_alpha_is_the_clamped_ratio():
    assert fit_alpha(16000, 40000) == 2.0 and fit_alpha(40000, 16000) == 0.5 and fit_alpha(32000, 40000) == 1.25 and fit_alpha(25600, 25600) == 1.0
    assert fit_alpha(30000, 40000) == 40000 / 30000


def test_cli_has_the_time_stretch_flag():
    from emotivoice_amd.inference_tts import build_parser, chain_from_args
    p = build_parser()
    assert p.parse_args(["-t", "x"]).time_stretch is None and "stretch" not in chain_from_args(p.parse_args(["-t", "x"]))
    assert chain_from_args(p.parse_args(["-t", "x", "--time-stretch", "1.25"]))["stretch"] == 1.25
    import argparse
    from emotivoice_amd.inference_tts import add_delivery_arguments, add_stretch_argument
    joint = argparse.ArgumentParser()      # the two arguments the other mirror adds to its parser
    add_stretch_argument(joint)
    add_delivery_arguments(joint)
    assert chain_from_args(joint.parse_args(["--time-stretch", "0.8"])) == dict(stretch=0.8)
