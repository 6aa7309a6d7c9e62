"""CPU checks of the pitch specification (include/evhip.h: ev_pitch): the float64 oracle on signals whose F0 is known by construction, its
continuous fill against scipy's interp1d, and PitchConfig.validate.  The bars are those of the specification's prototype runs (worst relative
error 3.7e-4 on steady tones, 0.5 % on the glide), with room to spare; nothing here touches a GPU."""
import numpy as np
import pytest

import pitch_oracle as po
from emotivoice_amd.pitch import PITCH_STATS, PitchConfig

SR = 16000
AMPS = (1.0, 0.5, 0.33, 0.25)


def steady(f, n=8000, amps=AMPS):
    return (0.3 * po.harmonic(np.full(n, f), amps)).astype(np.float32)


def glide(n=SR):
    return (0.3 * po.harmonic(np.linspace(110.0, 330.0, n), AMPS)).astype(np.float32)


def glide_truth(T, hop=256, n=SR):
    """F0 of the glide at the frame centres t hop"""
    return 110.0 + 220.0 * np.minimum(np.arange(T) * hop, n - 1) / (n - 1)


@pytest.mark.parametrize("f", [80.5, 100.0, 133.3, 220.0, 311.0, 399.0])
def test_steady_tones(f):
    o = po.pitch64(steady(f))
    inner = slice(3, -3)
    assert o["voiced"][inner].all(), f
    err = np.abs(o["f0"][inner] - f).max() / f
    print(f, "worst relative error %.2e" % err)
    assert err <= 1e-3, (f, err)


def test_glide():
    o = po.pitch64(glide())
    T = o["f0"].size
    inner = slice(3, T - 3)
    truth = glide_truth(T)[inner]
    assert o["voiced"][inner].all()
    err = (np.abs(o["f0"][inner] - truth) / truth).max()
    print("glide worst relative error %.2e" % err)
    assert err <= 1e-2, err


def test_missing_fundamental():
    o = po.pitch64(steady(120.0, amps=(0.0, 1.0, 0.7, 0.5)))
    inner = slice(3, -3)
    assert o["voiced"][inner].all()
    assert np.abs(o["f0"][inner] - 120.0).max() / 120.0 <= 1e-3


def test_noise_and_silence_are_unvoiced():
    rng = np.random.default_rng(5)
    o = po.pitch64((0.3 * rng.standard_normal(8000)).astype(np.float32))
    assert not o["voiced"].any() and (o["f0"] == 0).all()
    z = po.pitch64(np.zeros(5000, np.float32), stats=(200.0, 50.0))
    assert not z["voiced"].any() and (z["aperiodicity"] == 1.0).all() and (z["cont"] == 0).all()
    assert np.array_equal(z["pitch"], np.full(z["pitch"].shape, -4.0))


def test_float32_sequential_mode_is_close_to_float64():
    w = steady(220.0, 4000)
    a, b = po.pitch64(w), po.pitch64(w, dtype=np.float32, sequential=True)
    assert b["f0"].dtype == np.float32 and np.array_equal(a["tau"], b["tau"])
    assert po.rel_error(b["f0"], a["f0"]) <= 1e-4


def _interp_fill(f0):
    from scipy.interpolate import interp1d
    v = np.nonzero(f0 > 0)[0]
    if v.size == 0:
        return np.zeros_like(f0)
    if v.size == 1:
        return np.full_like(f0, f0[v[0]])
    f = interp1d(v, f0[v], bounds_error=False, fill_value=(f0[v[0]], f0[v[-1]]))
    return f(np.arange(f0.size))


def test_fill_equals_interp1d_with_edge_hold():
    rng = np.random.default_rng(2)
    cases = []
    for T in (1, 2, 17, 64, 65, 300):
        for p in (0.1, 0.5, 0.9):
            f0 = np.where(rng.random(T) < p, rng.uniform(80.0, 400.0, T), 0.0)
            cases.append(f0)
    one = np.zeros(40)
    one[23] = 200.0
    ends = np.zeros(40)
    ends[0], ends[-1] = 100.0, 300.0
    cases += [one, ends, rng.uniform(80.0, 400.0, 33), np.zeros(12)]
    for f0 in cases:
        got, want = po.fill(f0), _interp_fill(f0)
        assert np.allclose(got, want, rtol=1e-12, atol=0), f0
        assert np.array_equal(got[f0 > 0], f0[f0 > 0])
    assert (po.fill(np.zeros(12)) == 0).all()
    assert np.array_equal(po.fill(one), np.full(40, 200.0))
    assert po.fill(ends)[13] == pytest.approx(100.0 + 200.0 * 13 / 39, rel=1e-14)
    assert po.fill(np.asarray(one, np.float32)).dtype == np.float32


def test_config_defaults_and_rejections():
    c = PitchConfig().validate()
    assert c.tau_range() == (40, 200) and PitchConfig(hop=128, win=512, f_min=100.0, f_max=500.0).validate().tau_range() == (32, 160)
    assert PITCH_STATS == (225.089, 53.78)
    import dataclasses
    assert all(f.default not in PITCH_STATS for f in dataclasses.fields(PitchConfig))
    for kw, needle in ((dict(hop=0), "hop"), (dict(hop=2048), "hop"), (dict(win=4096), "win"), (dict(win=2048, hop=2048), "win"),
                       (dict(f_min=0.0), "f_min"), (dict(f_min=500.0), "f_min"), (dict(f_max=4001.0), "f_max"), (dict(f_max=float("nan")), "f_max"),
                       (dict(f_min=float("inf")), "f_min"), (dict(f_min=10.0), "tau_max"), (dict(threshold=0.0), "threshold"),
                       (dict(threshold=1.5), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(silence_rms=-1.0), "silence_rms"),
                       (dict(silence_rms=float("inf")), "silence_rms"), (dict(sample_rate=0), "sample_rate")):
        with pytest.raises(ValueError, match=needle):
            PitchConfig(**kw).validate()
    from emotivoice_amd.pitch import check_stats, pack_wavs
    for bad, needle in (((float("nan"), 1.0), "pitch_mean"), ((0.0, 0.0), "pitch_std"), ((0.0, -2.0), "pitch_std"), ((0.0, float("inf")), "pitch_std")):
        with pytest.raises(ValueError, match=needle):
            check_stats(bad)
    flat, is16, lens = pack_wavs([np.zeros(1, np.float32), np.ones(300, np.float64)])
    assert flat.dtype == np.float32 and not is16 and lens.tolist() == [1, 300]
    with pytest.raises(ValueError, match=r"wavs\[1\]"):
        pack_wavs([np.zeros(4, np.float32), np.zeros(0, np.float32)])


def test_frame_grid_is_the_features_grid():
    for L in (1, 255, 256, 777, 5000):
        o = po.pitch64(np.zeros(L, np.float32))
        assert o["f0"].size == L // 256 + 1
