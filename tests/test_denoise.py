"""Vocoder bias removal on the CPU: the float64 oracle (tests/denoise_oracle.py) against the fixtures of the reference's own STFT class
(tests/golden/denoise, made by make_golden_denoise.py), the identity at strength 0, the output lengths, the envelope table against the
reference's window_sumsquare, the configuration, and the place of ev_denoise in the output chain of EVEngine against the stand-in library of
tests/fake_evhip.py with a trivial ev_denoise added: it ADDS 1/8 and cuts every utterance to whole hops."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import denoise_oracle as do
import fake_evhip as fk
import features_oracle as fo
from conftest import GOLDEN_DIR
from emotivoice_amd import _ffi
from emotivoice_amd.denoise import DEFAULT_STRENGTH, DenoiseConfig, denoise_config, out_len, removed_db

DN_DIR = os.path.join(GOLDEN_DIR, "denoise")
FIXTURES = sorted(glob.glob(os.path.join(DN_DIR, "dn_[a-g]_*.npz")))
DEV = _ffi.EV_FLAG_DEVICE_INPUTS
# the reference accumulates n_fft = 1024 float32 products per cell and per sample: sqrt(1024) * 2^-24 of the peak
REF_BOUND = 32 * 2.0 ** -24


def test_the_fixtures_are_the_ones_the_issue_lists():
    names = [os.path.basename(p)[:-4] for p in FIXTURES]
    assert names == ["dn_a_l513", "dn_b_l2048", "dn_c_l20011", "dn_d_l20011_i16", "dn_e_l20011_s0", "dn_f_l20011_s30", "dn_g_l8192_zeros"]
    gs = [dict(np.load(p)) for p in FIXTURES]
    assert [g["wav"].size for g in gs] == [513, 2048, 20011, 20011, 20011, 20011, 8192]
    assert gs[3]["wav"].dtype == np.int16 and all(g["wav"].dtype == np.float32 for g in gs[:3])
    assert [round(float(g["strength"]), 3) for g in gs] == [0.1, 0.1, 0.1, 0.1, 0.0, 30.0, 0.1]
    assert np.all(gs[6]["wav"][2048:6144] == 0)
    assert all(os.path.getsize(p) < 1_000_000 for p in glob.glob(os.path.join(DN_DIR, "*.npz")))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_oracle_against_the_reference(path):
    """The reference's float32 transform -> clamp -> inverse lies within its own float32 error of the float64 closed form, the recorded ref_err is
    that error, and the output has hop * (L // hop) samples."""
    g = dict(np.load(path))
    y64 = do.denoise64(g["wav"], g["bias"], float(g["strength"]))
    assert y64.size == g["ref_out"].size == out_len(g["wav"].size) == 256 * (g["wav"].size // 256)
    e = do.peak_error(g["ref_out"], y64)
    print(os.path.basename(path), "E(ref)", e)
    assert e == pytest.approx(float(g["ref_err"]), rel=1e-6) and e <= REF_BOUND


def test_oracle_inverse_against_the_references_inverse():
    g = dict(np.load(os.path.join(DN_DIR, "dn_h_inverse_t9.npz")))
    assert np.all(g["im"][:, 0] == 0) and np.all(g["im"][:, -1] == 0)
    y64 = do.istft64(g["re"].astype(np.float64), g["im"].astype(np.float64))
    e = do.peak_error(g["ref_out"], y64)
    assert y64.size == 2048 and e == pytest.approx(float(g["ref_err"]), rel=1e-6) and e <= REF_BOUND
    # the weights 1, 2, ..., 2, 1 matter: the all-two basis is far outside
    assert do.peak_error(g["ref_out"], do.istft64(g["re"].astype(np.float64), g["im"].astype(np.float64), all_two=True)) > 100 * REF_BOUND


def test_strength_zero_is_the_identity_edges_included():
    """3 x 2^-24 of the peak: the float32 rounding of the three tables (forward basis, inverse basis, envelope: half an ulp, 2^-24 relative, each)
    is all that separates the float64 round trip from the input."""
    for path in (FIXTURES[0], FIXTURES[2]):
        g = dict(np.load(path))
        y = do.denoise64(g["wav"], g["bias"], 0.0)
        assert do.peak_error(y, g["wav"][:y.size]) <= 3 * 2.0 ** -24
    z = np.zeros(1024, np.float32)
    assert np.all(do.denoise64(z, np.ones(513, np.float32), 1.0) == 0)          # mag == 0: zero cells, no NaN


def test_envelope_table_is_the_references_window_sumsquare():
    """Bit for bit, for every T of the fixture (1, 3 and 4 frames: both ends reach into every chunk)."""
    ref = dict(np.load(os.path.join(DN_DIR, "dn_envelope.npz")))
    tab = do.envelope_table()
    assert tab.shape == (4, 4, 256) and tab.dtype == np.float32
    for key, ws in ref.items():
        T = int(key[1:])
        assert np.array_equal(do.envelope_from_table(tab, T), ws) and np.array_equal(do.envelope_f32(T), ws), key
    interior = ref["T79"][1024:-1024].reshape(-1, 256)
    assert np.all(interior == tab[0, 3][None, :]) and abs(float(tab[0, 3].mean()) - 1.5) < 1e-6      # constant in between: 4 hann^2 sum to 1.5
    # another shape, against the plain statement
    t2 = do.envelope_table(512, 128)
    for T in (1, 2, 5, 11):
        assert np.array_equal(do.envelope_from_table(t2, T, 512, 128), do.envelope_f32(T, 512, 128))


SHAPE_FIXTURES = sorted(glob.glob(os.path.join(DN_DIR, "dn_shape_*.npz")))


def test_the_shape_fixtures_are_the_three_shapes():
    assert [os.path.basename(p)[:-4] for p in SHAPE_FIXTURES] == ["dn_shape_128_128", "dn_shape_384_48", "dn_shape_640_320"]
    assert all(os.path.getsize(p) < 100_000 and np.load(p)["wav"].size == 2000 for p in SHAPE_FIXTURES)


@pytest.mark.parametrize("path", SHAPE_FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_oracle_against_the_reference_at_other_shapes(path):
    """The reference's STFT class built at 384 / 48 (R = 8), 640 / 320 (R = 2) and 128 / 128 (R = 1): its transform's magnitudes, its transform ->
    clamp -> inverse and its window_sumsquare against the oracle at the same shape.  The float32 rounding REF_BOUND describes is that of the
    overlap-added sum, before the division by the envelope; the division multiplies it by 1 / env.  For R >= 2 the envelope of the trimmed signal
    stays near its mean and the plain error is inside the bound.  At R = 1 a lone hann^2 comes down to sin^4(pi / 128) = 3.6e-7 next to every chunk
    edge, so there the bound is held on the error times env / max env, and the plain error (recorded: 1.6e-4) is the conditioning of that shape, which
    the reference's float32 run shows like any other float32 run."""
    g = dict(np.load(path))
    n_fft, hop = int(g["n_fft"]), int(g["hop"])
    T = 2000 // hop + 1
    re, im = do.stft64(g["wav"], n_fft, hop)
    assert g["ref_mag"].shape == re.shape == (T, n_fft // 2 + 1)
    e_mag = fo.mag_error(g["ref_mag"], np.sqrt(re * re + im * im))
    y64 = do.denoise64(g["wav"], g["bias"], float(g["strength"]), n_fft, hop)
    assert y64.size == g["ref_out"].size == out_len(2000, hop) == hop * (T - 1)
    e = do.peak_error(g["ref_out"], y64)
    env = do.envelope_f32(T, n_fft, hop).astype(np.float64)[n_fft // 2:n_fft // 2 + y64.size]
    e_sum = float((np.abs(g["ref_out"] - y64) * env / env.max()).max() / np.abs(y64).max())
    print(os.path.basename(path), "E_mag(ref) %.3e E(ref) %.3e before the division %.3e" % (e_mag, e, e_sum))
    assert e == pytest.approx(float(g["ref_err"]), rel=1e-6) and e_mag <= REF_BOUND and e_sum <= REF_BOUND
    assert e <= REF_BOUND or n_fft == hop
    # window_sumsquare, bit for bit, T < R included: both ends reach into the same chunk
    tab = do.envelope_table(n_fft, hop)
    keys = [k for k in g if k.startswith("env_T")]
    assert len(keys) >= 3 and (n_fft == hop or any(int(k[5:]) < n_fft // hop for k in keys))
    for k in keys:
        assert np.array_equal(do.envelope_f32(int(k[5:]), n_fft, hop), g[k]) and np.array_equal(do.envelope_from_table(tab, int(k[5:]), n_fft, hop), g[k]), k


def test_gain64_selects_a_zero_cell_where_mag_is_not_greater_than_zero():
    """Step 3 of include/evhip.h: mag == 0 and a NaN give a zero cell -- 0, not 0 * NaN; every other cell is untouched by the rule."""
    rng = np.random.default_rng(2)
    re, im = rng.standard_normal((4, 9)), rng.standard_normal((4, 9))
    bias = np.abs(rng.standard_normal(9)).astype(np.float32)
    want = do.gain64(re, im, bias, 0.5)
    re2, im2 = re.copy(), im.copy()
    re2[1, 3], im2[2, :] = np.nan, np.nan
    re2[3, 4] = im2[3, 4] = 0.0
    gre, gim, mag = do.gain64(re2, im2, bias, 0.5)
    dead = np.zeros((4, 9), bool)
    dead[1, 3] = dead[2, :] = dead[3, 4] = True
    assert np.all(gre[dead] == 0) and np.all(gim[dead] == 0) and np.all(np.isfinite(gre)) and np.all(np.isfinite(gim))
    assert np.array_equal(gre[~dead], want[0][~dead]) and np.array_equal(gim[~dead], want[1][~dead]) and np.isnan(mag[1, 3])
    # and through the inverse: a frame of NaN cells contributes nothing
    w = (0.3 * rng.standard_normal(2048)).astype(np.float32)
    r, i = do.stft64(w)
    r[4], i[4] = np.nan, np.nan
    r0, i0 = np.where(np.isnan(r), 0.0, r), np.where(np.isnan(i), 0.0, i)
    b513 = np.full(513, 0.01, np.float32)
    y = do.istft64(*do.gain64(r, i, b513, 0.1)[:2])
    assert np.all(np.isfinite(y)) and np.array_equal(y, do.istft64(*do.gain64(r0, i0, b513, 0.1)[:2]))


def test_config_window_is_part_of_the_setup_key():
    w = np.hanning(1024).astype(np.float32)
    assert DenoiseConfig(window=w).validate().key() != DenoiseConfig().key() and DenoiseConfig(window=w).key() == DenoiseConfig(window=w.copy()).key()
    assert DenoiseConfig(window=w).tables_key() != DenoiseConfig().tables_key() == DenoiseConfig(strength=0.3).tables_key()
    for bad in (DenoiseConfig(window=w[:512]), DenoiseConfig(window=np.full(1024, np.nan))):
        with pytest.raises(ValueError):
            bad.validate()


def test_config_validation():
    assert DenoiseConfig().validate().strength == DEFAULT_STRENGTH == 0.01
    assert denoise_config(None) is None and denoise_config(False) is None
    assert denoise_config(True).strength == 0.01 and denoise_config(0.1).strength == 0.1 and denoise_config(0).strength == 0.0
    c = denoise_config(dict(strength=0.2, report=True))
    assert (c.strength, c.report, c.n_fft, c.hop, c.want_int16) == (0.2, True, 1024, 256, False)
    given = DenoiseConfig(strength=0.3, bias=np.ones(513, np.float32))
    assert denoise_config(given) is given
    assert given.key() != DenoiseConfig(strength=0.3).key() and DenoiseConfig(0.3).key() == DenoiseConfig(0.3, report=True).key()
    for bad in (DenoiseConfig(strength=-0.1), DenoiseConfig(strength=float("nan")), DenoiseConfig(strength=float("inf")), DenoiseConfig(strength=True),
                DenoiseConfig(n_fft=1000), DenoiseConfig(n_fft=4096), DenoiseConfig(hop=96), DenoiseConfig(hop=64), DenoiseConfig(n_fft=2048, hop=512),
                DenoiseConfig(bias=np.ones(512, np.float32)), DenoiseConfig(bias=-np.ones(513, np.float32)), DenoiseConfig(bias=np.full(513, np.nan))):
        with pytest.raises(ValueError):
            bad.validate()
    for bad in ("0.1", [0.1], object()):
        with pytest.raises(ValueError):
            denoise_config(bad)
    DenoiseConfig(n_fft=512, hop=128).validate()
    DenoiseConfig(n_fft=2048, hop=256).validate()
    assert out_len(20011) == 19968 and out_len(513) == 512 and out_len(255) == 0
    assert removed_db([1.0, 0.0], [100.0, 4.0]).tolist() == [-20.0, -np.inf]


def test_cli_has_the_denoise_flag():
    from emotivoice_amd.inference_tts import build_parser
    p = build_parser()
    assert p.parse_args(["-t", "x"]).denoise is None
    assert p.parse_args(["-t", "x", "--denoise", "0.01"]).denoise == 0.01


# ---------------------------------------------------------------- the chain, against the stand-in library
TOKENS = (3, 5, 2)
LENS = [t * fk.UP for t in TOKENS]
OFFS = np.concatenate([[0], np.cumsum(LENS)])
N = int(OFFS[-1])
EIGHTH, DenoiseLib = fk.EIGHTH, fk.DenoiseLib


def utterances():
    return [dict(ling=np.arange(t) + 1, speaker=b, style=np.zeros(768, np.float32), content=np.zeros(768, np.float32)) for b, t in enumerate(TOKENS)]


@pytest.fixture
def eng(monkeypatch):
    lib = DenoiseLib()
    monkeypatch.setattr(_ffi, "lib", lambda: lib)
    from emotivoice_amd.engine import EVEngine
    e = EVEngine()
    e.fake = lib
    yield e
    e.close()


def test_denoise_runs_first_and_the_bias_is_measured_before_the_synthesis(eng):
    lib = eng.fake
    out = eng.synthesize(utterances(), denoise=0.1, loudness=-16.0, limiter=-1.0, want_int16=True, flac=True)
    assert lib.names() == ["ev_denoise_setup", "ev_vocoder(zero mel)", "ev_denoise_bias", "ev_synthesize", "ev_denoise", "ev_loudness", "ev_limit", "ev_flac"]
    assert lib.calls("ev_denoise_setup")[0]["bias"] is None      # measured once, before the synthesis
    (dn,), (ld,), (lim,) = lib.calls("ev_denoise"), lib.calls("ev_loudness"), lib.calls("ev_limit")
    assert (dn["B"], dn["flags"], dn["lens"], dn["is_i16"], dn["src"], dn["strengths"]) == (3, DEV, LENS, 0, ("synth.wav", 0), None)
    assert abs(dn["cfg"]["strength"] - 0.1) < 1e-7 and dn["cfg"]["want_i16"] == 0      # not the last stage: no int16
    assert ld["src"] == ("denoise.wav", 0) and lim["src"] == ("denoise.wav", 0) and lim["cfg"]["want_i16"] == 1
    assert lib.calls("ev_flac")[0]["src"] == ("limit.wav_i16", 0)
    assert np.all(np.isfinite(out["wav"])) and out["denoise"]["lens_out"].tolist() == LENS and "loudness" in out and "limiter" in out
    # a later call with another setup measures nothing: the kept bias is passed back
    n = len(lib.log)
    eng.synthesize(utterances(), denoise=0.2, want_int16=True)
    assert [e["name"] for e in lib.log[n:] if e["name"] != "ev_memcpy_d2h"] == ["ev_synthesize", "ev_denoise_setup", "ev_denoise"]
    assert lib.calls("ev_denoise_setup")[-1]["bias"] == [0.5] * 513 and lib.calls("ev_denoise_setup")[-1]["cfg"]["want_i16"] == 1


def test_denoise_alone_is_the_last_stage(eng):
    lib = eng.fake
    out = eng.synthesize(utterances(), denoise=DenoiseConfig(strength=0.2, bias=np.full(513, 0.25, np.float32), report=True), want_int16=True, flac=[True, False, True])
    assert "ev_vocoder(zero mel)" not in lib.names() and lib.names()[:3] == ["ev_synthesize", "ev_denoise_setup", "ev_denoise"]
    (st,) = lib.calls("ev_denoise_setup")
    assert st["bias"] == [0.25] * 513 and st["cfg"]["want_i16"] == 1 and abs(st["cfg"]["strength"] - 0.2) < 1e-7
    want = fk.ramp(N) + EIGHTH
    assert np.array_equal(out["wav"], want) and np.array_equal(out["wav_i16"], fk.to_i16(want))
    assert all(np.array_equal(w, want[a:b]) for w, a, b in zip(out["wav_list"], OFFS[:-1], OFFS[1:]))
    (cmp,) = lib.calls("ev_compare")
    assert (cmp["a"], cmp["b"], cmp["lens"], cmp["flags"]) == (("denoise.wav", 0), ("synth.wav", 0), LENS, DEV)
    assert out["denoise"]["removed_db"].tolist() == [-20.0] * 3
    assert [e["src"] for e in lib.calls("ev_flac")] == [("denoise.wav_i16", 0), ("denoise.wav_i16", 2 * int(OFFS[2]))]
    assert out["flac_list"][1] is None and out["flac_list"][0] == b"fLaC" + fk.to_i16(want).tobytes()[:8]


def test_delivery_reads_the_denoised_waveform(eng):
    from emotivoice_amd.delivery import DeliveryConfig
    import test_deliver_chain as tdc

    class Both(DenoiseLib, tdc.DeliverLib):
        pass
    lib = Both()
    lib.log, lib.bufs = eng.fake.log, eng.fake.bufs
    eng._lib = eng.fake = lib
    out = eng.synthesize(utterances(), denoise=DenoiseConfig(bias=np.ones(513, np.float32)), delivery=DeliveryConfig(8000, "s16"))
    (dl,) = lib.calls("ev_deliver")
    assert dl["src"] == ("denoise.wav", 0) and lib.calls("ev_denoise")[0]["cfg"]["want_i16"] == 0
    assert "wav" not in out and "denoise" in out and [e["src"][0] for e in lib.calls("ev_memcpy_d2h")] == ["deliver.data"]


def test_synthesize_long_denoises_after_the_stitch_and_cuts_to_whole_hops(eng, monkeypatch):
    from emotivoice_amd.longform import StitchConfig
    lib = eng.fake
    u = utterances()
    out = eng.synthesize_long([dict(utts=u[:2]), (u[2:], None)], config=StitchConfig(want_int16=True), denoise=DenoiseConfig(bias=np.ones(513, np.float32)), flac=True)
    assert lib.names() == ["ev_synthesize", "ev_stitch", "ev_denoise_setup", "ev_denoise", "ev_flac"]
    (dn,) = lib.calls("ev_denoise")
    assert dn["src"] == ("stitch.wav", 0) and dn["lens"] == [2048, 512] and dn["cfg"]["want_i16"] == 1
    assert lib.calls("ev_flac")[0]["src"] == ("denoise.wav_i16", 0) and lib.calls("ev_flac")[0]["lens"] == [2048, 512]
    want = fk.to_i16(-fk.ramp(N) + EIGHTH)
    assert all(np.array_equal(d, want[a:b]) for d, a, b in zip(out["documents"], (0, 2048), (2048, 2560)))
    assert out["doc_lens"].tolist() == [2048, 512]


def test_without_denoise_the_transcript_is_the_one_of_the_plain_library(monkeypatch):
    """denoise=None, the default, issues exactly the calls it issued before: the stand-in WITHOUT ev_denoise (it would raise on any call of it)
    logs the same entries with the same arguments."""
    logs = []
    for lib in (fk.FakeLib(), DenoiseLib()):
        monkeypatch.setattr(_ffi, "lib", lambda lib=lib: lib)
        from emotivoice_amd.engine import EVEngine
        e = EVEngine()
        e.synthesize(utterances(), loudness=-16.0, limiter=-1.0, want_int16=True, flac=True)
        e.synthesize(utterances(), denoise=None, flac=[True, False, True])
        e.synthesize_long([dict(utts=utterances())], flac=True, denoise=None)
        logs.append([repr(x) for x in lib.log])
        e.close()
    assert logs[0] == logs[1] and not any("denoise" in x for x in logs[1])


def test_serving_passes_denoise_through():
    from emotivoice_amd.serving import engine_flac_synth_fn, engine_prosody_synth_fn, engine_synth_fn

    class Engine:
        def __init__(self):
            self.calls = []

        def synthesize(self, utts, **kw):
            self.calls.append(kw)
            return dict(wav_list=[np.zeros(4, np.float32)] * len(utts), flac_list=[b"fLaC"] * len(utts))
    e = Engine()
    engine_synth_fn(e)([{}], 1.0)
    engine_synth_fn(e, denoise=0.05)([{}], 1.0)
    engine_prosody_synth_fn(e, denoise=DenoiseConfig(0.2))([{}], [None])
    engine_flac_synth_fn(e, denoise=0.05)([{}], 1.0, [True])
    assert "denoise" not in e.calls[0] and e.calls[1]["denoise"].strength == 0.05 and e.calls[2]["denoise"].strength == 0.2 and e.calls[3]["denoise"].strength == 0.05
    with pytest.raises(ValueError):
        engine_synth_fn(e, denoise=-1.0)
