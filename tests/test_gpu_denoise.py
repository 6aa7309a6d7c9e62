"""MI355X: ev_denoise -- STFT, gain, inverse STFT on the device (include/evhip.h).  Each kernel alone against the float64 oracle
(tests/denoise_oracle.py) at one tile, a full tile and a tile boundary; the whole call on every fixture of the reference's own STFT class
(tests/golden/denoise/dn_*.npz) with the reference's float32 error as the yardstick; bit invariance over the batch; the bias the engine measures
itself; the stage in synthesize.  What the card measured goes to denoise_report.json, next to parity_report.json."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import denoise_oracle as do
import features_oracle as fo
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DN_DIR = os.path.join(GOLDEN_DIR, "denoise")
FIXTURES = sorted(glob.glob(os.path.join(DN_DIR, "dn_[a-g]_*.npz")))
FLOOR = 2.0 ** -22           # the truncation class of the split-precision product
FWD_BAR = 4 * FLOOR          # what ev_features holds one such GEMM to
SPEC_BAR = 3 * FWD_BAR + FLOOR      # the gained spectrum: test_op_stft_gain_against_the_oracle says why
REPORT = {}


def _report(key, val):
    """denoise_report.json, next to parity_report.json"""
    from test_gpu_parity import _report as write_report
    write_report(key, val, "denoise_report.json", REPORT)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _signal(n, seed, amp=0.3):
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n) / 16000.0
    return (amp * np.sin(2 * np.pi * (200.0 + 37.0 * seed) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.02 * rng.standard_normal(n)).astype(np.float32)


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    blob, man = pack_state_dict(synth_state_dict(0, "parity"))
    eng = EVEngine(precision="mx")
    eng.load_blob(blob, man)
    gs = {os.path.basename(p)[:-4]: dict(np.load(p)) for p in FIXTURES}
    assert len(gs) == 7
    inv = dict(np.load(os.path.join(DN_DIR, "dn_h_inverse_t9.npz")))
    bar = 4 * max([float(g["ref_err"]) for g in gs.values()] + [float(inv["ref_err"])])
    assert 1e-6 < bar < 1e-5          # the recorded figure: the reference's own float32 error is about 1e-6 of the peak
    yield dict(eng=eng, gs=gs, inv=inv, bar=bar, bias=gs["dn_a_l513"]["bias"])
    eng.close()


def _lib():
    from emotivoice_amd import _ffi
    return _ffi.lib()


def _op_stft_gain(wavs, bias, strengths, n_fft=1024, hop=256, mag=False):
    """ev_op_stft_gain on torch buffers: the recombined spectrum (sum T, k_pad) float64 and the planes, or the magnitudes (sum T, n_bins)."""
    is16 = wavs[0].dtype == np.int16
    lens = np.array([len(w) for w in wavs], np.int64)
    T = int((lens // hop + 1).sum())
    kp = do.k_pad(n_fft)
    d_wav = torch.from_numpy(np.concatenate(wavs)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    if mag:
        d_mag = torch.full((T, n_fft // 2 + 1), float("nan"), device="cuda")
        rc = _lib().ev_op_stft_gain(d_wav.data_ptr(), int(is16), len(wavs), lens.ctypes.data, None, n_fft, hop, None, None, None, None, d_mag.data_ptr(), s)
        assert rc == 0
        return d_mag.cpu().numpy()
    d_bias, d_st = torch.from_numpy(np.asarray(bias, np.float32)).cuda(), torch.from_numpy(np.asarray(strengths, np.float32)).cuda()
    d_hi = torch.full((T, kp), float("nan"), dtype=torch.float16, device="cuda")
    d_lo = torch.full((T, kp), float("nan"), dtype=torch.float16, device="cuda")
    rc = _lib().ev_op_stft_gain(d_wav.data_ptr(), int(is16), len(wavs), lens.ctypes.data, None, n_fft, hop, d_bias.data_ptr(), d_st.data_ptr(),
                                d_hi.data_ptr(), d_lo.data_ptr(), None, s)
    assert rc == 0
    hi, lo = d_hi.cpu().numpy(), d_lo.cpu().numpy()
    return hi.astype(np.float64) + lo.astype(np.float64) / 2048.0, hi, lo


def _op_istft(spec, frames, n_fft=1024, hop=256, want_i16=False):
    """ev_op_istft on the planes of a float spectrum in the scratch layout (sum T, k_pad)."""
    hi, lo = do.split_planes(spec)
    d_hi, d_lo = torch.from_numpy(hi).cuda(), torch.from_numpy(lo).cuda()
    fr = np.asarray(frames, np.int32)
    n = int((hop * (fr - 1)).sum())
    d_out = torch.full((n,), float("nan"), device="cuda")
    d_i16 = torch.zeros(n, dtype=torch.int16, device="cuda") if want_i16 else None
    rc = _lib().ev_op_istft(d_hi.data_ptr(), d_lo.data_ptr(), len(fr), fr.ctypes.data, None, n_fft, hop, d_out.data_ptr(),
                            d_i16.data_ptr() if want_i16 else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return (d_out.cpu().numpy(), d_i16.cpu().numpy()) if want_i16 else d_out.cpu().numpy()


def _spec_error(got, want):
    """max over cells of |got - want| relative to the frame's largest magnitude (a frame of exact silence: relative to 1)."""
    den = np.sqrt(want[:, 0::2] ** 2 + want[:, 1::2] ** 2).max(axis=1, keepdims=True)
    return float((np.abs(got - want) / np.where(den > 0, den, 1.0)).max())


@pytest.mark.parametrize("frames,i16", ((3, False), (64, False), (65, True)))
def test_op_stft_gain_against_the_oracle(ctx, frames, i16):
    """Magnitudes and the gained spectrum (hi + lo / 2048) at the fewest frames an utterance can have (reflect padding needs n_fft / 2 + 1 = 513
    samples, which are 3 frames: one tile), a full tile and a tile boundary.  The magnitudes are held to the forward bar 4 x 2^-22 of the frame's
    largest magnitude M, as ev_features holds them.  The gained cell g x = x - s b x / mag inherits the error of x (one bar), that of the unit
    vector x / mag scaled by s b <= mag (two bars: x and mag), and the 2^-22 of its own hi / lo split: 3 bars + 2^-22; a cell at the floor's
    edge is off by at most the error of mag.  Padding columns are zero."""
    L = (frames - 1) * 256 + 77
    w = _signal(L, frames)
    if i16:
        w = np.clip(np.round(w * 32768.0), -32768, 32767).astype(np.int16)
    wavs = [w, _signal(700, 9) if not i16 else (_signal(700, 9) * 32768).astype(np.int16)]      # a second utterance: rows of another utterance next to the tile
    st = np.array([0.1, 2.0], np.float32)
    re, im = zip(*(do.stft64(x) for x in wavs))
    mag = _op_stft_gain(wavs, None, None, mag=True)
    mag64 = np.sqrt(np.concatenate(re) ** 2 + np.concatenate(im) ** 2)
    e_mag = fo.mag_error(mag, mag64)
    spec, hi, lo = _op_stft_gain(wavs, ctx["bias"], st)
    want = np.concatenate([do.pack_spectrum(*do.gain64(r, i, ctx["bias"], s)[:2]) for r, i, s in zip(re, im, st)]).astype(np.float64)
    assert spec.shape == want.shape == (frames + 3, 1056)
    e_spec = _spec_error(spec, want)
    _report("op_stft_gain/T%d%s" % (frames, "_i16" if i16 else ""), dict(e_mag=e_mag, e_spec=e_spec, bar_mag=FWD_BAR, bar_spec=SPEC_BAR))
    print("frames", frames, "E(mag)", e_mag, "E(spec)", e_spec)
    assert e_mag <= FWD_BAR and e_spec <= SPEC_BAR
    assert np.all(hi[:, 1026:] == 0) and np.all(lo[:, 1026:] == 0)
    assert np.all(np.isfinite(hi)) and np.all(np.isfinite(lo))


def test_op_stft_gain_other_shape(ctx):
    """n_fft = 512, hop = 128."""
    w = _signal(5000, 4)
    bias = np.abs(np.random.default_rng(5).standard_normal(257)).astype(np.float32) * 0.05
    re, im = do.stft64(w, 512, 128)
    spec, hi, _ = _op_stft_gain([w], bias, np.array([0.5], np.float32), 512, 128)
    want = do.pack_spectrum(*do.gain64(re, im, bias, 0.5)[:2], n_fft=512).astype(np.float64)
    e = _spec_error(spec, want)
    _report("op_stft_gain/512_128", dict(e_spec=e, bar=SPEC_BAR))
    assert spec.shape == want.shape == (40, 544) and e <= SPEC_BAR


@pytest.mark.parametrize("frames", (3, 64, 65, 130))
def test_op_istft_against_the_oracle(ctx, frames):
    """The inverse alone, on the oracle's own spectrum: E <= the bar of the whole call.  Two utterances, so that rows of a neighbour lie next to
    every edge; the int16 is the clamping rule applied to the fp32 output exactly."""
    specs, want = [], []
    for T in (frames, 3):
        re, im = do.stft64(_signal((T - 1) * 256 + 5, T, amp=0.9))
        gre, gim, _ = do.gain64(re, im, ctx["bias"], 1.0)
        gre, gim = gre.astype(np.float32), gim.astype(np.float32)
        specs.append(do.pack_spectrum(gre, gim))
        want.append(do.istft64(gre.astype(np.float64), gim.astype(np.float64)))
    out, i16 = _op_istft(np.concatenate(specs), [frames, 3], want_i16=True)
    n0 = 256 * (frames - 1)
    e = max(do.peak_error(out[:n0], want[0]), do.peak_error(out[n0:], want[1]))
    _report("op_istft/T%d" % frames, dict(e=e, bar=ctx["bar"]))
    print("frames", frames, "E", e)
    assert out.size == n0 + 512 and e <= ctx["bar"]
    assert np.array_equal(i16, do.to_i16(out))


def test_op_istft_reference_inverse_and_other_shape(ctx):
    """The inverse-only fixture (the reference's STFT.inverse on a spectrum with Im[0] = Im[n_fft / 2] = 0), and n_fft = 512, hop = 128."""
    g = ctx["inv"]
    want = do.istft64(g["re"].astype(np.float64), g["im"].astype(np.float64))
    out = _op_istft(do.pack_spectrum(g["re"], g["im"]), [9])
    e, e_ref = do.peak_error(out, want), do.peak_error(g["ref_out"], want)
    _report("op_istft/reference_inverse", dict(e=e, e_ref=e_ref, bar=ctx["bar"]))
    assert e <= ctx["bar"]
    re, im = do.stft64(_signal(3000, 8), 512, 128)
    re, im = re.astype(np.float32), im.astype(np.float32)
    out = _op_istft(do.pack_spectrum(re, im, 512), [re.shape[0]], 512, 128)
    e = do.peak_error(out, do.istft64(re.astype(np.float64), im.astype(np.float64), 512, 128))
    _report("op_istft/512_128", dict(e=e, bar=ctx["bar"]))
    assert out.size == 128 * (re.shape[0] - 1) and e <= ctx["bar"]


def _fixture_errors(ctx, oracle):
    """E per fixture of ev_denoise against ``oracle(wav, bias, strength)``."""
    eng, errs = ctx["eng"], {}
    for name, g in ctx["gs"].items():
        from emotivoice_amd.denoise import DenoiseConfig
        out = eng.denoise([g["wav"]], DenoiseConfig(strength=float(g["strength"]), bias=g["bias"]))
        y = out["wav_list"][0]
        assert y.size == 256 * (g["wav"].size // 256) == out["lens_out"][0] == g["ref_out"].size
        errs[name] = do.peak_error(y, oracle(g["wav"], g["bias"], float(g["strength"])))
    return errs


def test_denoise_on_every_fixture_against_the_float64_oracle(ctx):
    """E = max |y - y64| / max |y64| per utterance <= 4 x the largest E the reference's own float32 run shows over the fixtures (recorded by the
    generator: 9.6e-7, so the bar is 3.8e-6)."""
    errs = _fixture_errors(ctx, do.denoise64)
    for name, e in errs.items():
        _report("denoise/" + name, dict(e=e, e_ref=float(ctx["gs"][name]["ref_err"]), bar=ctx["bar"]))
        print(name, "E(dev) %.3e E(ref) %.3e bar %.3e" % (e, float(ctx["gs"][name]["ref_err"]), ctx["bar"]))
    assert all(e <= ctx["bar"] for e in errs.values()), errs


def test_negative_control_the_bar_sees_wrong_inverse_weights(ctx):
    """The same comparison against the oracle with every inverse weight c_k = 2 must fail on every fixture: the bar sees an error of that size."""
    errs = _fixture_errors(ctx, lambda w, b, s: do.denoise64(w, b, s, all_two=True))
    print(errs)
    assert all(e > ctx["bar"] for e in errs.values()), errs


def test_strength_zero_is_the_identity_and_int16_is_the_clamping_rule(ctx):
    from emotivoice_amd.denoise import DenoiseConfig
    eng = ctx["eng"]
    wavs = [ctx["gs"]["dn_c_l20011"]["wav"], ctx["gs"]["dn_a_l513"]["wav"], _signal(4096, 3, amp=1.4)]      # the last one clips
    out = eng.denoise(wavs, DenoiseConfig(strength=0.0, bias=ctx["bias"], want_int16=True))
    assert out["lens_out"].tolist() == [19968, 512, 4096]
    for y, w in zip(out["wav_list"], wavs):
        e = do.peak_error(y, w[:y.size])
        assert e <= ctx["bar"], e
    assert np.array_equal(out["wav_i16"], do.to_i16(out["wav"]))
    assert out["wav_i16"].max() == 32767 and out["wav_i16"].min() == -32768


def test_batch_independence_bit_for_bit(ctx):
    """An utterance alone, first, last and in the middle of a batch of five with mixed lengths and per-utterance strengths; int16 input equals
    the equal floats; device input equals host input."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.denoise import DenoiseConfig
    eng = ctx["eng"]
    cfg = DenoiseConfig(strength=0.3, bias=ctx["bias"])
    a = ctx["gs"]["dn_c_l20011"]["wav"]
    alone = eng.denoise([a], cfg, strengths=[0.7])["wav_list"][0].copy()
    others = [_signal(513, 1), _signal(16640, 2), _signal(3000, 3), _signal(777, 4)]
    for pos in (0, 2, 4):
        batch = others[:pos] + [a] + others[pos:]
        st = [0.1 * (i + 1) for i in range(5)]
        st[pos] = 0.7
        out = eng.denoise(batch, cfg, strengths=st)
        assert np.array_equal(_bits(out["wav_list"][pos]), _bits(alone)), pos
    i16 = ctx["gs"]["dn_d_l20011_i16"]["wav"]
    yi = eng.denoise([i16], cfg)["wav_list"][0].copy()
    yf = eng.denoise([i16.astype(np.float32) / np.float32(32768.0)], cfg)["wav_list"][0]
    assert np.array_equal(_bits(yi), _bits(yf))
    flat = torch.from_numpy(np.concatenate([a, others[0]])).cuda()
    torch.cuda.synchronize()
    res = eng.denoise_raw(2, flat.data_ptr(), False, np.array([a.size, 513], np.int64), [0.7, 0.2], _ffi.EV_FLAG_DEVICE_INPUTS)
    assert np.array_equal(_bits(eng.denoise_to_numpy(res)["wav_list"][0]), _bits(alone))


def test_rejections(ctx):
    from emotivoice_amd.denoise import DenoiseConfig
    from emotivoice_amd.engine import EVError
    eng = ctx["eng"]
    eng.denoise_setup(DenoiseConfig(bias=ctx["bias"]))
    short = np.zeros(512, np.float32)
    with pytest.raises(EVError, match="n_fft / 2"):
        eng.denoise_raw(1, short.ctypes.data, False, [512])
    ok = _signal(2048, 1)
    with pytest.raises(EVError, match="strengths"):
        eng.denoise_raw(1, ok.ctypes.data, False, [2048], [-1.0])
    from emotivoice_amd import _ffi
    c = _ffi.ev_denoise_config()
    eng._lib.ev_default_denoise_config(C.byref(c))
    assert (c.n_fft, c.hop, c.want_i16, c.window) == (1024, 256, 0, None) and abs(c.strength - 0.01) < 1e-9
    c.hop = 96
    assert eng._lib.ev_denoise_setup(eng._h, C.byref(c), ctx["bias"].ctypes.data) != 0 and b"hop" in eng._lib.ev_last_error(eng._h)
    c.hop, c.n_fft = 64, 1024      # R = 16
    assert eng._lib.ev_denoise_setup(eng._h, C.byref(c), ctx["bias"].ctypes.data) != 0
    # a rejected setup leaves the previous one in place
    assert eng.denoise([ok], DenoiseConfig(bias=ctx["bias"]))["lens_out"].tolist() == [2048]


def test_setup_measures_the_vocoders_own_bias(ctx):
    """ev_denoise_setup(bias = NULL): the captured bias is the oracle's magnitudes of frame 0 of ev_vocoder's own answer to a zero mel of 88
    frames, within the forward bar; ev_denoise_bias round-trips through setup(bias = ...) bit for bit."""
    from emotivoice_amd.denoise import BIAS_FRAMES, DenoiseConfig
    eng = ctx["eng"]
    eng.denoise_setup(DenoiseConfig(strength=0.1))
    got = eng.denoise_bias()
    zero = eng.vocoder([np.zeros((eng.shapes.n_mels, BIAS_FRAMES), np.float32)])["wav"]
    assert zero.size == BIAS_FRAMES * 256
    re, im = do.stft64(zero)
    mag64 = np.sqrt(re * re + im * im)[:1]
    e = fo.mag_error(got[None, :], mag64)
    _report("setup/own_bias", dict(e=e, bar=FWD_BAR, peak=float(mag64.max())))
    assert got.shape == (513,) and np.all(np.isfinite(got)) and got.max() > 0 and e <= FWD_BAR
    w = _signal(4000, 2)
    y0 = eng.denoise([w], DenoiseConfig(strength=0.1))["wav_list"][0].copy()
    eng.denoise_setup(DenoiseConfig(strength=0.1, bias=got))
    assert np.array_equal(_bits(eng.denoise_bias()), _bits(got))
    y1 = eng.denoise([w], DenoiseConfig(strength=0.1, bias=got))["wav_list"][0]
    assert np.array_equal(_bits(y0), _bits(y1))


def test_synthesize_with_denoise_equals_denoise_of_synthesize(ctx):
    """synthesize(utts, denoise=0.1) equals engine.denoise(synthesize(utts)["wav_list"], 0.1) bit for bit; the stage runs before loudness; the
    report is ev_compare's."""
    from emotivoice_amd.denoise import DenoiseConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 17], [3, 8])
    plain = eng.synthesize(utts)
    want = eng.denoise(plain["wav_list"], 0.1)
    out = eng.synthesize(utts, denoise=dict(strength=0.1, report=True), want_int16=True, flac=True)
    assert out["denoise"]["lens_out"].tolist() == [w.size for w in plain["wav_list"]]
    for b in range(2):
        assert np.array_equal(_bits(out["wav_list"][b]), _bits(want["wav_list"][b]))
    assert np.array_equal(out["wav_i16"], do.to_i16(out["wav"])) and all(s[:4] == b"fLaC" for s in out["flac_list"])
    d = np.concatenate(plain["wav_list"]).astype(np.float64) - out["wav"].astype(np.float64)
    offs = np.concatenate([[0], np.cumsum([w.size for w in plain["wav_list"]])])
    db = [10 * np.log10((d[a:b] ** 2).sum() / (np.concatenate(plain["wav_list"]).astype(np.float64)[a:b] ** 2).sum()) for a, b in zip(offs[:-1], offs[1:])]
    assert np.allclose(out["denoise"]["removed_db"], db, atol=1e-6), (out["denoise"]["removed_db"], db)
    # before loudness: the loudness stage reads the denoised waveform
    both = eng.synthesize(utts, denoise=DenoiseConfig(strength=0.1), loudness=-20.0)
    alone = eng.loudness(want["wav_list"], target_lufs=-20.0)
    for b in range(2):
        assert np.array_equal(_bits(both["wav_list"][b]), _bits(alone["wav_list"][b]))
    # and without denoise= nothing changed
    again = eng.synthesize(utts)
    assert np.array_equal(_bits(again["wav"]), _bits(plain["wav"]))
