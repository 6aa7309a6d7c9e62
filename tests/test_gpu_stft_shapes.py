"""MI355X: the windowed-DFT kernels (stft_mel_kernel, stft_gain_kernel, istft_ola_kernel; the shared parts of ev_audio_dev.h) over the shape classes
their launchers accept, with windows that are not symmetric, at quiet and loud levels, and with non-finite samples.  Everything goes through
ev_op_stft_mel, ev_op_stft_gain (both modes) and ev_op_istft on guard-banded buffers, and once each through EVEngine.features / EVEngine.denoise.

Shape table (n_fft / hop; every case is a batch of two, the second utterance n_fft / 2 + 1 samples long):
  128 / 8      the minimum hop; R = 16, so both ev_denoise entry points answer -2
  128 / 128    R = 1: with a hann window the envelope is 0 at the first sample of every chunk; the short utterance has one frame and no output
  384 / 48     n_fft not a power of two, R = 8, a partial column block (hop < 128), an utterance with fewer frames than R
  640 / 320    R = 2, three column blocks, the last one partial and clamped
  2048 / 352   the largest run a tile may hold (about 106 KB of LDS); 352 does not divide 2048: -2 from ev_denoise's entry points
  2048 / 256   R = 8 at the largest n_fft: the longest k loop
Windows: None (periodic hann), A = float32(hann * linspace(0.2, 1, n)) -- asymmetric, so that a reversed or shifted window index shows -- and
B = A with a run of exact zeros, which puts zeros of the envelope inside chunks.  Every case with A or B also shows on the CPU that the oracle
with the reversed window is more than 0.1 away: the case can see a flip.

Bars.  None comes from the device.  Forward: E <= 4 max(E32, 2^-22), E32 = the error of a plain float32 numpy evaluation of the same operation
against the same float64 oracle, computed here; 2^-22 is the truncation class of the split product.  Gained planes: 3 forward bars + 2^-22
(tests/test_gpu_denoise.py says why).  Inverse: E <= 4 max(E32_inv, ref_err), ref_err = what the reference's own float32 STFT class shows at that
shape (tests/golden/denoise), where a fixture exists (not at 2048 / 256).  At 128 / 128 a lone hann^2 divides by as little as 3.6e-7 next to a
chunk edge, which multiplies every float32 error: the reference's own run is 1.6e-4 off there, and that is the yardstick.
Every figure and its bar goes to features_report.json / denoise_report.json.

Measured on an MI355X (worst over the cases of a family / the bar of that case):
  table, ev_op_stft_mel     mel 5.5e-7 / 1.8e-6    energy 3.6e-7 / 9.5e-7    mag 6.3e-7 / 1.8e-6   (2048 / 256 and 2048 / 352)
  table, ev_op_stft_gain    mag 6.3e-7 / 1.8e-6    planes 6.8e-7 / 5.5e-6                          (2048 / 256, hann, 9 frames)
  table, ev_op_istft        1.25e-6 / 1.53e-6 (2048 / 256, window A, 9 frames); 128 / 128: 4.0e-7 / 6.6e-4
  windows                   forward A at 1024 / 256: mag 4.8e-7 / 2.0e-6; inverse B at 128 / 128: 2.7e-6 / 6.6e-4
  peak 2^-12                mag 6.1e-7 / 1.5e-6    planes 5.9e-7 / 4.8e-6    inverse 3.7e-7 / 3.8e-6: the matrix cores keep fp16 subnormal operands
                            (a numpy emulation with subnormals flushed gives 7e-2)
  peak 8.0                  mag 4.3e-7 / 1.5e-6    planes 5.6e-7 / 4.8e-6    inverse 4.8e-7 / 3.8e-6
  int16 +-2 LSB             mag 2.2e-7 / 2.4e-6    planes 3.2e-7 / 7.4e-6    inverse 4.7e-7 / 3.8e-6
  peak 2^-16 (no bar)       mag 9.3e-7             planes 9.4e-7             inverse 4.8e-7
  NaN, +inf                 planes 4.5e-7 / 7.0e-6, output 1.1e-6 / 3.8e-6, no non-finite value anywhere; with the cell rule as a product (g * Re, g = 0)
                            all 8448 plane values of the four frames (4 x 1056 x 2) were NaN, and with them every output sample those frames reach
  public calls, window A    EVEngine.features: mag 4.8e-7 / 2.2e-6; EVEngine.denoise: 1.1e-6 / 3.8e-6
"""
import glob
import os

import numpy as np
import pytest

import denoise_oracle as do
import features_oracle as fo
import test_gpu_denoise as tgd
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLOOR = 2.0 ** -22
DN_DIR = os.path.join(GOLDEN_DIR, "denoise")
FEAT_REPORT = {}
# n_fft, hop, frames of utterance 0, ev_denoise takes the shape
TABLE = ((128, 8, (65, 130), False), (128, 128, (3, 65), True), (384, 48, (5, 64, 65), True), (640, 320, (2, 65), True), (2048, 352, (65,), False),
         (2048, 256, (9, 65), True))
TABLE_IDS = ["%d_%d" % t[:2] for t in TABLE]


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rep_f(key, val):
    from test_gpu_parity import _report
    _report(key, val, "features_report.json", FEAT_REPORT)


def _rep_d(key, val):
    tgd._report(key, val)      # the one dictionary behind denoise_report.json


def _lib():
    from emotivoice_amd import _ffi
    return _ffi.lib()


def window_of(name, n_fft, hop):
    """None, A or B (module docstring)."""
    if name == "hann":
        return None
    a = ((0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)) * np.linspace(0.2, 1.0, n_fft)).astype(np.float32)
    if name == "B":
        a[n_fft // 4:n_fft // 4 + hop // 2] = 0.0
    return a


def _wav_len(T, n_fft, hop):
    L = (T - 1) * hop + 5
    assert L >= n_fft // 2 + 1 and L // hop + 1 == T
    return L


def _sig(n, seed, n_fft, amp=0.3):
    """A tone plus noise, peak ``amp``, under a sawtooth envelope of period n_fft / 1.7 samples: a stationary tone has the same magnitudes under a
    window and under its mirror image, so the signal must change inside a frame for a reversed window to show."""
    rng = np.random.default_rng(1000 + seed)
    i = np.arange(n)
    x = np.sin(2 * np.pi * (200.0 + 37.0 * seed) * i / 16000.0) * (0.15 + 0.85 * ((i * 1.7 / n_fft) % 1.0)) + 0.05 * rng.standard_normal(n)
    return (x / np.abs(x).max() * amp).astype(np.float32)


def _pair(T, n_fft, hop, seed, amp=0.3):
    """utterance 0 of T frames and the shortest legal utterance"""
    return [_sig(_wav_len(T, n_fft, hop), seed, n_fft, amp), _sig(n_fft // 2 + 1, seed + 50, n_fft, amp)]


def _bias(n_fft, scale=1.0):
    return (np.abs(np.random.default_rng(5 + n_fft).standard_normal(n_fft // 2 + 1)) * 0.05 * scale).astype(np.float32)


def _inverse_ref_err(n_fft, hop):
    """the reference's own float32 error at this shape, where a fixture records one"""
    if (n_fft, hop) == (1024, 256):
        return max(float(np.load(p)["ref_err"]) for p in glob.glob(os.path.join(DN_DIR, "dn_[a-h]_*.npz")))
    p = os.path.join(DN_DIR, "dn_shape_%d_%d.npz" % (n_fft, hop))
    return float(np.load(p)["ref_err"]) if os.path.exists(p) else 0.0


# ---------------------------------------------------------------- the float32 yardsticks, on the CPU
def _frames32(wav, n_fft, hop):
    x = fo.to_float(wav)
    padded = np.pad(x, n_fft // 2, mode="reflect")
    return np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(padded, n_fft)[::hop][:x.size // hop + 1])


def _forward32(wav, mb, n_fft, hop, window):
    """features_oracle.features64 in plain float32: (mag, mel, energy)"""
    fr = _frames32(wav, n_fft, hop)
    re_b, im_b = fo.basis_f32(n_fft, window)
    re, im = fr @ re_b.T, fr @ im_b.T
    mag = np.sqrt(re * re + im * im)
    assert mag.dtype == np.float32
    if mb is None:
        return mag, None, None
    mel = np.log(np.maximum(np.asarray(mb, np.float32) @ mag.T, np.float32(1e-5)))
    return mag, mel, np.sqrt(np.maximum((mag * mag).sum(axis=1, dtype=np.float32), np.float32(1e-10)))


def _istft32(gre, gim, n_fft, hop, window):
    """denoise_oracle.istft64 in plain float32"""
    T = gre.shape[0]
    cb, sb = do.inverse_basis_f32(n_fft, window)
    fr = np.asarray(gre, np.float32) @ cb + np.asarray(gim, np.float32) @ sb
    u = np.zeros(n_fft + hop * (T - 1), np.float32)
    for t in range(T):
        u[t * hop:t * hop + n_fft] += fr[t]
    y = u * np.float32(1.0 / n_fft)
    env = do.envelope_f32(T, n_fft, hop, window)
    ok = env > do.TINY
    y[ok] = y[ok] / env[ok]
    assert y.dtype == np.float32
    return y[n_fft // 2:n_fft // 2 + hop * (T - 1)]


# ---------------------------------------------------------------- the entry points, on guard-banded buffers
def _wp(window):
    return None if window is None else np.ascontiguousarray(window, np.float32).ctypes.data


def _gain(wavs, bias, strengths, n_fft, hop, window=None, mag=False, expect=0):
    """ev_op_stft_gain: the magnitudes (sum T, n_bins), or the planes (hi, lo) (sum T, k_pad).  Two rows past the end stay as they were filled."""
    is16 = wavs[0].dtype == np.int16
    lens = np.array([len(w) for w in wavs], np.int64)
    T, kp, nb = int((lens // hop + 1).sum()), do.k_pad(n_fft), n_fft // 2 + 1
    d_wav = torch.from_numpy(np.concatenate(wavs)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    win = None if window is None else np.ascontiguousarray(window, np.float32)
    if mag:
        d_mag = torch.full((T + 2, nb), float("nan"), device="cuda")
        rc = _lib().ev_op_stft_gain(d_wav.data_ptr(), int(is16), len(wavs), lens.ctypes.data, _wp(win), n_fft, hop, None, None, None, None, d_mag.data_ptr(), s)
        assert rc == expect
        m = d_mag.cpu().numpy()
        assert np.isnan(m[T:]).all() and (not expect or np.isnan(m).all())
        return m[:T]
    d_bias, d_st = torch.from_numpy(np.asarray(bias, np.float32)).cuda(), torch.from_numpy(np.asarray(strengths, np.float32)).cuda()
    d_hi = torch.full((T + 2, kp), float("nan"), dtype=torch.float16, device="cuda")
    d_lo = torch.full((T + 2, kp), float("nan"), dtype=torch.float16, device="cuda")
    rc = _lib().ev_op_stft_gain(d_wav.data_ptr(), int(is16), len(wavs), lens.ctypes.data, _wp(win), n_fft, hop, d_bias.data_ptr(), d_st.data_ptr(),
                                d_hi.data_ptr(), d_lo.data_ptr(), None, s)
    assert rc == expect
    hi, lo = d_hi.cpu().numpy(), d_lo.cpu().numpy()
    assert np.isnan(hi[T:]).all() and np.isnan(lo[T:]).all()
    if expect:
        assert np.isnan(hi).all() and np.isnan(lo).all()
    return hi[:T], lo[:T]


def _istft(hi, lo, frames, n_fft, hop, window=None, expect=0):
    """ev_op_istft on planes (sum T, k_pad): (out fp32, out int16); 64 elements past the end stay as they were filled."""
    d_hi, d_lo = torch.from_numpy(np.ascontiguousarray(hi)).cuda(), torch.from_numpy(np.ascontiguousarray(lo)).cuda()
    fr = np.asarray(frames, np.int32)
    n = int((hop * (fr - 1)).sum())
    d_out = torch.full((n + 64,), float("nan"), device="cuda")
    d_i16 = torch.full((n + 64,), 12345, dtype=torch.int16, device="cuda")
    win = None if window is None else np.ascontiguousarray(window, np.float32)
    rc = _lib().ev_op_istft(d_hi.data_ptr(), d_lo.data_ptr(), len(fr), fr.ctypes.data, _wp(win), n_fft, hop, d_out.data_ptr(), d_i16.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    assert rc == expect
    out, i16 = d_out.cpu().numpy(), d_i16.cpu().numpy()
    assert np.isnan(out[n:]).all() and (i16[n:] == 12345).all()
    if expect:
        assert np.isnan(out).all()
    return out[:n], i16[:n]


def _planes64(hi, lo):
    return hi.astype(np.float64) + lo.astype(np.float64) / 2048.0


def _oracle_spectrum(wav, bias, strength, n_fft, hop, window):
    """the oracle's gained spectrum as the float32 values a scratch would hold: (gre, gim) float32"""
    re, im = do.stft64(wav, n_fft, hop, window)
    gre, gim, _ = do.gain64(re, im, bias, strength)
    return gre.astype(np.float32), gim.astype(np.float32)


def _check_forward_gain(tag, wavs, n_fft, hop, wname, bias, strengths=(0.1, 2.0), check=True):
    """ev_op_stft_gain in both modes on one batch against the oracle: (e_mag, bar_mag, e_spec, bar_spec), reported under ``tag``."""
    window = window_of(wname, n_fft, hop)
    nb = n_fft // 2 + 1
    re, im = zip(*(do.stft64(w, n_fft, hop, window) for w in wavs))
    mag64 = np.sqrt(np.concatenate(re) ** 2 + np.concatenate(im) ** 2)
    e32 = fo.mag_error(np.concatenate([_forward32(w, None, n_fft, hop, window)[0] for w in wavs]), mag64)
    bar_mag = 4 * max(e32, FLOOR)
    bar_spec = 3 * bar_mag + FLOOR
    mag = _gain(wavs, None, None, n_fft, hop, window, mag=True)
    e_mag = fo.mag_error(mag, mag64)
    hi, lo = _gain(wavs, bias, strengths, n_fft, hop, window)
    want = np.concatenate([do.pack_spectrum(*do.gain64(r, i, bias, s)[:2], n_fft=n_fft) for r, i, s in zip(re, im, strengths)]).astype(np.float64)
    assert hi.shape == lo.shape == want.shape
    e_spec = tgd._spec_error(_planes64(hi, lo), want)
    _rep_d(tag, dict(e_mag=e_mag, e32_mag=e32, bar_mag=bar_mag if check else None, e_spec=e_spec, bar_spec=bar_spec if check else None))
    print(tag, "E(mag) %.3e E32 %.3e bar %.3e | E(spec) %.3e bar %.3e" % (e_mag, e32, bar_mag, e_spec, bar_spec))
    assert np.all(np.isfinite(hi)) and np.all(np.isfinite(lo))
    assert np.all(hi[:, 2 * nb:] == 0) and np.all(lo[:, 2 * nb:] == 0)
    if check:
        assert e_mag <= bar_mag and e_spec <= bar_spec, tag
    return e_mag, bar_mag, e_spec, bar_spec


def _check_inverse(tag, wavs, n_fft, hop, wname, check=True, alone=True):
    """ev_op_istft on the oracle's own float32 spectrum of ``wavs`` against istft64: (the worst E over the utterances, its bar, how far the oracle
    with the reversed window is from the oracle).  The spectrum is gained at strength 1 with a bias at the 0.9 quantile of utterance 0's own
    magnitudes per bin: an STFT left as it is comes back as the signal times a smooth factor within 8 % of 1 under ANY window pair at R >= 4, so
    only a spectrum the gain has thinned out shows a reversed window by more than 0.1."""
    window = window_of(wname, n_fft, hop)
    re0, im0 = do.stft64(wavs[0], n_fft, hop, window)
    bias = np.quantile(np.sqrt(re0 * re0 + im0 * im0), 0.9, axis=0).astype(np.float32)
    specs, want, y32, frames, flip = [], [], [], [], 0.0
    for w in wavs:
        gre, gim = _oracle_spectrum(w, bias, 1.0, n_fft, hop, window)
        specs.append(do.pack_spectrum(gre, gim, n_fft))
        want.append(do.istft64(gre.astype(np.float64), gim.astype(np.float64), n_fft, hop, window))
        y32.append(_istft32(gre, gim, n_fft, hop, window))
        frames.append(gre.shape[0])
    hi, lo = do.split_planes(np.concatenate(specs))
    out, i16 = _istft(hi, lo, frames, n_fft, hop, window)
    offs = np.concatenate([[0], np.cumsum([hop * (T - 1) for T in frames])])
    assert out.size == offs[-1]
    e = max(do.peak_error(out[a:b], y) for a, b, y in zip(offs[:-1], offs[1:], want))
    e32 = max(do.peak_error(y, y64) for y, y64 in zip(y32, want))
    bar = 4 * max(e32, _inverse_ref_err(n_fft, hop))
    _rep_d(tag, dict(e=e, e32=e32, ref_err=_inverse_ref_err(n_fft, hop), bar=bar if check else None))
    print(tag, "E %.3e E32 %.3e ref_err %.3e bar %.3e" % (e, e32, _inverse_ref_err(n_fft, hop), bar))
    assert np.all(np.isfinite(out)) and np.array_equal(i16, do.to_i16(out))
    if check:
        assert e <= bar, tag
    if wname != "hann":      # how far a reversed window is
        nb2 = 2 * (n_fft // 2 + 1)
        flip = do.peak_error(do.istft64(specs[0][:, 0:nb2:2].astype(np.float64), specs[0][:, 1:nb2:2].astype(np.float64), n_fft, hop,
                                        np.ascontiguousarray(window[::-1])), want[0])
    if alone:                # utterance 0 alone: the same bits
        T0 = frames[0]
        one, _ = _istft(hi[:T0], lo[:T0], [T0], n_fft, hop, window)
        assert np.array_equal(tgd._bits(one), tgd._bits(out[:offs[1]])), tag
    return e, bar, flip


# ---------------------------------------------------------------- 1, 2: the shape table, with the hann window and with window A
@pytest.mark.parametrize("wname", ("hann", "A"))
@pytest.mark.parametrize("n_fft,hop,frames,denoise_ok", TABLE, ids=TABLE_IDS)
def test_table_forward(n_fft, hop, frames, denoise_ok, wname):
    """ev_op_stft_mel (mel, energy, mag) and ev_op_stft_gain (magnitudes; planes) at one shape, every frame count of the table."""
    from test_gpu_features import _op
    from emotivoice_amd.features import mel_filterbank
    window = window_of(wname, n_fft, hop)
    flips = []      # how far the oracle with the reversed window is from the oracle, utterance 0 of every frame count
    for n_mels in ((20,) if n_fft == 128 else (128, 80) if hop == 352 else (80,)):
        mb = mel_filterbank(16000, n_fft, n_mels, 0.0, 8000.0)
        for T in frames:
            wavs = _pair(T, n_fft, hop, T)
            outs = _op(wavs, mb, n_fft, hop, window=window)
            assert [o[2].shape[0] for o in outs] == [T, (n_fft // 2 + 1) // hop + 1]
            for b, (w, (mel, en, mag)) in enumerate(zip(wavs, outs)):
                o = fo.features64(w, mb, n_fft=n_fft, hop=hop, window=window)
                m32, l32, e32 = _forward32(w, mb, n_fft, hop, window)
                rows = {}
                for what, e_dev, e_f32 in (("mel", fo.mel_error(mel, o["mel"]), fo.mel_error(l32, o["mel"])),
                                           ("energy", fo.energy_error(en, o["energy"]), fo.energy_error(e32, o["energy"])),
                                           ("mag", fo.mag_error(mag, o["mag"]), fo.mag_error(m32, o["mag"]))):
                    rows[what] = dict(e=e_dev, e32=e_f32, bar=4 * max(e_f32, FLOOR))
                tag = "table/stft_mel/%d_%d/%s/m%d/T%d/u%d" % (n_fft, hop, wname, n_mels, T, b)
                _rep_f(tag, rows)
                print(tag, " | ".join("%s E %.3e E32 %.3e" % (k, v["e"], v["e32"]) for k, v in rows.items()))
                assert mel.shape == o["mel"].shape and all(v["e"] <= v["bar"] for v in rows.values()), (tag, rows)
                if wname != "hann" and b == 0:
                    flips.append(fo.mag_error(fo.features64(w, mb, n_fft=n_fft, hop=hop, window=window[::-1])["mag"], o["mag"]))
    if wname != "hann":      # the case can see a flip (an utterance of two frames is mostly its own reflection and shows less: the longer one counts)
        print("reversed window:", flips)
        assert max(flips) > 0.1, flips
    for T in frames:
        wavs = _pair(T, n_fft, hop, T)
        if denoise_ok:
            _check_forward_gain("table/stft_gain/%d_%d/%s/T%d" % (n_fft, hop, wname, T), wavs, n_fft, hop, wname, _bias(n_fft))
        else:      # R = 16, or a hop that does not divide n_fft: rejected before anything is launched, nothing written
            _gain(wavs, None, None, n_fft, hop, window, mag=True, expect=-2)
            _gain(wavs, _bias(n_fft), (0.1, 2.0), n_fft, hop, window, expect=-2)


@pytest.mark.parametrize("wname", ("hann", "A"))
@pytest.mark.parametrize("n_fft,hop,frames,denoise_ok", TABLE, ids=TABLE_IDS)
def test_table_inverse(n_fft, hop, frames, denoise_ok, wname):
    """ev_op_istft at one shape, every frame count of the table (65 frames: a second chunk tile), the int16 rule exactly."""
    if not denoise_ok:
        kp = do.k_pad(n_fft)
        z = np.zeros((frames[0], kp), np.float16)
        _istft(z, z, [frames[0]], n_fft, hop, window_of(wname, n_fft, hop), expect=-2)
        return
    flips = [_check_inverse("table/istft/%d_%d/%s/T%d" % (n_fft, hop, wname, T), _pair(T, n_fft, hop, T, amp=0.9), n_fft, hop, wname)[2] for T in frames]
    if wname != "hann":
        print("reversed window:", flips)
        assert min(flips) > 0.1, flips


def test_windows_at_the_default_shape():
    """Window A through the forward entry points and window B through the inverse at 1024 / 256; window B at 128 / 128, where its zeros and the
    zeros of a lone window's envelope lie inside every chunk."""
    from test_gpu_features import _op
    from emotivoice_amd.features import mel_filterbank
    mb = mel_filterbank()
    A = window_of("A", 1024, 256)
    for T in (3, 65):
        wavs = _pair(T, 1024, 256, T)
        for b, (w, (mel, en, mag)) in enumerate(zip(wavs, _op(wavs, mb, 1024, 256, window=A))):
            o = fo.features64(w, mb, window=A)
            m32, l32, e32 = _forward32(w, mb, 1024, 256, A)
            rows = dict(mel=(fo.mel_error(mel, o["mel"]), fo.mel_error(l32, o["mel"])), energy=(fo.energy_error(en, o["energy"]), fo.energy_error(e32, o["energy"])),
                        mag=(fo.mag_error(mag, o["mag"]), fo.mag_error(m32, o["mag"])))
            _rep_f("window/stft_mel/1024_256/A/T%d/u%d" % (T, b), {k: dict(e=v[0], e32=v[1], bar=4 * max(v[1], FLOOR)) for k, v in rows.items()})
            assert all(v[0] <= 4 * max(v[1], FLOOR) for v in rows.values()), (T, b, rows)
            assert fo.mag_error(fo.features64(w, mb, window=A[::-1])["mag"], o["mag"]) > 0.1
        _check_forward_gain("window/stft_gain/1024_256/A/T%d" % T, wavs, 1024, 256, "A", _bias(1024))
        for wname in ("A", "B"):
            assert _check_inverse("window/istft/1024_256/%s/T%d" % (wname, T), _pair(T, 1024, 256, T, amp=0.9), 1024, 256, wname)[2] > 0.1
        assert _check_inverse("window/istft/128_128/B/T%d" % T, _pair(T, 128, 128, T, amp=0.9), 128, 128, "B")[2] > 0.1
    assert np.all(window_of("B", 128, 128)[32:96] == 0) and np.all(do.envelope_f32(3, 128, 128, window_of("B", 128, 128))[32:96] == 0)


# ---------------------------------------------------------------- 3: quiet and loud input
@pytest.mark.parametrize("level", ("2^-12", "8", "2^-16", "i16_2lsb"))
@pytest.mark.parametrize("n_fft,hop", ((1024, 256), (384, 48)))
def test_amplitude(n_fft, hop, level):
    """The same signal at a peak of 2^-12 (about -72 dBFS: most samples are fp16 subnormals in the hi plane) and 8.0, held to the same relative bars;
    int16 input of +-2 LSB, exact in the hi plane and half of it subnormal there.  At 2^-16 the lo plane is subnormal too and the representation
    alone is at 1e-6: recorded, not asserted."""
    T = 20
    L = [_wav_len(T, n_fft, hop), n_fft // 2 + 1]
    if level == "i16_2lsb":
        rng = np.random.default_rng(77)
        wavs = [rng.integers(-2, 3, n).astype(np.int16) for n in L]
        peak = 2.0 / 32768.0
    else:
        peak = {"2^-12": 2.0 ** -12, "8": 8.0, "2^-16": 2.0 ** -16}[level]
        wavs = [_sig(n, 3 + i, n_fft, peak) for i, n in enumerate(L)]
        assert abs(float(np.abs(wavs[0]).max()) / peak - 1) < 1e-6
    check = level != "2^-16"
    bias = _bias(n_fft, peak / 0.3)
    tag = "amplitude/%s/%d_%d/%s" % ("%s", n_fft, hop, level)
    _check_forward_gain(tag % "stft_gain", wavs, n_fft, hop, "hann", bias, check=check)
    _check_inverse(tag % "istft", wavs, n_fft, hop, "hann", check=check, alone=False)


# ---------------------------------------------------------------- 4: non-finite samples
def _reached(i0, n_fft, hop):
    """the frames whose n_fft samples hold sample i0 (away from the reflected ends)"""
    return np.arange((i0 - n_fft // 2) // hop + 1, (i0 + n_fft // 2) // hop + 1)


@pytest.mark.parametrize("kind", ("nan", "inf"))
def test_a_non_finite_sample_gives_zero_cells_and_stays_in_its_frames(kind):
    """include/evhip.h, ev_denoise step 3: mag == 0 (and a NaN) gives a zero cell.  One NaN (or +inf, whose lo plane is inf - inf) in the middle of
    utterance 0: every cell of the frames that hold it is zero, padding bins included, the planes and the output are finite, the output is the
    oracle's with those frames zeroed, and utterance 1 keeps the bits it has alone -- through the two entry points and through EVEngine.denoise."""
    n_fft, hop, T, i0 = 1024, 256, 20, 2400
    clean = _pair(T, n_fft, hop, 6)
    bad = [clean[0].copy(), clean[1]]
    bad[0][i0] = np.float32(np.nan if kind == "nan" else np.inf)
    clean[0][i0] = 0.0
    dead = _reached(i0, n_fft, hop)
    assert dead.tolist() == [8, 9, 10, 11]
    bias, st = _bias(n_fft), (0.5, 2.0)
    spec, frames = [], []
    for w, s in zip(clean, st):
        re, im = do.stft64(w, n_fft, hop)
        gre, gim, _ = do.gain64(re, im, bias, s)
        if w is clean[0]:
            gre[dead], gim[dead] = 0.0, 0.0
        spec.append((gre, gim))
        frames.append(gre.shape[0])
    # the corrected oracle says the same of the signal that holds the NaN itself
    if kind == "nan":
        g2 = do.gain64(*do.stft64(bad[0], n_fft, hop), bias, st[0])
        assert np.array_equal(g2[0], spec[0][0]) and np.array_equal(g2[1], spec[0][1])
    want_spec = np.concatenate([do.pack_spectrum(*s, n_fft=n_fft) for s in spec]).astype(np.float64)
    want = [do.istft64(*s, n_fft, hop) for s in spec]
    e32 = max(do.peak_error(_istft32(s[0], s[1], n_fft, hop, None), y) for s, y in zip(spec, want))
    bar = 4 * max(e32, _inverse_ref_err(n_fft, hop))
    bar_mag = 4 * max(fo.mag_error(np.concatenate([_forward32(w, None, n_fft, hop, None)[0] for w in clean]),
                                   np.concatenate([np.sqrt(r * r + i * i) for r, i in (do.stft64(w, n_fft, hop) for w in clean)])), FLOOR)
    hi, lo = _gain(bad, bias, st, n_fft, hop)
    n_nonf = int((~np.isfinite(hi)).sum() + (~np.isfinite(lo)).sum())
    print(kind, "non-finite plane values", n_nonf, "of", 2 * hi.size)
    assert n_nonf == 0, "%d non-finite values in the planes" % n_nonf
    assert np.all(hi[dead] == 0) and np.all(lo[dead] == 0) and np.all(hi[:, 1026:] == 0) and np.all(lo[:, 1026:] == 0)
    e_spec = tgd._spec_error(_planes64(hi, lo), want_spec)
    out, i16 = _istft(hi, lo, frames, n_fft, hop)
    n0 = hop * (T - 1)
    e = max(do.peak_error(out[:n0], want[0]), do.peak_error(out[n0:], want[1]))
    _rep_d("nonfinite/%s/ops" % kind, dict(e_spec=e_spec, bar_spec=3 * bar_mag + FLOOR, e=e, bar=bar))
    assert np.all(np.isfinite(out)) and e_spec <= 3 * bar_mag + FLOOR and e <= bar and np.array_equal(i16, do.to_i16(out))
    hi1, lo1 = _gain(bad[1:], bias, st[1:], n_fft, hop)
    out1, _ = _istft(hi1, lo1, frames[1:], n_fft, hop)
    assert np.array_equal(hi1.view(np.uint16), hi[T:].view(np.uint16)) and np.array_equal(lo1.view(np.uint16), lo[T:].view(np.uint16))
    assert np.array_equal(tgd._bits(out1), tgd._bits(out[n0:]))
    # the public call
    from emotivoice_amd.denoise import DenoiseConfig
    from emotivoice_amd.engine import EVEngine
    eng = EVEngine(precision="mx")
    try:
        cfg = DenoiseConfig(strength=0.5, bias=bias, want_int16=True)
        res = eng.denoise(bad, cfg, strengths=list(st))
        ys = [y.copy() for y in res["wav_list"]]
        e_api = max(do.peak_error(y, y64) for y, y64 in zip(ys, want))
        _rep_d("nonfinite/%s/denoise" % kind, dict(e=e_api, bar=bar))
        assert all(np.all(np.isfinite(y)) for y in ys) and e_api <= bar and np.array_equal(res["wav_i16"], do.to_i16(res["wav"]))
        alone = eng.denoise(bad[1:], cfg, strengths=[st[1]])["wav_list"][0]
        assert np.array_equal(tgd._bits(alone), tgd._bits(ys[1]))
    finally:
        eng.close()


def test_features_keeps_a_non_finite_sample_inside_its_utterance():
    """include/evhip.h states no rule for a non-finite sample in ev_features: what is held is that the other utterance keeps its bits and nothing
    is written outside the packed outputs (the sentinel check of the helper)."""
    from test_gpu_features import _op
    from emotivoice_amd.features import mel_filterbank
    mb = mel_filterbank()
    wavs = _pair(20, 1024, 256, 6)
    alone = _op(wavs[1:], mb, 1024, 256)[0]
    for v in (np.nan, np.inf):
        bad = [wavs[0].copy(), wavs[1]]
        bad[0][2400] = np.float32(v)
        both = _op(bad, mb, 1024, 256)
        for a, b in zip(alone, both[1]):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
        ok = np.setdiff1d(np.arange(20), _reached(2400, 1024, 256))
        o = fo.features64(wavs[0], mb)      # frames the sample does not reach are those of the clean signal
        assert fo.mag_error(both[0][2][ok], o["mag"][ok]) <= 4 * FLOOR


# ---------------------------------------------------------------- 5: the two forward kernels share one front end
@pytest.mark.parametrize("i16", (False, True), ids=("f32", "i16"))
@pytest.mark.parametrize("n_fft,hop,T", ((128, 128, 3), (384, 48, 70)), ids=("128_128", "384_48"))
def test_mel_and_gain_kernels_give_the_same_magnitude_bits(n_fft, hop, T, i16):
    """stft_mel_kernel's mag output and stft_gain_kernel's magnitude mode are the same code up to and including sqrtf(re * re + im * im)
    (stft_begin, stft_tile_loop): through ev_op_stft_mel and ev_op_stft_gain the two arrays are equal bit for bit.  B = 2, window A; 3 frames, and
    70 frames (a partial second tile).  The small shape is 128 / 128: at 128 / 8 an utterance has 9 frames or more (n_fft / 2 + 1 = 65 samples)
    and ev_op_stft_gain answers -2 (R = 16), so no shape with hop 8 reaches both kernels."""
    from emotivoice_amd.features import mel_filterbank
    window = window_of("A", n_fft, hop)
    wavs = _pair(T, n_fft, hop, T)
    if i16:
        wavs = [np.round(w * 32767.0).astype(np.int16) for w in wavs]
    lens = np.array([len(w) for w in wavs], np.int64)
    TT, nb, n_mels = int((lens // hop + 1).sum()), n_fft // 2 + 1, 20
    assert int(lens[0]) // hop + 1 == T
    mb = np.ascontiguousarray(mel_filterbank(16000, n_fft, n_mels, 0.0, 8000.0), np.float32)
    d_wav = torch.from_numpy(np.concatenate(wavs)).cuda()
    d_mel, d_en = torch.zeros(TT * n_mels, device="cuda"), torch.zeros(TT, device="cuda")
    d_mag = torch.full((TT, nb), float("nan"), device="cuda")
    rc = _lib().ev_op_stft_mel(d_wav.data_ptr(), int(i16), len(wavs), lens.ctypes.data, mb.ctypes.data, _wp(window), n_fft, hop, n_mels, 1e-5, 1e-10,
                               0.0, 1.0, d_mel.data_ptr(), d_en.data_ptr(), d_mag.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    from_mel = d_mag.cpu().numpy()
    from_gain = _gain(wavs, None, None, n_fft, hop, window, mag=True)
    assert from_mel.shape == from_gain.shape and np.all(np.isfinite(from_mel)) and from_mel.max() > 0
    assert np.array_equal(tgd._bits(from_mel), tgd._bits(from_gain))


# ---------------------------------------------------------------- 2: the public configurations with a real window
def test_public_configs_take_a_real_window_and_forget_it():
    """EVEngine.features with FeatureConfig(window=A) and EVEngine.denoise with DenoiseConfig(window=A) at the default shape against the oracle
    with that window; a second setup with window=None on the same engine gives the default's bits again."""
    from emotivoice_amd.denoise import DenoiseConfig
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.features import FeatureConfig, mel_filterbank
    A = window_of("A", 1024, 256)
    wavs = [_sig(20011, 2, 1024), _sig(513, 3, 1024)]
    mb = mel_filterbank()
    re0, im0 = do.stft64(wavs[0], window=A)
    bias = np.quantile(np.sqrt(re0 * re0 + im0 * im0), 0.9, axis=0).astype(np.float32)      # as _check_inverse has it: a thinned-out spectrum shows a flip
    rev = np.ascontiguousarray(A[::-1])
    eng = EVEngine(precision="mx", keep_stages=True)
    try:
        eng.features_setup(FeatureConfig())
        f0 = eng.features(wavs)
        d0 = [y.copy() for y in eng.denoise(wavs, DenoiseConfig(strength=1.0, bias=bias))["wav_list"]]
        eng.features_setup(FeatureConfig(window=A))
        fa = eng.features(wavs)
        mags = eng.get_stage("feat_mag").reshape(-1, 513)
        offs = np.concatenate([[0], np.cumsum(fa["mel_lens"])])
        for b, w in enumerate(wavs):
            o = fo.features64(w, mb, window=A)
            m32, l32, e32 = _forward32(w, mb, 1024, 256, A)
            rows = dict(mel=(fo.mel_error(fa["mel_list"][b], o["mel"]), fo.mel_error(l32, o["mel"])),
                        energy=(fo.energy_error(fa["energy_list"][b], o["energy"]), fo.energy_error(e32, o["energy"])),
                        mag=(fo.mag_error(mags[offs[b]:offs[b + 1]], o["mag"]), fo.mag_error(m32, o["mag"])))
            _rep_f("api/features/A/u%d" % b, {k: dict(e=v[0], e32=v[1], bar=4 * max(v[1], FLOOR)) for k, v in rows.items()})
            assert all(v[0] <= 4 * max(v[1], FLOOR) for v in rows.values()), (b, rows)
            assert fo.mag_error(fo.features64(w, mb, window=rev)["mag"], o["mag"]) > 0.1
        da = [y.copy() for y in eng.denoise(wavs, DenoiseConfig(strength=1.0, bias=bias, window=A))["wav_list"]]
        for b, w in enumerate(wavs):
            y64 = do.denoise64(w, bias, 1.0, window=A)
            gre, gim = _oracle_spectrum(w, bias, 1.0, 1024, 256, A)
            e32 = do.peak_error(_istft32(gre, gim, 1024, 256, A), do.istft64(gre.astype(np.float64), gim.astype(np.float64), window=A))
            e, bar = do.peak_error(da[b], y64), 4 * max(e32, _inverse_ref_err(1024, 256))
            _rep_d("api/denoise/A/u%d" % b, dict(e=e, e32=e32, bar=bar))
            assert da[b].size == 256 * (w.size // 256) and e <= bar, (b, e, bar)
            if b == 0:      # the window reversed in both halves, in the forward half alone, in the inverse half alone: each is far away
                fre, fim = _oracle_spectrum(w, bias, 1.0, 1024, 256, rev)
                flips = (do.peak_error(do.denoise64(w, bias, 1.0, window=rev), y64), do.peak_error(do.istft64(fre.astype(np.float64), fim.astype(np.float64), window=A), y64),
                         do.peak_error(do.istft64(gre.astype(np.float64), gim.astype(np.float64), window=rev), y64))
                assert min(flips) > 0.1, flips
        # the tables of the custom setups do not survive a default setup
        eng.features_setup(FeatureConfig())
        f1 = eng.features(wavs)
        d1 = eng.denoise(wavs, DenoiseConfig(strength=1.0, bias=bias))["wav_list"]
        for b in range(2):
            assert np.array_equal(tgd._bits(f1["mel_list"][b]), tgd._bits(f0["mel_list"][b])) and np.array_equal(tgd._bits(f1["energy_list"][b]), tgd._bits(f0["energy_list"][b]))
            assert np.array_equal(tgd._bits(d1[b]), tgd._bits(d0[b]))
            assert not np.array_equal(tgd._bits(fa["mel_list"][b]), tgd._bits(f0["mel_list"][b])) and not np.array_equal(tgd._bits(da[b]), tgd._bits(d0[b]))
    finally:
        eng.close()
