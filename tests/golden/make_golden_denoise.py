#!/usr/bin/env python3
"""Generate tests/golden/denoise/dn_*.npz (ev_denoise fixtures) by running the REFERENCE ITSELF: its STFT class (imported in place from a reference
checkout, which the tests never need) computes transform -> clamp(mag - strength * bias, 0) -> inverse in float32, which is what the
Tacotron 2 / WaveGlow / FastPitch Denoiser does on that class.  librosa is stubbed as make_golden_features.py stubs it, plus a ``normalize`` that
returns its argument for norm=None (audio_processing.window_sumsquare calls it).

Recorded per case: the input wav, the bias, the strength, the reference's float32 output, and ref_err: E = max |y - y64| / max |y64| of that output
against the float64 oracle (tests/denoise_oracle.py).  The GPU test's bar is 4 x the largest ref_err over the fixtures.

Signal: the tests' synthetic voiced signal (24 harmonics of 120 Hz under a 3 Hz envelope) plus a 3.1 kHz tone and a noise floor; the bias is the
magnitude of frame 0 of the reference's transform of that tone and noise alone, 88 x 256 samples long.

dn_shape_<n_fft>_<hop>.npz tie the oracle to the same class at the other frame shapes the GPU tests run (SHAPES below): the reference takes named
windows only, so these are hann too.

Usage:  python tests/golden/make_golden_denoise.py [--shapes]      (--shapes: the shape fixtures alone)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import denoise_oracle as do  # noqa: E402
import features_oracle as fo  # noqa: E402
from loudness_oracle import voiced  # noqa: E402
from make_golden import REF  # noqa: E402
from make_golden_features import stub_librosa  # noqa: E402

TONE_HZ, TONE_AMP, NOISE = 3100.0, 0.004, 0.001


def hum(n, seed):
    """What stands for the vocoder's bias: a 3.1 kHz tone and a noise floor."""
    t = np.arange(n, dtype=np.float64) / 16000.0
    return TONE_AMP * np.sin(2 * np.pi * TONE_HZ * t + 0.5) + NOISE * np.random.default_rng(seed).standard_normal(n)


def signal(n, seed):
    return (voiced(n, seed=seed).astype(np.float64) + hum(n, 100 + seed)).astype(np.float32)


def reference_denoise(stft, wav_f32, bias, strength):
    y = torch.from_numpy(np.ascontiguousarray(wav_f32, np.float32)).unsqueeze(0)
    with torch.no_grad():
        mag, phase = stft.transform(y)
        mag = torch.clamp(mag - torch.from_numpy(bias).view(1, -1, 1) * float(np.float32(strength)), 0.0)
        return stft.inverse(mag, phase).reshape(-1).numpy().astype(np.float32), mag.squeeze(0).t().numpy()


def save(name, wav, bias, strength, stft):
    wav_f = fo.to_float(wav)
    ref, mag = reference_denoise(stft, wav_f, bias, strength)
    y64 = do.denoise64(wav, bias, strength)
    assert ref.size == y64.size == 256 * (wav_f.size // 256), (ref.size, y64.size)
    err = do.peak_error(ref, y64)
    rel = float(np.linalg.norm(ref - y64) / max(np.linalg.norm(y64), 1e-30))
    path = os.path.join(HERE, "denoise", name + ".npz")
    np.savez_compressed(path, wav=np.asarray(wav), bias=bias, strength=np.float32(strength), ref_out=ref, ref_err=np.float64(err))
    print("%-20s L %6d out %6d s %5.2f  E(ref) %.3e  rel L2(ref) %.3e  cells at the floor %.1f %%  %d bytes"
          % (name, wav_f.size, ref.size, strength, err, rel, 100.0 * float((mag == 0).mean()), os.path.getsize(path)))
    assert os.path.getsize(path) < 1_000_000, path
    return err


SHAPES = ((384, 48), (640, 320), (128, 128))      # a non-power-of-two n_fft with R = 8, R = 2, R = 1: the shapes the GPU shape table adds


def save_shape(n_fft, hop, STFT, window_sumsquare):
    """dn_shape_<n_fft>_<hop>.npz: the reference's STFT class at another frame shape on a 2000-sample signal -- its transform's magnitudes, its
    transform -> clamp -> inverse, its window_sumsquare -- and ref_err of that output against the float64 oracle at the same shape."""
    stft = STFT(n_fft, hop, n_fft, "hann")
    R = n_fft // hop
    wav = signal(2000, 20 + n_fft // 128)
    with torch.no_grad():
        bias = stft.transform(torch.from_numpy(hum(88 * hop, 7).astype(np.float32)).unsqueeze(0))[0][0, :, 0].numpy().astype(np.float32).copy()
        ref_mag = stft.transform(torch.from_numpy(wav).unsqueeze(0))[0].squeeze(0).t().contiguous().numpy().astype(np.float32)
    ref, _ = reference_denoise(stft, wav, bias, 0.1)
    y64 = do.denoise64(wav, bias, 0.1, n_fft, hop)
    assert ref.size == y64.size == hop * (2000 // hop) and ref_mag.shape == (2000 // hop + 1, n_fft // 2 + 1)
    err = do.peak_error(ref, y64)
    envs = {"env_T%d" % T: window_sumsquare("hann", T, hop_length=hop, win_length=n_fft, n_fft=n_fft, dtype=np.float32) for T in sorted({1, 2, R, R + 1, 2 * R + 3})}
    for key, ws in envs.items():
        assert np.array_equal(ws, do.envelope_f32(int(key[5:]), n_fft, hop)), (n_fft, hop, key)
    path = os.path.join(HERE, "denoise", "dn_shape_%d_%d.npz" % (n_fft, hop))
    np.savez_compressed(path, wav=wav, bias=bias, strength=np.float32(0.1), n_fft=np.int64(n_fft), hop=np.int64(hop), ref_mag=ref_mag, ref_out=ref,
                        ref_err=np.float64(err), **envs)
    re, im = do.stft64(wav, n_fft, hop)
    print("%-20s T %3d out %5d  E(ref) %.3e  E_mag(ref) %.3e  %d bytes"
          % (os.path.basename(path)[:-4], ref_mag.shape[0], ref.size, err, fo.mag_error(ref_mag, np.sqrt(re * re + im * im)), os.path.getsize(path)))
    assert os.path.getsize(path) < 100_000, path
    return err


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    stub_librosa()
    sys.modules["librosa.util"].normalize = lambda x, norm=None, **kw: x if norm is None else (_ for _ in ()).throw(NotImplementedError("norm"))
    sys.path.insert(0, REF)
    from models.prompt_tts_modified.stft import STFT
    if "--shapes" in sys.argv:      # the shape fixtures alone: the others keep their bytes
        from models.prompt_tts_modified.audio_processing import window_sumsquare
        for n_fft, hop in SHAPES:
            save_shape(n_fft, hop, STFT, window_sumsquare)
        return
    stft = STFT(1024, 256, 1024, "hann")
    os.makedirs(os.path.join(HERE, "denoise"), exist_ok=True)
    with torch.no_grad():
        bias = stft.transform(torch.from_numpy(hum(88 * 256, 7).astype(np.float32)).unsqueeze(0))[0][0, :, 0].numpy().astype(np.float32).copy()
    errs = []
    errs.append(save("dn_a_l513", signal(513, 1), bias, 0.1, stft))                 # three frames: every output sample is in an edge region
    errs.append(save("dn_b_l2048", signal(2048, 2), bias, 0.1, stft))
    errs.append(save("dn_c_l20011", signal(20011, 3), bias, 0.1, stft))             # not a multiple of the hop: 19 968 out
    x = signal(20011, 3)
    errs.append(save("dn_d_l20011_i16", np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16), bias, 0.1, stft))
    errs.append(save("dn_e_l20011_s0", signal(20011, 4), bias, 0.0, stft))          # strength 0: the identity
    errs.append(save("dn_f_l20011_s30", signal(20011, 5), bias, 30.0, stft))        # most cells at the floor
    z = signal(8192, 6)
    z[2048:6144] = 0.0                                                              # frames of exact zeros: mag == 0
    errs.append(save("dn_g_l8192_zeros", z, bias, 0.1, stft))

    # inverse only: a spectrum with Im[0] = Im[n_fft / 2] = 0 through the reference's STFT.inverse
    rng = np.random.default_rng(11)
    T = 9
    re = (rng.standard_normal((T, 513)) * 4.0).astype(np.float32)
    im = (rng.standard_normal((T, 513)) * 4.0).astype(np.float32)
    im[:, 0] = im[:, 512] = 0.0
    mag = torch.from_numpy(np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2).astype(np.float32).T.copy()).unsqueeze(0)
    ph = torch.from_numpy(np.arctan2(im.astype(np.float64), re.astype(np.float64)).astype(np.float32).T.copy()).unsqueeze(0)
    with torch.no_grad():
        ref = stft.inverse(mag, ph).reshape(-1).numpy().astype(np.float32)
    y64 = do.istft64(re.astype(np.float64), im.astype(np.float64))
    err = do.peak_error(ref, y64)
    path = os.path.join(HERE, "denoise", "dn_h_inverse_t9.npz")
    np.savez_compressed(path, re=re, im=im, ref_out=ref, ref_err=np.float64(err))
    print("%-20s T %d out %d  E(ref) %.3e  %d bytes" % ("dn_h_inverse_t9", T, ref.size, err, os.path.getsize(path)))
    errs.append(err)

    # the envelope the reference normalises with, for the table test
    from models.prompt_tts_modified.audio_processing import window_sumsquare
    for T in (1, 3, 4, 9, 79):
        ws = window_sumsquare("hann", T, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32)
        assert np.array_equal(ws, do.envelope_f32(T)), T
    np.savez_compressed(os.path.join(HERE, "denoise", "dn_envelope.npz"),
                        **{"T%d" % T: window_sumsquare("hann", T, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32) for T in (1, 3, 4, 9, 79)})
    print("largest E(ref) %.3e -> the bar is 4 x that = %.3e" % (max(errs), 4 * max(errs)))
    for n_fft, hop in SHAPES:
        save_shape(n_fft, hop, STFT, window_sumsquare)


if __name__ == "__main__":
    main()
