#!/usr/bin/env python3
"""Generate tests/golden/features/feat_*.npz (ev_features fixtures) by running the REFERENCE ITSELF: its TacotronSTFT (imported in place
from a reference checkout, which the tests never need) computes the mel and its STFT.transform the magnitudes, in float32 as its training
stack does.  The generator runs without librosa: a stub module provides the names the reference's modules import from it (util.pad_center,
util.tiny, filters.mel = emotivoice_amd.features.mel_filterbank; audio_processing.py's import of librosa.util resolves to the same stub), the
way make_golden.py stubs numba.

Recorded per case: the wav, the reference's mel and magnitudes, the energy formed from those magnitudes (sqrt(max(sum_k mag^2, 1e-10)), float32).
Where all magnitudes would not fit the repository's 1 MB limit per file, ref_mag holds the frames mag_frames (evenly spaced, first and last
included).  The aligned case also records the inputs, log_p_attn, duration_targets and bin_loss of the reference's teacher-forced forward on that
mel, as make_golden_align.py does, after checking on the reference's own log_p_attn that no decision of the search is a near tie (margin >= 1e-4):
a seed whose case has one is skipped for the next.

Cases: (a) the reference's own synthesis of a 48-phoneme utterance, (b) the same wav as int16, (c) a chirp at 0.99 full scale followed by 0.3 s
of exact zeros and by 1e-4 noise, (d) L = 513 and an L that is not a multiple of 256.

stft_<n_fft>_<hop>.npz tie the oracle to the same class built at the other frame shapes the GPU tests run (SHAPES below), with the hann window the
reference's named windows allow.

Usage:  python tests/golden/make_golden_features.py [--shapes]      (--shapes: the shape fixtures alone)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import align_oracle as ao  # noqa: E402
import features_oracle as fo  # noqa: E402
from emotivoice_amd.features import mel_filterbank  # noqa: E402
from make_golden import load_reference  # noqa: E402
from oracle.weights import EVShapes, synth_inputs, synth_state_dict  # noqa: E402

MAX_MAG_BYTES = 600_000
NEAR_TIE = 1e-4


def stub_librosa():
    lib, util, filters = types.ModuleType("librosa"), types.ModuleType("librosa.util"), types.ModuleType("librosa.filters")

    def pad_center(data, size, axis=-1, **kw):
        n = data.shape[axis]
        lpad = (size - n) // 2
        widths = [(0, 0)] * data.ndim
        widths[axis] = (lpad, size - n - lpad)
        return np.pad(data, widths, **kw)

    util.pad_center = pad_center
    util.tiny = lambda x: np.finfo(np.asarray(x).dtype if np.issubdtype(np.asarray(x).dtype, np.floating) else np.float32).tiny
    filters.mel = lambda sr, n_fft, n_mels=128, fmin=0.0, fmax=None, **kw: mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    lib.util, lib.filters = util, filters
    sys.modules["librosa"], sys.modules["librosa.util"], sys.modules["librosa.filters"] = lib, util, filters


def reference_features(stft, wav_f32):
    """the reference's float32 mel (80, T) and magnitudes (T, 513) of one utterance, and the energy of those magnitudes"""
    y = torch.from_numpy(np.ascontiguousarray(wav_f32, np.float32)).unsqueeze(0)
    with torch.no_grad():
        mel = stft.mel_spectrogram(y).squeeze(0).numpy()
        mag = stft.stft_fn.transform(y)[0].squeeze(0).t().contiguous().numpy()
    energy = np.sqrt(np.maximum((mag.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32), np.float32(1e-10))).astype(np.float32)
    return mel, mag, energy


def save(name, wav, stft, extra=None):
    wav_f = fo.to_float(wav)
    mel, mag, energy = reference_features(stft, wav_f)
    T = mel.shape[1]
    assert T == wav_f.size // 256 + 1 and mag.shape == (T, 513)
    keep = np.arange(T)
    if mag.nbytes > MAX_MAG_BYTES:
        keep = np.unique(np.round(np.linspace(0, T - 1, MAX_MAG_BYTES // (513 * 4))).astype(np.int64))
    o = fo.features64(wav)
    res = dict(wav=np.asarray(wav), ref_mel=mel, ref_mag=mag[keep], mag_frames=keep.astype(np.int64), ref_energy=energy)
    res.update(extra or {})
    path = os.path.join(HERE, "features", name + ".npz")
    np.savez_compressed(path, **res)
    clamped = int((o["mel"] == np.log(float(np.float32(1e-5)))).sum())
    print("%-22s L %7d T %4d  E_mel(ref) %.3e  E_energy(ref) %.3e  E_mag(ref) %.3e  clamped cells %d  floor frames %d  %d bytes"
          % (name, wav_f.size, T, fo.mel_error(mel, o["mel"]), fo.energy_error(energy, o["energy"]), fo.mag_error(mag, o["mag"]), clamped,
             int((o["energy"] <= 1.0001e-5).sum()), os.path.getsize(path)))
    assert os.path.getsize(path) < 1_000_000, path
    return mel, energy


SHAPES = ((384, 48), (640, 320))      # the non-power-of-two frame shapes the GPU shape table adds


def save_shape(n_fft, hop, TacotronSTFT):
    """stft_<n_fft>_<hop>.npz: the reference's TacotronSTFT built at another frame shape, on a 2000-sample signal: mel, magnitudes, energy."""
    stft = TacotronSTFT(n_fft, hop, n_fft, 80, 16000, 0.0, 8000.0)
    rng = np.random.default_rng(1000 + n_fft)
    t = np.arange(2000) / 16000.0
    wav = (0.3 * np.sin(2 * np.pi * 310.0 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 9.0 * t)) + 0.02 * rng.standard_normal(2000)).astype(np.float32)
    y = torch.from_numpy(wav).unsqueeze(0)
    with torch.no_grad():
        mel = stft.mel_spectrogram(y).squeeze(0).numpy()
        mag = stft.stft_fn.transform(y)[0].squeeze(0).t().contiguous().numpy()
    energy = np.sqrt(np.maximum((mag.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32), np.float32(1e-10))).astype(np.float32)
    T = 2000 // hop + 1
    assert mel.shape == (80, T) and mag.shape == (T, n_fft // 2 + 1)
    o = fo.features64(wav, mel_filterbank(16000, n_fft, 80, 0.0, 8000.0), n_fft=n_fft, hop=hop)
    path = os.path.join(HERE, "features", "stft_%d_%d.npz" % (n_fft, hop))
    np.savez_compressed(path, wav=wav, n_fft=np.int64(n_fft), hop=np.int64(hop), ref_mel=mel, ref_mag=mag, ref_energy=energy)
    print("%-22s T %4d  E_mel(ref) %.3e  E_energy(ref) %.3e  E_mag(ref) %.3e  %d bytes"
          % (os.path.basename(path)[:-4], T, fo.mel_error(mel, o["mel"]), fo.energy_error(energy, o["energy"]), fo.mag_error(mag, o["mag"]), os.path.getsize(path)))
    assert os.path.getsize(path) < 100_000, path


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    stub_librosa()
    if "--shapes" in sys.argv:      # the shape fixtures alone: the others keep their bytes
        from make_golden import REF
        sys.path.insert(0, REF)
        from models.prompt_tts_modified.tacotron_stft import TacotronSTFT
        for n_fft, hop in SHAPES:
            save_shape(n_fft, hop, TacotronSTFT)
        return
    gen = load_reference()
    from models.prompt_tts_modified.tacotron_stft import TacotronSTFT
    stft = TacotronSTFT(1024, 256, 1024, 80, 16000, 0.0, 8000.0)
    os.makedirs(os.path.join(HERE, "features"), exist_ok=True)
    shapes = EVShapes()
    sd = ao.aligner_state_dict(synth_state_dict(0, "parity", shapes))
    gen.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)

    # (a) / (b): the reference's own synthesis of a 48-phoneme utterance, aligned back to its text through the reference's features
    N, spk = 48, 17
    for iseed in range(41, 61):
        utt = synth_inputs(iseed, [N], [spk], shapes)[0]
        args = dict(inputs_ling=torch.from_numpy(utt["ling"]).long().unsqueeze(0), input_lengths=torch.tensor([N]),
                    inputs_speaker=torch.tensor([utt["speaker"]]), inputs_style_embedding=torch.from_numpy(utt["style"]).unsqueeze(0),
                    inputs_content_embedding=torch.from_numpy(utt["content"]).unsqueeze(0))
        with torch.no_grad():
            wav = gen(**args)["wav_predictions"].reshape(-1).numpy().astype(np.float32).copy()
            mel, _, energy = reference_features(stft, wav)
            T = mel.shape[1]
            out = gen(**args, mel_targets=torch.from_numpy(mel).unsqueeze(0), output_lengths=torch.tensor([T]),
                      pitch_targets=torch.zeros(1, T, 1), energy_targets=torch.from_numpy(energy).view(1, T, 1), cut_flag=False)
        lp = out["log_p_attn"].squeeze(0).numpy()
        m = ao.margins(lp, ao.mas(lp))
        print("seed %d: N %d T %d min margin of the search on the reference's log_p_attn %.3e" % (iseed, N, T, float(m.min())))
        if m.min() >= NEAR_TIE:
            break
        print("  near tie (< %g): next seed" % NEAR_TIE)
    else:
        raise SystemExit("no seed without a near tie")
    extra = dict(in_ling=utt["ling"], in_speaker=np.int64(utt["speaker"]), in_style=utt["style"], in_content=utt["content"],
                 weight_seed=np.int64(0), dur_mode=np.array("parity"), input_seed=np.int64(iseed), log_p_attn=lp,
                 duration_targets=out["duration_targets"].squeeze(0).numpy().astype(np.int64),
                 energy_targets=out["energy_targets"].squeeze(0).numpy(), bin_loss=np.float32(out["bin_loss"]),
                 min_margin=np.float64(m.min()))
    save("feat_a_n48_self", wav, stft, extra)
    save("feat_b_n48_self_i16", np.clip(np.round(wav * 32768.0), -32768, 32767).astype(np.int16), stft)

    # (c) chirp at 0.99 full scale, 0.3 s of exact zeros, 1e-4 noise: both clamps
    rng = np.random.default_rng(7)
    t = np.arange(int(0.9 * 16000)) / 16000.0
    chirp = 0.99 * np.sin(2 * np.pi * (100.0 * t + 0.5 * (7000.0 / 0.9) * t * t))
    c = np.concatenate([chirp, np.zeros(int(0.3 * 16000)), 1e-4 * rng.standard_normal(int(0.4 * 16000))]).astype(np.float32)
    save("feat_c_chirp_zeros", c, stft)

    # (d) the shortest utterance and a length that is not a multiple of the hop
    save("feat_d_l513", (0.5 * rng.standard_normal(513)).clip(-1, 1).astype(np.float32), stft)
    save("feat_d_l20011", (0.3 * np.sin(2 * np.pi * 440.0 * np.arange(20011) / 16000.0) + 0.05 * rng.standard_normal(20011)).clip(-1, 1).astype(np.float32), stft)
    for n_fft, hop in SHAPES:
        save_shape(n_fft, hop, TacotronSTFT)


if __name__ == "__main__":
    main()
