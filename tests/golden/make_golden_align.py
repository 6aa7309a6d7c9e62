#!/usr/bin/env python3
"""Generate tests/golden/align/aln_*.npz (ev_align fixtures) by running the REFERENCE ITSELF in its teacher-forced branch
(imported in place from the reference checkout -- only possible in the build container, never on the GPU box).

The synthetic weights of oracle/weights.py (with the aligner biases of tests/align_oracle.aligner_state_dict: synth_state_dict leaves
them at zero) are loaded with load_state_dict(strict=True) into the reference's JETSGenerator, and
JETSGenerator.forward(..., mel_targets, output_lengths, pitch_targets, energy_targets, cut_flag=False) runs with B = 1 -- AlignmentModule,
viterbi_decode (the numba functions as plain Python, through make_golden.py's stub), average_by_duration, the length regulator fed
with the aligned durations and the generator on the whole mel.  Recorded: the inputs, x_proj (embed_projection1 output), log_p_attn,
duration_targets, pitch_targets / energy_targets (the per-token averages), bin_loss, dec_outputs and wav_predictions.

Cases: a mel the reference itself synthesised for the same text, that mel time-stretched to ~1.4x its length, a smooth random mel,
and a T == N case (every duration 1).

Usage:  python tests/golden/make_golden_align.py [--only <case>]
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

from align_oracle import aligner_state_dict  # noqa: E402
from make_golden import load_reference  # noqa: E402
from oracle.weights import EVShapes, synth_inputs, synth_state_dict  # noqa: E402

# name: (input seed, N, speaker, mel kind, T for the random kinds)
CASES = {
    "aln_n48_selfmel": (31, 48, 17, "self", None),
    "aln_n48_stretch": (31, 48, 17, "stretch", None),
    "aln_n96_random": (32, 96, 905, "random", 300),
    "aln_n24_tn": (33, 24, 1500, "random", 24),
}


def smooth(rng, T, ch, width=9, scale=1.0):
    """(ch, T) smooth random signal: white noise through a moving average."""
    x = rng.standard_normal((ch, T + width - 1))
    k = np.ones(width) / width
    return (np.stack([np.convolve(r, k, mode="valid") for r in x]) * scale).astype(np.float32)


def stretch(mel, factor):
    """linear interpolation along time to round(factor * T) frames."""
    T = mel.shape[1]
    T2 = int(round(T * factor))
    pos = np.linspace(0, T - 1, T2)
    return np.stack([np.interp(pos, np.arange(T), r) for r in mel]).astype(np.float32)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen = load_reference()
    shapes = EVShapes()
    sd = aligner_state_dict(synth_state_dict(0, "parity", shapes))
    gen.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    for name, (iseed, N, spk, kind, Tr) in CASES.items():
        if only and name != only:
            continue
        utt = synth_inputs(iseed, [N], [spk], shapes)[0]
        ling = torch.from_numpy(utt["ling"]).long().unsqueeze(0)
        args = dict(inputs_ling=ling, input_lengths=torch.tensor([N]), inputs_speaker=torch.tensor([utt["speaker"]]),
                    inputs_style_embedding=torch.from_numpy(utt["style"]).unsqueeze(0),
                    inputs_content_embedding=torch.from_numpy(utt["content"]).unsqueeze(0))
        rng = np.random.default_rng(1000 + iseed)
        with torch.no_grad():
            if kind in ("self", "stretch"):
                mel = gen(**args)["dec_outputs"].squeeze(0).t().numpy().copy()       # (n_mels, T): the reference's own synthesis
                if kind == "stretch":
                    mel = stretch(mel, 1.4)
            else:
                mel = smooth(rng, Tr, shapes.n_mels, scale=2.0)
            T = mel.shape[1]
            pitch_f = smooth(rng, T, 1, width=15, scale=3.0)[0]
            energy_f = smooth(rng, T, 1, width=5, scale=3.0)[0]
            taps = {}
            hk = gen.am.embed_projection1.register_forward_hook(lambda _m, _i, o: taps.__setitem__("x_proj", o.detach().squeeze(0).clone()))
            out = gen(**args, mel_targets=torch.from_numpy(mel).unsqueeze(0), output_lengths=torch.tensor([T]),
                      pitch_targets=torch.from_numpy(pitch_f).view(1, T, 1), energy_targets=torch.from_numpy(energy_f).view(1, T, 1),
                      cut_flag=False)
            hk.remove()
        res = dict(
            in_ling=utt["ling"], in_speaker=np.int64(utt["speaker"]), in_style=utt["style"], in_content=utt["content"],
            in_mel=mel, in_pitch_frames=pitch_f, in_energy_frames=energy_f, weight_seed=np.int64(0), dur_mode=np.array("parity"),
            x_proj=taps["x_proj"].numpy(),
            log_p_attn=out["log_p_attn"].squeeze(0).numpy(),
            duration_targets=out["duration_targets"].squeeze(0).numpy().astype(np.int64),
            pitch_targets=out["pitch_targets"].squeeze(0).numpy(),
            energy_targets=out["energy_targets"].squeeze(0).numpy(),
            bin_loss=np.float32(out["bin_loss"]),
            dec_outputs=out["dec_outputs"].squeeze(0).numpy(),
            wav_predictions=out["wav_predictions"].reshape(-1).numpy(),
        )
        os.makedirs(os.path.join(HERE, "align"), exist_ok=True)       # not tests/golden/*.npz: the parity tests take those as inference fixtures
        path = os.path.join(HERE, "align", name + ".npz")
        np.savez_compressed(path, **res)
        d = res["duration_targets"]
        print(name, "N", N, "T", T, "dur[min,max]", d.min(), d.max(), "bin_loss %.4f" % float(res["bin_loss"]), "%d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
