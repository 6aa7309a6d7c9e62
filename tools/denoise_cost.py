#!/usr/bin/env python3
"""Cost of ev_denoise on device input at 32 utterances x 16 s and at one utterance of 1 s: the stft_gain and istft_ola kernel times (the
handle's launch records with profiling on), the "total" region and the wall time per call with profiling off -- and, for comparison, the path
it replaces: the D2H copy of the fp32 waveform plus the same arithmetic in torch on the CPU (torch.stft, the gain, torch.istft with the hann
window: a restatement of the reference's STFT class, which is a conv1d / conv_transpose1d pair and slower still), and one synthesis step at
batch 32 for scale.  The sclk that rocm-smi shows right after the timed loop is recorded as the clock state of the run.

    python tools/denoise_cost.py [--reps 10] [--json profiles/denoise_cost.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=10).stdout
        m = re.search(r"sclk clock level: \S+ \((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from emotivoice_amd import _ffi
    from emotivoice_amd.denoise import DenoiseConfig
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_inputs, synth_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("denoise_cost.py measures on the GPU: none found")
    eng = EVEngine(device_id=0)
    eng.load_blob(*pack_state_dict(synth_state_dict(0, "bench")))
    eng.denoise_setup(DenoiseConfig(strength=0.01))      # measures the seeded vocoder's own bias
    bias = torch.from_numpy(eng.denoise_bias())
    med = lambda x: float(np.median(x)) if len(x) else None      # noqa: E731
    rng = np.random.default_rng(0)
    cases = []
    for B, L in ((32, 16 * 16000), (1, 16000)):
        host = (0.3 * rng.standard_normal(B * L)).clip(-1, 1).astype(np.float32)
        wav = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        lens = np.full(B, L, np.int64)

        def call():
            return eng.denoise_raw(B, wav.data_ptr(), False, lens, None, _ffi.EV_FLAG_DEVICE_INPUTS)

        for _ in range(2):
            res = call()
        assert res.total == B * (L // 256) * 256
        total, kern = [], {}
        eng.set_profiling(True)
        for _ in range(args.reps):
            call()
            total.append(eng.timings()["total"])
            for r in eng.launch_records():
                kern.setdefault(r["name"], []).append(r)
        eng.set_profiling(False)
        wall = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        clock = sclk()
        kernels = {}
        for name, rs in kern.items():
            ms = med([r["ms"] for r in rs])
            kernels[name] = dict(ms_median=ms, tflops=rs[0]["flops"] / (ms * 1e9) if ms else None, gbytes_per_s=rs[0]["bytes"] / (ms * 1e6) if ms else None)
        # the path it replaces: D2H, then the CPU
        win = torch.hann_window(1024, periodic=True)
        d2h, cpu = [], []
        for _ in range(max(2, args.reps // 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = wav.cpu().view(B, L)
            t1 = time.perf_counter()
            S = torch.stft(x, 1024, 256, 1024, win, center=True, pad_mode="reflect", return_complex=True)
            mag = S.abs()
            g = torch.where(mag > 0, torch.clamp(mag - 0.01 * bias.view(1, -1, 1), min=0.0) / torch.where(mag > 0, mag, torch.ones_like(mag)), torch.zeros_like(mag))
            y = torch.istft(S * g, 1024, 256, 1024, win, center=True, length=(L // 256) * 256)
            t2 = time.perf_counter()
            d2h.append((t1 - t0) * 1e3)
            cpu.append((t2 - t1) * 1e3)
        del y
        cases.append(dict(workload="ev_denoise: %d x %d samples, device input, n_fft 1024, hop 256" % (B, L), reps=args.reps, total_ms_median=med(total),
                          wall_ms_median=med(wall), wall_ms_min=float(min(wall)), wall_ms_max=float(max(wall)), kernels=kernels, sclk_mhz_after=clock,
                          replaced_path=dict(d2h_ms_median=med(d2h), cpu_torch_stft_ms_median=med(cpu), cpu_threads=torch.get_num_threads())))
    # one synthesis step at batch 32, for scale
    utts = synth_inputs(1, [64] * 32, [0] * 32)
    from emotivoice_amd.packing import pack_utts
    ling, cu, spk, style, content = pack_utts(utts)
    step = []
    for i in range(args.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = eng.synthesize_raw(32, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data)
        if i >= 2:
            step.append((time.perf_counter() - t0) * 1e3)
    out = dict(cases=cases, synthesis_step=dict(workload="ev_synthesize: 32 x 64 phonemes, host inputs", wall_ms_median=med(step), seconds_of_audio=r.total_samples / 16000.0))
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
