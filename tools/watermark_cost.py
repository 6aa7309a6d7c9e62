#!/usr/bin/env python3
"""Cost of ev_watermark and ev_watermark_detect on device input, beside ev_denoise at the same shapes in the same run: 32 segments x 16 s and one
segment of 1 s (latency).  The three calls alternate inside every repetition, so that they see the same clocks and the same neighbours on the
machine.  Per call the kernel times (the handle's launch records with profiling on), the "total" region and the wall time per call with
profiling off (every call ends in a device synchronise).  The sclk that rocm-smi shows right after the timed loop is recorded as the clock state.

``--dump-vocoder PATH`` also writes 16 s of the vocoder's waveform under the seeded weights (utterances back to back, int16) as an .npz: the
input tools/watermark_robustness.py reads on the CPU.

    python tools/watermark_cost.py [--reps 20] [--json profiles/watermark_cost.json] [--dump-vocoder tests/golden/watermark/vocoder_seeded.npz]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--dump-vocoder", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from emotivoice_amd import _ffi
    from emotivoice_amd.denoise import DenoiseConfig
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_inputs, synth_state_dict
    from emotivoice_amd.watermark import WatermarkConfig

    if not torch.cuda.is_available():
        raise SystemExit("watermark_cost.py measures on the GPU: none found")
    eng = EVEngine(device_id=0)
    eng.load_blob(*pack_state_dict(synth_state_dict(0, "bench")))
    eng.denoise_setup(DenoiseConfig(strength=0.01, bias=np.full(513, 0.5, np.float32)))
    med = lambda x: float(np.median(x)) if len(x) else None      # noqa: E731
    rng = np.random.default_rng(0)
    dev = _ffi.EV_FLAG_DEVICE_INPUTS
    wc = WatermarkConfig(key=0x5EED1234, payload=0xA5, nbits=8)

    def signal(n):      # harmonics with a drifting pitch under a little noise: the cost does not depend on the data
        t = np.arange(n, dtype=np.float64)
        ph = 2 * np.pi * np.cumsum(110.0 + 40.0 * np.sin(2 * np.pi * t / 9000.0)) / 16000.0
        return (0.4 * np.sin(ph) + 0.2 * np.sin(2 * ph) + 0.1 * np.sin(3 * ph) + 0.01 * rng.standard_normal(n)).astype(np.float32)

    cases = []
    for name, B, L in (("batch", 32, 16 * 16000), ("latency", 1, 16000)):
        wav = torch.from_numpy(np.ascontiguousarray(np.tile(signal(L), B))).cuda()
        torch.cuda.synchronize()
        lens = np.full(B, L, np.int64)
        calls = dict(denoise=lambda: eng.denoise_raw(B, wav.data_ptr(), False, lens, None, dev),
                     embed=lambda: eng.watermark_raw(B, wav.data_ptr(), False, lens, wc, dev),
                     detect=lambda: eng.watermark_detect_raw(B, wav.data_ptr(), False, lens, wc.key, 8, dev))
        for _ in range(3):
            for c in calls.values():
                c()
        total, kern, wall = ({k: [] for k in calls} for _ in range(3))
        eng.set_profiling(True)
        for _ in range(args.reps):
            for k, c in calls.items():
                c()
                total[k].append(eng.timings()["total"])
                for r in eng.launch_records():
                    kern[k].append(r)
        eng.set_profiling(False)
        for _ in range(args.reps):
            for k, c in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        clock = sclk()
        per_call = {}
        for k in calls:
            names = sorted({r["name"] for r in kern[k]})
            per_call[k] = dict(total_ms_median=med(total[k]), wall_ms_median=med(wall[k]), wall_ms_min=float(min(wall[k])), wall_ms_max=float(max(wall[k])),
                               kernels={n: dict(ms_median=med([r["ms"] for r in kern[k] if r["name"] == n])) for n in names})
        ratio = per_call["embed"]["total_ms_median"] / per_call["denoise"]["total_ms_median"]
        cases.append(dict(case=name, workload="%d x %d samples at 16 kHz, device input, 8-bit payload" % (B, L), reps=args.reps, calls=per_call,
                          embed_over_denoise_total=ratio, sclk_mhz_after=clock))
    out = dict(cases=cases)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    if args.dump_vocoder:
        need, got, seed = 16 * 16000, [], 1
        while sum(w.size for w in got) < need and seed < 40:
            got += [w for w in eng.synthesize(synth_inputs(seed, [200] * 4, [0, 1, 2, 3]))["wav_list"] if w.size and np.all(np.isfinite(w))]
            seed += 1
        wav = np.concatenate(got)[:need]
        os.makedirs(os.path.dirname(os.path.abspath(args.dump_vocoder)), exist_ok=True)
        np.savez_compressed(args.dump_vocoder, wav=np.clip(np.round(wav * 32768.0), -32768, 32767).astype(np.int16), sample_rate=16000,
                            source="ev_synthesize, synth_state_dict(0, 'bench'), synth_inputs(seed, [200] * 4) for seed = 1 .. %d, back to back" % (seed - 1))
        print("vocoder waveform: %d samples, peak %.3f, from %d utterances" % (wav.size, float(np.abs(wav).max()), len(got)))
    eng.close()


if __name__ == "__main__":
    main()
