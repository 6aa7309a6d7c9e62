#!/usr/bin/env python3
"""Cost of ev_resample at 32 utterances of 16 s, device input, from 48 000, 44 100 and 22 050 Hz to 16 000 Hz with the trim on and off: the "total"
region (ev_get_timing), the launch records with profiling on and the wall time per call with it off -- and, for comparison, the same handle's
ev_features on the call's output.

    python tools/resample_cost.py [--reps 10] [--json profiles/resample_cost.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "resample_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.resample import ResampleConfig

    eng = EVEngine(device_id=0)          # ev_resample needs no weights
    eng.features_setup()
    B, seconds = 32, 16
    rng = np.random.default_rng(0)
    med = lambda x: float(np.median(x)) if x else None      # noqa: E731
    rows = []
    for sr in (48000, 44100, 22050):
        L = sr * seconds
        t = np.arange(L) / sr
        # a voiced source between half a second of near-silence on each side, so that the trim has something to cut
        one = 0.3 * sum(a * np.sin(2.0 * np.pi * 140.0 * (h + 1) * t) for h, a in enumerate((1.0, 0.5, 0.33, 0.25)))
        one[:sr // 2] *= 1e-4
        one[-sr // 2:] *= 1e-4
        wav = np.concatenate([one + 1e-5 * rng.standard_normal(L) for _ in range(B)]).clip(-1, 1).astype(np.float32)
        wav = torch.from_numpy(wav).cuda()
        torch.cuda.synchronize()
        lens = np.full(B, L, np.int64)
        for trim in (False, True):
            eng.resample_setup(ResampleConfig(sr_in=sr, trim=trim))

            def resample():
                return eng.resample_raw(B, wav.data_ptr(), False, lens, _ffi.EV_FLAG_DEVICE_INPUTS)

            def feats(r):
                out_lens = np.array([r.wav_lens[b] for b in range(B)], np.int64)
                return eng.features_raw(B, r.wav, False, out_lens, 0.0, 1.0, _ffi.EV_FLAG_DEVICE_INPUTS)

            r = resample()
            feats(r)
            total, recs, ftotal = [], None, []
            eng.set_profiling(True)
            for _ in range(args.reps):
                r = resample()
                total.append(eng.timings()["total"])
                recs = eng.launch_records()
                feats(r)
                ftotal.append(eng.timings()["total"])
            eng.set_profiling(False)
            wall = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                resample()
                wall.append((time.perf_counter() - t0) * 1e3)
            for rec in recs:
                rec["tflops"] = rec["flops"] / (rec["ms"] * 1e9) if rec["ms"] > 0 else None
            rows.append(dict(sr_in=sr, trim=trim, samples_in=int(B * L), samples_out=int(r.total_samples), total_ms_median=med(total),
                             wall_ms_median=med(wall), launches=recs, features_total_ms_median=med(ftotal)))
    out = dict(workload="ev_resample: %d x %d s -> 16 kHz, device input" % (B, seconds), reps=args.reps, cases=rows)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
