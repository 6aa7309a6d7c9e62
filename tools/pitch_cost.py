#!/usr/bin/env python3
"""Cost of ev_pitch at 32 utterances x 1024 frames (262 143 samples each, device input): the "total" region (ev_get_timing), the launch
records with profiling on and the wall time per call with it off -- and, for comparison, the same handle's ev_features on the same waveforms.

    python tools/pitch_cost.py [--reps 10] [--json out.json]
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
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine

    eng = EVEngine(device_id=0)          # ev_pitch needs no weights
    eng.features_setup()
    B, T = 32, 1024
    L = (T - 1) * 256 + 255
    rng = np.random.default_rng(0)
    # a voiced source with noise: the dip search stops early on voiced frames and runs the whole lag range on unvoiced ones
    f0 = np.interp(np.arange(L), np.linspace(0, L - 1, 40), rng.uniform(90.0, 380.0, 40))
    phi = 2.0 * np.pi * np.cumsum(f0) / 16000.0
    one = 0.3 * sum(a * np.sin((h + 1) * phi) for h, a in enumerate((1.0, 0.5, 0.33, 0.25)))
    wav = np.concatenate([one + 0.01 * rng.standard_normal(L) for _ in range(B)]).clip(-1, 1).astype(np.float32)
    wav = torch.from_numpy(wav).cuda()
    torch.cuda.synchronize()
    lens = np.full(B, L, np.int64)

    def pitch():
        return eng.pitch_raw(B, wav.data_ptr(), False, lens, 225.089, 53.78, None, _ffi.EV_FLAG_DEVICE_INPUTS)

    def feats():
        return eng.features_raw(B, wav.data_ptr(), False, lens, 0.0, 1.0, _ffi.EV_FLAG_DEVICE_INPUTS)

    r = pitch()
    assert r.total_frames == B * T
    voiced = float((eng.d2h(r.f0_hz, (B * T,), np.float32) > 0).mean())
    feats()
    total, recs, ftotal = [], None, []
    eng.set_profiling(True)
    for _ in range(args.reps):
        pitch()
        total.append(eng.timings()["total"])
        recs = eng.launch_records()
        feats()
        ftotal.append(eng.timings()["total"])
    eng.set_profiling(False)
    wall = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pitch()
        wall.append((time.perf_counter() - t0) * 1e3)
    med = lambda x: float(np.median(x)) if x else None      # noqa: E731
    for r in recs:
        r["tflops"] = r["flops"] / (r["ms"] * 1e9) if r["ms"] > 0 else None
    out = dict(workload="ev_pitch: %d x %d frames (%d samples each), device input" % (B, T, L), reps=args.reps, voiced_share=voiced,
               total_ms_median=med(total), wall_ms_median=med(wall), launches=recs, features_total_ms_median=med(ftotal))
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
