#!/usr/bin/env python3
"""Cost of loudness normalisation: one ``ev_loudness`` on a device waveform of B = 32 segments of 262 144 fp32 samples (the size of a BASELINE
configs[1] batch: 32 x 1 024 frames x 256) -- measure only, with the fp32 output, and with the int16 output as well: the call's device time
from ``ev_get_timing("total")`` and the hipEvent time of its launches (profiling on, median over --reps after a warm-up), and the wall time of the
call with profiling off (launches, the tile sums to the host with the synchronisation, the host's blocks / gates / gain, the gain pass).  The
signal is the tests' synthetic voiced one; the cost does not depend on it.

    python tools/loudness_cost.py [--reps 10] [--json profiles/loudness_cost.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def voiced(n, sample_rate=16000, seed=0):
    import numpy as np
    t = np.arange(n, dtype=np.float64) / sample_rate
    x = sum(np.sin(2 * np.pi * 120.0 * h * t + 0.37 * h) / h for h in range(1, 25))
    x *= 0.5 * (1.0 + np.sin(2 * np.pi * 3.0 * t))
    return (0.22 * x + 0.002 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "loudness_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.loudness import EXAMPLE_TARGET_LUFS, LoudnessConfig

    med = lambda x: float(np.median(x))      # noqa: E731
    eng = EVEngine(device_id=0)
    B = args.batch
    lens = np.full(B, args.samples, np.int64)
    one = voiced(args.samples)
    dev = torch.from_numpy(np.concatenate([one * np.float32(0.5 + 0.05 * (b % 8)) for b in range(B)])).cuda()
    torch.cuda.synchronize()
    rows = []
    for name, cfg in (("measure only", LoudnessConfig()), ("fp32 output", LoudnessConfig(target_lufs=EXAMPLE_TARGET_LUFS)),
                      ("fp32 + int16 output", LoudnessConfig(target_lufs=EXAMPLE_TARGET_LUFS, want_int16=True))):
        run = lambda: eng.loudness_raw(B, dev.data_ptr(), False, lens, cfg, _ffi.EV_FLAG_DEVICE_INPUTS)      # noqa: E731
        res = run()
        figures = eng.loudness_to_numpy(res) if not res.wav else None
        wall, total, kern = [], [], {}
        for _ in range(args.reps):
            t0 = time.perf_counter()
            run()
            wall.append((time.perf_counter() - t0) * 1e3)
        eng.set_profiling(True)
        for _ in range(args.reps):
            run()
            total.append(eng.timings()["total"])
            for r in eng.launch_records():
                kern.setdefault(r["name"], []).append(r["ms"])
        eng.set_profiling(False)
        row = dict(mode=name, batch=B, samples=int(lens.sum()), tiles=int(lens.sum()) // _ffi.EV_LOUDNESS_TILE, call_wall_ms_median=med(wall),
                   timing_total_ms_median=med(total), **{k + "_ms_median": med(v) for k, v in kern.items()})
        if figures is not None:
            row["loudness_lufs_first"] = float(figures["loudness"][0])
        rows.append(row)
    eng.close()
    out = dict(reps=args.reps, signal="synthetic voiced (not speech)", rows=rows)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(args.json), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
