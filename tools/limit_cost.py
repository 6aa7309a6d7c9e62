#!/usr/bin/env python3
"""Cost of true-peak limiting: one ``ev_limit`` on a device waveform -- 32 segments of 4 s and 8 segments of 60 s at 16 kHz, fp32 + int16 output,
the default look-ahead and hold (80, 800 samples) and a pre-gain of 2.5 that makes the limiter work -- beside one ``ev_loudness`` with a target on
the same input in the same run, the call it replaces: per kernel the hipEvent time and the GB/s of its algorithmic bytes (profiling on, median
over --reps after a warm-up) and the wall time of each call with profiling off.  The signal is the tests' synthetic voiced one.

    python tools/limit_cost.py [--reps 10] [--json profiles/limit_cost.json]
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
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "limit_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.limiter import LimiterConfig
    from emotivoice_amd.loudness import EXAMPLE_TARGET_LUFS, LoudnessConfig

    med = lambda x: float(np.median(x))      # noqa: E731
    eng = EVEngine(device_id=0)
    rows = []
    for B, seconds in ((32, 4), (8, 60)):
        n = seconds * 16000
        lens = np.full(B, n, np.int64)
        one = voiced(n)
        dev = torch.from_numpy(np.concatenate([one * np.float32(0.5 + 0.05 * (b % 8)) for b in range(B)])).cuda()
        torch.cuda.synchronize()
        gains = np.full(B, 2.5, np.float32)
        calls = (("ev_limit", lambda: eng.limit_raw(B, dev.data_ptr(), False, lens, gains, LimiterConfig(want_int16=True), _ffi.EV_FLAG_DEVICE_INPUTS)),
                 ("ev_loudness", lambda: eng.loudness_raw(B, dev.data_ptr(), False, lens, LoudnessConfig(target_lufs=EXAMPLE_TARGET_LUFS, want_int16=True),
                                                          _ffi.EV_FLAG_DEVICE_INPUTS)))
        for name, run in calls:
            res = run()
            wall, total, kern, gbs = [], [], {}, {}
            for _ in range(args.reps):
                t0 = time.perf_counter()
                run()
                wall.append((time.perf_counter() - t0) * 1e3)
            eng.set_profiling(True)
            run()
            for _ in range(args.reps):
                run()
                total.append(eng.timings()["total"])
                for r in eng.launch_records():
                    kern.setdefault(r["name"], []).append(r["ms"])
                    gbs.setdefault(r["name"], []).append(r["bytes"] / (r["ms"] * 1e6) if r["ms"] > 0 else 0.0)
            eng.set_profiling(False)
            row = dict(call=name, batch=B, seconds=seconds, samples=int(lens.sum()), call_wall_ms_median=med(wall), timing_total_ms_median=med(total),
                       **{k + "_ms_median": med(v) for k, v in kern.items()}, **{k + "_gb_per_s_median": med(v) for k, v in gbs.items()})
            if name == "ev_limit":
                row["limited_fraction"] = float(np.ctypeslib.as_array(res.limited, (B,)).sum()) / float(lens.sum())
            rows.append(row)
    eng.close()
    out = dict(reps=args.reps, signal="synthetic voiced (not speech)", lookahead=80, hold=800, rows=rows)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(args.json), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
