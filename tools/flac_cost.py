#!/usr/bin/env python3
"""Cost of a flac response: one ``ev_flac`` on device PCM at 1 and at 32 utterances of about 10 s (16 kHz), from int16 and from fp32 -- the
hipEvent time of its two kernels (profiling on, median over --reps after a warm-up), the wall time of the call (encode, the frame sizes to the
host, the layout, the gather) and the stream's size -- beside the device -> host copy of the same PCM as int16, which is what a pcm response
moves.  The signal is the tests' synthetic voiced one (24 harmonics, a 3 Hz envelope, a noise floor): its ratio says nothing about speech.

    python tools/flac_cost.py [--reps 10] [--json profiles/flac_cost.json]
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
    x = 0.22 * x + 0.002 * np.random.default_rng(seed).standard_normal(n)
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "flac_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine

    med = lambda x: float(np.median(x))      # noqa: E731
    eng = EVEngine(device_id=0)
    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        lens = np.array([int(args.seconds * 16000) + 256 * ((7 * b) % 13) for b in range(B)], np.int64)      # about 10 s, unequal
        pcm = np.concatenate([voiced(int(n), seed=b) for b, n in enumerate(lens)])
        d16 = torch.from_numpy(pcm).cuda()
        d32 = torch.from_numpy(pcm.astype(np.float32) / np.float32(32768.0)).cuda()
        torch.cuda.synchronize()
        for name, ptr, is16 in (("int16", d16.data_ptr(), True), ("fp32", d32.data_ptr(), False)):
            run = lambda: eng.flac_raw(B, ptr, is16, lens, None, _ffi.EV_FLAG_DEVICE_INPUTS)      # noqa: E731
            res = run()
            wall, kern = [], {}
            for _ in range(args.reps):
                t0 = time.perf_counter()
                run()
                wall.append((time.perf_counter() - t0) * 1e3)
            eng.set_profiling(True)
            for _ in range(args.reps):
                run()
                for r in eng.launch_records():
                    kern.setdefault(r["name"], []).append(r["ms"])
            eng.set_profiling(False)
            d2h_flac = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                eng.d2h(res.bytes, (int(res.total_bytes),), np.uint8)
                d2h_flac.append((time.perf_counter() - t0) * 1e3)
            rows.append(dict(batch=B, input=name, samples=int(lens.sum()), frames=int(res.total_frames), pcm_bytes=int(2 * lens.sum()),
                             flac_bytes=int(res.total_bytes), call_wall_ms_median=med(wall), flac_encode_ms_median=med(kern["flac_encode"]),
                             flac_gather_ms_median=med(kern["flac_gather"]), d2h_flac_ms_median=med(d2h_flac)))
        d2h = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            eng.d2h(d16.data_ptr(), (pcm.size,), np.int16)
            d2h.append((time.perf_counter() - t0) * 1e3)
        for r in rows:
            if r["batch"] == B:
                r["d2h_pcm_int16_ms_median"] = med(d2h[1:])
        del d16, d32
    eng.close()
    out = dict(reps=args.reps, seconds=args.seconds, signal="synthetic voiced (not speech)", rows=rows)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(args.json), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
