#!/usr/bin/env python3
"""Cost of response delivery: 32 utterances of 16 s at 16 kHz, already on the device, to 8 kHz mu-law, 24 kHz int16 and 48 kHz int16 --
(a) ``ev_deliver`` and the D2H copy of its bytes; (b) the way without it to the SAME bytes (checked once per target): ``ev_resample`` to fp32, the
D2H copy of the fp32 waveform, then numpy / ``audioop`` on the host; (c) the kernel time of ``ev_deliver``'s kernel beside ``ev_resample``'s for
the same rate pair (hipEvents around the launch, profiling on, in passes of their own).  (a) and (b) are host clocks around calls that end in a
device synchronise, profiling off, alternating within every repeat; median, minimum and maximum over --reps after a warm-up of every shape.  The
signal is the tests' synthetic voiced one, not speech.

    python tools/bench_deliver.py [--reps 7] [--json profiles/deliver_cost.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TARGETS = ((8000, "ulaw"), (24000, "s16"), (48000, "s16"))
B, SECONDS, SR = 32, 16, 16000


def voiced(n, sample_rate=16000, seed=0):
    import numpy as np
    t = np.arange(n, dtype=np.float64) / sample_rate
    x = sum(np.sin(2 * np.pi * 120.0 * h * t + 0.37 * h) / h for h in range(1, 25))
    x *= 0.5 * (1.0 + np.sin(2 * np.pi * 3.0 * t))
    return (0.22 * x + 0.002 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def host_convert(y, encoding):
    """fp32 -> the bytes ev_deliver writes without dither, on the host: the truncating int16 rule, then audioop for G.711."""
    import audioop

    import numpy as np
    s16 = np.trunc(np.clip(y * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)
    if encoding == "s16":
        return s16.tobytes()
    return (audioop.lin2ulaw if encoding == "ulaw" else audioop.lin2alaw)(s16.tobytes(), 2)


def stats(x):
    import numpy as np
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "deliver_cost.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5: the spread is part of the result")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_deliver needs a GPU: no time is reported without one")
    from emotivoice_amd import _ffi
    from emotivoice_amd.delivery import DeliveryConfig
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.resample import ResampleConfig

    DEV = _ffi.EV_FLAG_DEVICE_INPUTS
    eng = EVEngine(device_id=0)
    n = SECONDS * SR
    lens = np.full(B, n, np.int64)
    one = voiced(n)
    dev = torch.from_numpy(np.concatenate([one * np.float32(0.5 + 0.05 * (b % 8)) for b in range(B)])).cuda()
    torch.cuda.synchronize()
    rows = []
    for sr_out, enc in TARGETS:
        dc = DeliveryConfig(sr_out, enc)
        eng.deliver_setup(dc, SR)
        eng.resample_setup(ResampleConfig(sr_in=SR, sr_out=sr_out))

        def with_deliver():
            return eng.deliver_to_numpy(eng.deliver_raw(B, dev.data_ptr(), False, lens, None, DEV), dc)["delivered_list"]

        def without():
            y = eng.resample_to_numpy(eng.resample_raw(B, dev.data_ptr(), False, lens, DEV))["wav_list"]
            return [host_convert(w, enc) for w in y]

        got, ref = with_deliver(), without()      # the warm-up of both shapes, and the check that both ways give the same bytes
        same = all(g.tobytes() == r for g, r in zip(got, ref))
        ta, tb = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); with_deliver(); ta.append((time.perf_counter() - t0) * 1e3)      # noqa: E702
            t0 = time.perf_counter(); without(); tb.append((time.perf_counter() - t0) * 1e3)           # noqa: E702
        kern = {}
        eng.set_profiling(True)
        for name, run in (("deliver", lambda: eng.deliver_raw(B, dev.data_ptr(), False, lens, None, DEV)),
                          ("resample", lambda: eng.resample_raw(B, dev.data_ptr(), False, lens, DEV))):
            run()
            for _ in range(args.reps):
                run()
                for r in eng.launch_records():
                    kern.setdefault(r["name"], []).append(r["ms"])
        eng.set_profiling(False)
        d2h_a = int(eng.last_deliver.total_bytes)
        row = dict(sr_out=sr_out, encoding=enc, batch=B, seconds=SECONDS, same_bytes=bool(same), d2h_bytes_deliver=d2h_a, d2h_bytes_resample_fp32=int(eng.last_resample.total_samples) * 4,
                   deliver_and_copy_ms=stats(ta), resample_copy_host_convert_ms=stats(tb), kernels_ms={k: stats(v) for k, v in kern.items()})
        rows.append(row)
    eng.close()
    out = dict(reps=args.reps, signal="synthetic voiced (not speech)", input="device fp32, %d x %d s at %d Hz" % (B, SECONDS, SR), rows=rows)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
