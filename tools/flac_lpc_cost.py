#!/usr/bin/env python3
"""What LPC subframes and the MD5 signature buy and cost on the vocoder's own output: the default benchmark shape (32 utterances of 256 synthetic
phonemes, seeded "bench" weights, precision "mx", int16) is synthesised once; its device int16 then goes through ``ev_flac`` and ``ev_flac_lpc``
(order 8 and 12, with and without md5).  Per call: the hipEvent time of its kernels (profiling on) and the wall time, medians over --reps warm
calls; per utterance: stream bytes with LPC over stream bytes without (worst, median); and one document of 30 / 120 s (and the whole waveform)
with md5, to show where the serial chain dominates.  The weights are seeded, not a voice: the ratio says nothing about speech.  To compare the
plain path with another build of the library, run this in both trees and alternate the processes.

    python tools/flac_lpc_cost.py [--reps 15] [--json profiles/flac_lpc_cost.json]
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--phonemes", type=int, default=256)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.flac import FlacConfig
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_inputs, synth_state_dict

    med = lambda v: float(np.median(v))      # noqa: E731
    eng = EVEngine(precision="mx")
    eng.load_blob(*pack_state_dict(synth_state_dict(0, "bench")))
    utts = synth_inputs(1, [args.phonemes] * args.batch, None)
    out = eng.synthesize(utts, want_int16=True)
    lens = out["mel_lens"].astype(np.int64) * int(eng.shapes.upsample_factor)
    wall = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.synthesize(utts, want_int16=True)
        wall.append((time.perf_counter() - t0) * 1e3)
    res = dict(reps=args.reps, batch=args.batch, samples=int(lens.sum()), synthesize_wall_ms_median=med(wall[2:]), data="seeded synthetic weights (not speech)")
    d16 = torch.from_numpy(out["wav_i16"]).cuda()
    torch.cuda.synchronize()

    def timed(B, ln, fc):
        run = lambda: eng.flac_raw(B, d16.data_ptr(), True, ln, fc, _ffi.EV_FLAG_DEVICE_INPUTS)      # noqa: E731
        run()
        run()
        w, tot, per = [], [], {}
        for _ in range(args.reps):
            t0 = time.perf_counter()
            run()
            w.append((time.perf_counter() - t0) * 1e3)
        eng.set_profiling(True)
        for _ in range(args.reps):
            run()
            recs = eng.launch_records()
            tot.append(sum(r["ms"] for r in recs))
            for r in recs:
                per.setdefault(r["name"], []).append(r["ms"])
        eng.set_profiling(False)
        sizes = np.diff(eng.flac_to_numpy(run())["stream_offsets"])
        return dict(call_wall_ms_median=med(w), kernels_ms_median=med(tot), kernels_ms_min=min(tot), kernels_ms_max=max(tot),
                    **{k + "_ms_median": med(v) for k, v in per.items()}), sizes

    B = len(lens)
    res["ev_flac"], base = timed(B, lens, FlacConfig())
    res["stream_over_pcm"] = float(base.sum() / (2.0 * lens.sum()))
    for L in (0, 8, 12):
        for md5 in (False, True):
            if L == 0 and not md5:
                continue
            row, sizes = timed(B, lens, FlacConfig(max_lpc_order=L, md5=md5))
            if L and not md5:
                r = sizes / base
                row.update(ratio_worst=float(r.max()), ratio_median=float(np.median(r)))
            res["ev_flac_lpc_order%d%s" % (L, "_md5" if md5 else "")] = row
    for sec in (30, 120, None):
        n = int(lens.sum()) if sec is None else min(sec * 16000, int(lens.sum()))
        row, _ = timed(1, np.array([n], np.int64), FlacConfig(max_lpc_order=8, md5=True))
        res["document_%d_samples_order8_md5" % n] = row
    eng.close()
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
