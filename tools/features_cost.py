#!/usr/bin/env python3
"""Cost of ev_features at 32 utterances x 1024 frames (262 143 samples each, device input): the "total" region (ev_get_timing), the launch
records with profiling on and the wall time per call with it off -- and, for comparison only, the same handle's ev_align on that mel
(32 x 256 synthetic phonemes, EV_FLAG_DEVICE_MEL) next to the 3.7 ms INTEGRATION.md gives for ev_align at this size.

    python tools/features_cost.py [--reps 10] [--json out.json]
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
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_inputs, synth_state_dict

    eng = EVEngine(device_id=0)
    eng.load_blob(*pack_state_dict(synth_state_dict(0, "bench")))
    eng.features_setup()
    B, N, T = 32, 256, 1024
    L = (T - 1) * 256 + 255
    rng = np.random.default_rng(0)
    wav = torch.from_numpy((0.3 * rng.standard_normal(B * L)).clip(-1, 1).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    lens = np.full(B, L, np.int64)
    utts = synth_inputs(1, [N] * B, [0] * B)
    ling = np.concatenate([u["ling"] for u in utts])
    spk = np.zeros(B, np.int64)
    style = np.ascontiguousarray(np.stack([u["style"] for u in utts]))
    content = np.ascontiguousarray(np.stack([u["content"] for u in utts]))
    cu = np.arange(B + 1, dtype=np.int32) * N

    def feats():
        return eng.features_raw(B, wav.data_ptr(), False, lens, 0.0, 1.0, _ffi.EV_FLAG_DEVICE_INPUTS)

    def align(f):
        return eng.align_raw(B, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data, f.mel, False,
                             np.full(B, T, np.int32), None, f.energy, _ffi.EV_FLAG_DEVICE_MEL)

    f = feats()
    assert f.total_frames == B * T
    align(f)
    total, recs, atotal = [], None, []
    eng.set_profiling(True)
    for _ in range(args.reps):
        f = feats()
        total.append(eng.timings()["total"])
        recs = eng.launch_records()
        align(f)
        atotal.append(eng.timings()["total"])
    eng.set_profiling(False)
    wall = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        feats()
        wall.append((time.perf_counter() - t0) * 1e3)
    med = lambda x: float(np.median(x)) if x else None      # noqa: E731
    for r in recs:
        r["tflops"] = r["flops"] / (r["ms"] * 1e9) if r["ms"] > 0 else None
    out = dict(workload="ev_features: %d x %d frames (%d samples each), device input" % (B, T, L), reps=args.reps,
               total_ms_median=med(total), wall_ms_median=med(wall), launches=recs,
               align_total_ms_median=med(atotal), align_ms_integration_md=3.7)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
