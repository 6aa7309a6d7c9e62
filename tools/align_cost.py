#!/usr/bin/env python3
"""Cost of ev_align at 32 utterances x 256 synthetic phonemes x 1024 mel frames (device inputs): the "total" region (ev_get_timing) and
the summed time per kernel family with profiling on, and the wall time per call with it off.

    python tools/align_cost.py [--reps 10] [--json out.json]
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
    B, N, T = 32, 256, 1024
    utts = synth_inputs(1, [N] * B, [0] * B)
    rng = np.random.default_rng(0)
    ling = torch.from_numpy(np.concatenate([u["ling"] for u in utts])).cuda()
    spk = torch.zeros(B, dtype=torch.int64, device="cuda")
    style = torch.from_numpy(np.stack([u["style"] for u in utts])).cuda()
    content = torch.from_numpy(np.stack([u["content"] for u in utts])).cuda()
    mel = torch.from_numpy(rng.standard_normal(B * 80 * T).astype(np.float32)).cuda()
    pf = torch.from_numpy(rng.standard_normal(B * T).astype(np.float32)).cuda()
    ef = torch.from_numpy(rng.standard_normal(B * T).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    cu = np.arange(B + 1, dtype=np.int32) * N
    lens = np.full(B, T, np.int32)

    def call():
        return eng.align_raw(B, ling.data_ptr(), cu, spk.data_ptr(), style.data_ptr(), content.data_ptr(), mel.data_ptr(), False, lens,
                             pf.data_ptr(), ef.data_ptr(), _ffi.EV_FLAG_DEVICE_INPUTS)

    call()
    total, fam = [], {}
    eng.set_profiling(True)
    for _ in range(args.reps):
        call()
        total.append(eng.timings()["total"])
        for s in eng.kernel_stats():
            fam.setdefault(s["name"], []).append((s["launches"], s["ms"]))
    eng.set_profiling(False)
    wall = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    med = lambda x: float(np.median(x)) if x else None      # noqa: E731
    out = dict(workload="ev_align: %d x %d phonemes x %d frames, device inputs" % (B, N, T), reps=args.reps,
               total_ms_median=med(total), wall_ms_median=med(wall),
               families={k: dict(launches=v[0][0], ms_median=med([m for _, m in v])) for k, v in sorted(fam.items(), key=lambda kv: -med([m for _, m in kv[1]]))})
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
