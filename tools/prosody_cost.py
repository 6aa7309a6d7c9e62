#!/usr/bin/env python3
"""Cost of ev_synthesize_prosody over ev_synthesize at bench.py's configs[1] (32 x 256 synthetic phonemes, AM + vocoder, device inputs),
in one process: the "variance" region (ev_get_timing) and the prosody launches with profiling on, and the wall time per call with it off,
plain and identity-prosody calls alternating.

    python tools/prosody_cost.py [--reps 10] [--json out.json]
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
    from emotivoice_amd.prosody import pack_prosody
    from emotivoice_amd.synthetic import synth_inputs, synth_state_dict

    eng = EVEngine(device_id=0)
    eng.load_blob(*pack_state_dict(synth_state_dict(0, "bench")))
    B, N = 32, 256
    utts = synth_inputs(1, [N] * B, [0] * B)
    ling = torch.from_numpy(np.concatenate([u["ling"] for u in utts])).cuda()
    spk = torch.zeros(B, dtype=torch.int64, device="cuda")
    style = torch.from_numpy(np.stack([u["style"] for u in utts])).cuda()
    content = torch.from_numpy(np.stack([u["content"] for u in utts])).cuda()
    cu = np.arange(B + 1, dtype=np.int32) * N
    flags = _ffi.EV_FLAG_DEVICE_INPUTS
    ident = pack_prosody([None] * B, [N] * B, device=True)
    ptrs = (ling.data_ptr(), cu, spk.data_ptr(), style.data_ptr(), content.data_ptr())

    def plain():
        return eng.synthesize_raw(B, *ptrs, 1.0, flags)

    def pros():
        return eng.synthesize_prosody_raw(B, *ptrs, 1.0, ident, flags)

    a, b = eng.result_to_numpy(plain()), eng.result_to_numpy(pros())
    same = all(np.array_equal(a[k], b[k]) for k in ("wav", "mel", "durations"))
    names = ("prosody_tracks", "durations_prosody", "durations")
    var = {"plain": [], "prosody": []}
    launches = {n: [] for n in names}
    eng.set_profiling(True)
    for _ in range(args.reps):
        for tag, fn in (("plain", plain), ("prosody", pros)):
            fn()
            var[tag].append(eng.timings()["variance"])
            for r in eng.launch_records():
                if r["name"] in names:
                    launches[r["name"]].append(r["ms"])
    eng.set_profiling(False)
    wall = {"plain": [], "prosody": []}
    for _ in range(args.reps):
        for tag, fn in (("plain", plain), ("prosody", pros)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[tag].append((time.perf_counter() - t0) * 1e3)
    med = lambda x: float(np.median(x)) if x else None      # noqa: E731
    out = dict(workload="configs[1]: %d x %d phonemes, AM + vocoder, device inputs" % (B, N), reps=args.reps, identity_bitwise=bool(same),
               frames=int(a["mel_lens"].sum()),
               variance_ms_median={k: med(v) for k, v in var.items()}, launch_ms_median={k: med(v) for k, v in launches.items()},
               wall_ms_median={k: med(v) for k, v in wall.items()})
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
