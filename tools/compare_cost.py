#!/usr/bin/env python3
"""Cost of the precision guard (seeded weights): one ``ev_compare`` on device signals at a few sizes -- bytes moved (8 per element: both signals
read once), the hipEvent time of its two kernels (profiling on, median over --reps after a warm-up) and the rate that gives, with 16-byte
aligned chunks (float4 loads staged through LDS) and with the signals shifted by one element (element-wise loads) -- and the wall time
of one ``choose_precision`` on the default probe and ladder, against the wall time of building and loading one plain engine (what a load costs
without the guard).

    python tools/compare_cost.py [--reps 10] [--json profiles/compare_cost.json]
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
    ap.add_argument("--sizes", default="65536,1048576,16777216,134217728", help="elements per signal, one segment each")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "compare_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from emotivoice_amd import _ffi
    from emotivoice_amd.config import EVShapes
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.precision_guard import choose_precision
    from emotivoice_amd.synthetic import synth_state_dict

    med = lambda x: float(np.median(x))      # noqa: E731
    eng = EVEngine(device_id=0)

    def timed(pa, pb, lens):
        run = lambda: eng.compare_raw(1, pa, pb, lens, _ffi.EV_FLAG_DEVICE_INPUTS)      # noqa: E731
        run()
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
        return med(wall), med(kern["compare_chunks"]), med(kern["compare_finish"])

    sizes = []
    for n in [int(x) for x in args.sizes.split(",")]:
        b = torch.randn(n, device="cuda") * 0.1
        a = b + 1e-4 * torch.randn(n, device="cuda")
        torch.cuda.synchronize()
        wall, chunks_ms, finish_ms = timed(a.data_ptr(), b.data_ptr(), np.array([n], np.int64))
        # the same signals from their second element on: no chunk is 16-byte aligned, so every one takes the element-wise path
        _, scalar_ms, _ = timed(a.data_ptr() + 4, b.data_ptr() + 4, np.array([n - 1], np.int64))
        sizes.append(dict(elements=n, bytes_read=8 * n, call_wall_ms_median=wall, compare_chunks_ms_median=chunks_ms,
                          compare_finish_ms_median=finish_ms, compare_chunks_gb_per_s=8 * n / chunks_ms / 1e6,
                          compare_chunks_misaligned_ms_median=scalar_ms, compare_chunks_misaligned_gb_per_s=8 * (n - 1) / scalar_ms / 1e6))
        del a, b
    eng.close()

    shapes = EVShapes()
    blob = pack_state_dict(synth_state_dict(0, "parity"), pe_len=4096)
    choose_precision(shapes, blob)          # warm-up: code objects, allocator
    guard_ms, load_ms, rep = [], [], None
    for _ in range(max(3, args.reps // 3)):
        t0 = time.perf_counter()
        rep = choose_precision(shapes, blob)
        guard_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        e = EVEngine(shapes, 0)
        e.load_blob(*blob)
        load_ms.append((time.perf_counter() - t0) * 1e3)
        e.close()
    res = dict(reps=args.reps, ev_compare=sizes, choose_precision_wall_ms_median=med(guard_ms), plain_engine_create_and_load_wall_ms_median=med(load_ms),
               report=rep.as_dict(), report_line=rep.line())
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(args.json), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
