#!/usr/bin/env python3
"""Cost of objective scoring: ``ev_score_load`` (both sides) and ``ev_score`` on features already on the device, per kernel (hipEvents around every
launch, profiling on; the two sides' loads summed) and per call (a host clock around calls that end in a device synchronise, profiling off); median, minimum and maximum over
--reps after a warm-up of every shape.  Workloads: 32 pairs of 1000 x 1000 frames, and one pair of 4096 x 4096.  The features are log-mel-like noise,
not speech: the cost does not depend on the values.

    python tools/bench_score.py [--reps 7] [--json profiles/score_cost.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ((32, 1000, 1000), (1, 4096, 4096))
N_MELS, N_CEPS = 80, 13


def stats(x):
    import numpy as np
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "score_cost.json"))
    args = ap.parse_args(argv)
    if args.reps < 5:
        ap.error("--reps must be at least 5: the spread is part of the result")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_score needs a GPU: no time is reported without one")
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine

    DEV = _ffi.EV_FLAG_DEVICE_INPUTS
    eng = EVEngine(device_id=0)
    rows = []
    for B, Ta, Tb in WORKLOADS:
        rng = np.random.default_rng(B * 7 + Ta)
        sides = []
        for T in (Ta, Tb):
            mel = torch.from_numpy((rng.standard_normal(B * N_MELS * T) * 1.5 - 4.0).astype(np.float32)).cuda()
            f0 = torch.from_numpy((120.0 * np.exp2(rng.uniform(-0.5, 0.5, B * T))).astype(np.float32)).cuda()
            sides.append((mel, f0, np.full(B, T, np.int32)))
        torch.cuda.synchronize()

        def load_side(side):
            mel, f0, lens = sides[side]
            eng.score_load_raw(side, B, N_MELS, N_CEPS, mel.data_ptr(), lens, f0.data_ptr(), DEV)

        def load():
            load_side(0)
            load_side(1)

        for linear in (False, True):
            load(); eng.score_raw(linear)          # noqa: E702 -- the warm-up of every shape
            t_load, t_score = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter(); load(); t_load.append((time.perf_counter() - t0) * 1e3)                    # noqa: E702
                t0 = time.perf_counter(); eng.score_raw(linear); t_score.append((time.perf_counter() - t0) * 1e3)    # noqa: E702
            kern = {}
            eng.set_profiling(True)
            load(); eng.score_raw(linear)          # noqa: E702
            for _ in range(args.reps):
                per_rep = {}
                for run in (lambda: load_side(0), lambda: load_side(1), lambda: eng.score_raw(linear)):
                    run()
                    for r in eng.launch_records():          # the records of the call that just returned
                        per_rep[r["name"]] = per_rep.get(r["name"], 0.0) + r["ms"]          # both sides' loads, and every pass of a kernel, summed
                for k, v in per_rep.items():
                    kern.setdefault(k, []).append(v)
            eng.set_profiling(False)
            res = eng.last_score
            K = int(res.path_offsets[B])
            row = dict(pairs=B, frames_a=Ta, frames_b=Tb, linear=linear, n_mels=N_MELS, n_ceps=N_CEPS, path_cells=K, load_both_sides_ms=stats(t_load),
                       score_ms=stats(t_score), kernels_ms={k: stats(v) for k, v in kern.items()})
            if not linear:          # one wavefront per pair: all pairs of a launch run side by side (B <= the chip's 256 CUs x 8 waves per SIMD x 4)
                row["dtw_ms_per_pair"] = row["kernels_ms"]["score_dtw"]["median"]
                row["dtw_pairs_concurrent"] = B
                row["dtw_cells_per_us_per_wave"] = Ta * Tb / (row["dtw_ms_per_pair"] * 1e3)
            rows.append(row)
    eng.close()
    out = dict(reps=args.reps, signal="log-mel-like noise (not speech)", input="device fp32 mel and f0", rows=rows)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
