#!/usr/bin/env python3
"""Cost of ev_stretch on device input: 32 utterances x 16 s at speeds 0.8 and 1.25, one utterance of 1 s (latency) and one document of 10 minutes
(the serial search at its longest).  Per case the wsola_search and wsola_ola kernel times (the handle's launch records with profiling on), the
search's microseconds per frame, the overlap-add's GB/s, the "total" region and the wall time per call with profiling off.  For scale: one
synthesis step at batch 32, and the D2H copy of the batch's fp32 waveform -- the first step of the only other route, a loop on the host (no host
stretcher is installed to time the rest of it).  The sclk that rocm-smi shows right after the timed loop is recorded as the clock state of the run.

    python tools/stretch_cost.py [--reps 10] [--json profiles/stretch_cost.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=10).stdout
        m = re.search(r"sclk clock level: \S+ \((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


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
    from emotivoice_amd.stretch import plan_lengths
    from emotivoice_amd.synthetic import synth_inputs, synth_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("stretch_cost.py measures on the GPU: none found")
    eng = EVEngine(device_id=0)
    eng.load_blob(*pack_state_dict(synth_state_dict(0, "bench")))
    med = lambda x: float(np.median(x)) if len(x) else None      # noqa: E731
    rng = np.random.default_rng(0)

    def signal(n):      # harmonics with a drifting pitch under a little noise: the cost does not depend on the data, the lags do
        t = np.arange(n, dtype=np.float64)
        ph = 2 * np.pi * np.cumsum(110.0 + 40.0 * np.sin(2 * np.pi * t / 9000.0)) / 16000.0
        return (0.4 * np.sin(ph) + 0.2 * np.sin(2 * ph) + 0.1 * np.sin(3 * ph) + 0.01 * rng.standard_normal(n)).astype(np.float32)

    cases = []
    for name, B, L, speed, reps in (("batch", 32, 16 * 16000, 0.8, args.reps), ("batch", 32, 16 * 16000, 1.25, args.reps), ("latency", 1, 16000, 1.25, args.reps),
                                    ("document", 1, 600 * 16000, 1.25, max(2, args.reps // 3))):
        one = signal(L)
        host = np.ascontiguousarray(np.tile(one, B))
        wav = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        lens = np.full(B, L, np.int64)
        lens_out = plan_lengths(lens, [speed] * B)

        def call():
            return eng.stretch_raw(B, wav.data_ptr(), False, lens, lens_out, None, _ffi.EV_FLAG_DEVICE_INPUTS)

        for _ in range(2):
            res = call()
        frames = int(res.frame_offsets[B])
        figs = eng.stretch_to_numpy(res, skip_wav=True)
        total, kern = [], {}
        eng.set_profiling(True)
        for _ in range(reps):
            call()
            total.append(eng.timings()["total"])
            for r in eng.launch_records():
                kern.setdefault(r["name"], []).append(r)
        eng.set_profiling(False)
        wall = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        clock = sclk()
        kernels = {}
        for kname, rs in kern.items():
            ms = med([r["ms"] for r in rs])
            kernels[kname] = dict(ms_median=ms, gbytes_per_s=rs[0]["bytes"] / (ms * 1e6) if ms else None)
        search_ms = kernels.get("wsola_search", {}).get("ms_median")
        d2h = []
        for _ in range(max(2, reps // 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wav.cpu()
            d2h.append((time.perf_counter() - t0) * 1e3)
        cases.append(dict(case=name, workload="ev_stretch: %d x %d samples at speed %g, device input" % (B, L, speed), reps=reps, frames_total=frames,
                          frames_per_segment=frames // B, edge_frames=int(figs["edge_frames"].sum()), total_ms_median=med(total), wall_ms_median=med(wall),
                          wall_ms_min=float(min(wall)), wall_ms_max=float(max(wall)), kernels=kernels,
                          search_us_per_frame_of_a_segment=search_ms * 1e3 / (frames // B) if search_ms else None, sclk_mhz_after=clock,
                          d2h_of_the_input_ms_median=med(d2h)))
    # one synthesis step at batch 32, for scale
    utts = synth_inputs(1, [256] * 32, [0] * 32)
    from emotivoice_amd.packing import pack_utts
    ling, cu, spk, style, content = pack_utts(utts)
    step = []
    for i in range(args.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = eng.synthesize_raw(32, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data)
        if i >= 2:
            step.append((time.perf_counter() - t0) * 1e3)
    out = dict(cases=cases, synthesis_step=dict(workload="ev_synthesize: 32 x 256 phonemes, host inputs", wall_ms_median=med(step), seconds_of_audio=r.total_samples / 16000.0))
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
