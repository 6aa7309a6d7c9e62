#!/usr/bin/env python3
"""Cost of long-form synthesis at 4 documents of 8 sentences of 256 phonemes (seeded weights): ``synthesize_long`` (one ev_synthesize, one
ev_stitch on its device waveform, one D2H copy of the documents) against ``synthesize`` + the D2H copy of every waveform + the numpy oracle of
the same stitching on the host.  Wall time per call around work that ends in a device synchronise, after a warm-up; with profiling on, the
"total" region of the ev_stitch call alone (ev_get_timing) and its launch records.

    python tools/stitch_cost.py [--reps 10] [--json profiles/stitch_cost.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--docs", type=int, default=4)
    ap.add_argument("--sentences", type=int, default=8)
    ap.add_argument("--phonemes", type=int, default=256)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "stitch_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import stitch_oracle as so
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.longform import StitchConfig, plan_document
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_inputs, synth_state_dict

    eng = EVEngine(device_id=0)
    blob, man = pack_state_dict(synth_state_dict(0, "parity"), pe_len=4096)
    eng.load_blob(blob, man)
    D, K = args.docs, args.sentences
    utts = synth_inputs(3, [args.phonemes] * (D * K))
    documents = [dict(utts=utts[d * K:(d + 1) * K], pauses=["sentence"] * (K - 1)) for d in range(D)]
    cfg = StitchConfig(want_int16=True)
    seg_doc, pause_after = plan_document([d for d in range(D) for _ in range(K)], (["sentence"] * (K - 1) + [None]) * D)
    tab = so.ramp_table(cfg.samples("fade"))
    med = lambda x: float(np.median(x))      # noqa: E731

    def device():
        return eng.synthesize_long(documents, config=cfg)

    def host():
        wavs = eng.synthesize(utts)["wav_list"]
        r = so.stitch(wavs, seg_doc, pause_after, tab, trim_frac=np.float32(cfg.trim_frac), keep=cfg.samples("keep"))
        return [so.to_i16(d) for d in r["docs"]]

    out, ref = device(), host()          # warm-up of both, and the same documents
    same = all(np.array_equal(a, b) for a, b in zip(out["documents"], ref))
    wall_dev, wall_host, stitch_total, recs = [], [], [], None
    for _ in range(args.reps):           # alternating, so that drift hits both
        t0 = time.perf_counter()
        device()
        wall_dev.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        host()
        wall_host.append((time.perf_counter() - t0) * 1e3)
    eng.set_profiling(True)
    for _ in range(args.reps):
        device()
        stitch_total.append(eng.timings()["total"])          # the last call of synthesize_long is ev_stitch
        recs = eng.launch_records()
    eng.set_profiling(False)
    samples = int(out["doc_lens"].sum())
    res = dict(workload="synthesize_long: %d documents x %d sentences x %d phonemes, int16 out" % (D, K, args.phonemes), reps=args.reps,
               samples_out=samples, seconds_of_audio=samples / 16000.0, equal_to_host_oracle=bool(same),
               synthesize_long_wall_ms_median=med(wall_dev), synthesize_d2h_numpy_wall_ms_median=med(wall_host),
               ev_stitch_total_ms_median=med(stitch_total), ev_stitch_launches=recs)
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
