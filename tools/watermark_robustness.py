#!/usr/bin/env python3
"""How well the watermark survives, measured on the CPU with the oracles of tests/ alone (no device code runs here): z, bit errors, the SNR
(tests/compare_oracle.py) and the mel-cepstral distortion (tests/score_oracle.py, no warp) of marked against unmarked audio, over

    length 1 / 2 / 4 / 8 / 16 s  x  strength 0.25 / 0.5 / 1 / 2 dB  x  nbits 0 / 8 / 16  x  plain and the telephone chain
    (loudness to -16 LUFS as the limiter's pre-gain -> limiter -> 8 kHz mu-law -> G.711 decode -> back to 16 kHz)

on the two fixtures of the tests, on a harmonic signal with a syllable-rate tremolo and a wide pitch sweep (the case the detector's contrast is
weak against) and, where tests/golden/watermark/vocoder_seeded.npz exists (tools/watermark_cost.py --dump-vocoder writes it on the GPU), on
the vocoder's waveform under the seeded weights.  Recorded, not gated: nothing here can be derived.  The summary names, per signal, the shortest
length from which every row at 1 dB clears 1.25 x the threshold.

    python tools/watermark_robustness.py [--json profiles/watermark_robustness.json] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR, KEY = 16000, 0x5EED1234
PAYLOAD = {0: 0, 8: 0xA5, 16: 0xBEEF}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="4 s and 1 dB only: a rehearsal")
    args = ap.parse_args()
    import numpy as np
    import compare_oracle as co
    import deliver_oracle as dl
    import features_oracle as fo
    import limit_oracle as lim
    import loudness_oracle as lo
    import resample_oracle as ro
    import score_oracle as so
    import watermark_oracle as wo
    from emotivoice_amd.limiter import pre_gain
    from emotivoice_amd.loudness import LoudnessConfig

    def telephone(y):
        g, _ = pre_gain(lo.measure(y, SR)["loudness"], LoudnessConfig(target_lufs=-16.0).validate())
        law = dl.deliver(lim.limit(y, gain_in=g)["wav"], SR, 8000, dl.ULAW)["data"]
        h, up, down, _ = ro.design(8000, SR)
        return ro.resample32(wo.ulaw_decode(law), h, up, down)

    signals = dict(speech_like=lambda n: wo.speech_like(3, n), harmonic_rich=lambda n: wo.harmonic_rich(3, n),
                   harmonic_fast_modulation=lambda n: wo.harmonic_rich(3, n, vibrato_hz=25.0, vibrato_period=13000.0, tremolo=0.4, tremolo_period=4000.0))
    voc = os.path.join(ROOT, "tests", "golden", "watermark", "vocoder_seeded.npz")
    if os.path.exists(voc):
        v = np.load(voc)["wav"].astype(np.float32) / np.float32(32768.0)
        signals["vocoder_seeded"] = lambda n: v[:n]
    lengths, strengths = ((4,), (1.0,)) if args.quick else ((1, 2, 4, 8, 16), (0.25, 0.5, 1.0, 2.0))
    basis = so.design(80, 13)
    rows = []
    for name, make in signals.items():
        for secs in lengths:
            x = make(secs * SR)
            if x.size < secs * SR:
                continue
            mel_x = fo.features64(x)["mel"]
            for db in strengths:
                for nbits in (0, 8, 16):
                    y = wo.embed64(x, KEY, nbits, PAYLOAD[nbits], db).astype(np.float32)
                    cmp = co.compare_segment(y, x[:y.size])
                    mcd = so.score([fo.features64(y)["mel"]], [mel_x[:, :y.size // 256 + 1]], linear=True, basis=basis)["mcd_db"][0]
                    for chain, heard, clean in (("plain", y, x), ("telephone", telephone(y), None)):
                        d = wo.detect(heard, KEY, nbits)
                        errs = bin(d["payload"] ^ PAYLOAD[nbits]).count("1")
                        unmarked = wo.detect(x if clean is not None else telephone(x), KEY, nbits)["z"] if nbits == 0 else None
                        rows.append(dict(signal=name, seconds=secs, strength_db=db, nbits=nbits, chain=chain, z=round(d["z"], 3), offset=d["offset"],
                                         present=d["present"], clears_margin=bool(d["z"] >= 1.25 * wo.THRESHOLD), bit_errors=errs,
                                         z_unmarked=None if unmarked is None else round(unmarked, 3),
                                         snr_db=round(float(-20.0 * np.log10(cmp["rel_l2"])), 2), mcd_db=round(float(mcd), 4)))
                        print(rows[-1], flush=True)
    summary = {}
    for name in signals:
        for db in strengths:
            ok = [s for s in lengths if all(r["clears_margin"] and r["bit_errors"] == 0 for r in rows
                                            if r["signal"] == name and r["strength_db"] == db and r["nbits"] == 0 and r["seconds"] >= s)
                  and any(r["signal"] == name and r["seconds"] == s for r in rows)]
            summary["%s at %g dB, presence only" % (name, db)] = dict(shortest_seconds_from_which_every_row_clears_1_25_x_threshold=min(ok) if ok else None)
        for nbits in (8, 16):
            ok = [s for s in lengths if all(r["clears_margin"] and r["bit_errors"] == 0 for r in rows
                                            if r["signal"] == name and r["strength_db"] == 1.0 and r["nbits"] == nbits and r["seconds"] >= s)
                  and any(r["signal"] == name and r["seconds"] == s for r in rows)]
            summary["%s at 1 dB, %d bits read without error" % (name, nbits)] = dict(shortest_seconds=min(ok) if ok else None)
    out = dict(threshold=wo.THRESHOLD, margin=1.25 * wo.THRESHOLD, key=KEY, payloads={str(k): v for k, v in PAYLOAD.items()}, rows=rows, summary=summary,
               not_verified=["nobody has listened to any of these signals", "synthetic signals and a seeded vocoder, not speech",
                             "no mp3, Opus or acoustic re-recording", "one key"])
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
