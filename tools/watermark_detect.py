#!/usr/bin/env python3
"""Did this recording come from us?  Reads a PCM .wav with the standard ``wave`` module and runs ev_watermark_detect on the device with the
operator's key; a recording at another rate than 16 kHz is brought there by ev_resample first.  Prints one JSON line: z, present, offset and,
with --nbits, the payload.  present = z >= threshold (6.25: a false-alarm bound of 5e-7 per segment and key IF the hash's bits were independent,
which is not proven); see emotivoice_amd/watermark.py for what is not verified.  Exit status 0 = present, 1 = absent.

    python tools/watermark_detect.py FILE.wav --key 0x5EED1234 [--nbits 8] [--threshold 6.25]
"""
import argparse
import json
import os
import sys
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_wav(path):
    """(int16 mono samples, sample rate) of a 16-bit PCM file; several channels are averaged."""
    import numpy as np
    with wave.open(path, "rb") as fh:
        if fh.getsampwidth() != 2 or fh.getcomptype() != "NONE":
            raise SystemExit("%s: only 16-bit PCM is read (sample width %d, compression %s)" % (path, fh.getsampwidth(), fh.getcomptype()))
        ch, sr = fh.getnchannels(), fh.getframerate()
        x = np.frombuffer(fh.readframes(fh.getnframes()), "<i2")
    if ch > 1:
        x = np.round(x.reshape(-1, ch).astype(np.float64).mean(axis=1)).astype(np.int16)
    return np.ascontiguousarray(x), sr


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("--key", required=True, type=lambda s: int(s, 0))
    ap.add_argument("--nbits", type=int, default=0)
    ap.add_argument("--threshold", type=float, default=None)
    args = ap.parse_args(argv)
    wav, sr = read_wav(args.file)
    from emotivoice_amd.engine import EVEngine
    eng = EVEngine(device_id=0)
    try:
        rep = eng.watermark_detect([wav], args.key, args.nbits, sample_rate=sr, threshold=args.threshold)["report"][0]
    finally:
        eng.close()
    rep.update(file=args.file, sample_rate=sr, seconds=wav.size / float(sr), key=args.key, nbits=args.nbits)
    if not args.nbits:
        rep.pop("bits"), rep.pop("payload"), rep.pop("bit_z")
    print(json.dumps(rep))
    return 0 if rep["present"] else 1


if __name__ == "__main__":
    sys.exit(main())
