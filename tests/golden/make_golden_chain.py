#!/usr/bin/env python3
"""Records tests/golden/chain/transcripts.json: what the output chain of EVEngine.synthesize / synthesize_long asks of the library, call by call,
and what it returns, for the cross product of the stage arguments and for four sequences of calls on one engine (the setup caches).

The library is the stand-in with every entry (tests/fake_evhip.py: DenoiseLib + DeliverLib) and only the public API is used, so the script runs
on any commit that has both.  The committed file was recorded from the commit BEFORE the chain became emotivoice_amd/output_chain.py (its
``recorded_from`` says which); tests/test_chain_transcripts.py holds the code under test to it.  Re-record only from a commit whose chain is
known good:

    python tests/golden/make_golden_chain.py [--out tests/golden/chain/transcripts.json] [--full /some/path/outside/the/repository.txt]

Per run: the call names (without the D2H copies), a digest of the full transcript (the ``repr`` of every log entry, ev_memcpy_d2h sources and
byte counts included) and a digest of the returned dict (keys in order, dtypes, shapes, bytes, recursively); for a rejected call the exception's
type and message, and the transcript must be empty.  ``--full`` writes the text behind the digests, to diff a mismatch by hand."""
import argparse
import hashlib
import itertools
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fake_evhip as fk  # noqa: E402
from emotivoice_amd import _ffi  # noqa: E402
from emotivoice_amd.delivery import DeliveryConfig  # noqa: E402
from emotivoice_amd.denoise import DenoiseConfig  # noqa: E402
from emotivoice_amd.longform import StitchConfig  # noqa: E402
from emotivoice_amd.prosody import Prosody  # noqa: E402

TOKENS = (3, 5, 2)
DENOISE = dict(none=lambda: None, s01=lambda: 0.1, cfg=lambda: DenoiseConfig(strength=0.2, bias=np.full(513, 0.25, np.float32), report=True))
DELIVERY = dict(none=lambda: None, r8000=lambda: 8000, ulaw24000=lambda: DeliveryConfig(24000, "ulaw"),
                dither48000=lambda: DeliveryConfig(48000, "s16", dither=True))
FLAC = dict(none=None, all=True, mask=[True, False, True])


class FullLib(fk.DenoiseLib, fk.DeliverLib):
    pass


def utterances():
    return [dict(ling=np.arange(t) + 1, speaker=b, style=np.zeros(768, np.float32), content=np.zeros(768, np.float32)) for b, t in enumerate(TOKENS)]


def documents():
    u = utterances()
    return [dict(utts=u[:2]), (u[2:], None)]


def ramps():
    return [fk.ramp(600), fk.ramp(1024)]


def describe(x) -> str:
    """A returned value as text: keys in order, dtypes, shapes and a digest of the bytes, recursively."""
    if isinstance(x, dict):
        return "{" + ", ".join("%r: %s" % (k, describe(v)) for k, v in x.items()) + "}"
    if isinstance(x, (list, tuple)):
        return type(x).__name__ + "[" + ", ".join(describe(v) for v in x) + "]"
    if isinstance(x, np.ndarray):
        return "ndarray(%s, %s, %s)" % (x.dtype.str, x.shape, hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16])
    if isinstance(x, np.generic):
        return "%s(%r)" % (x.dtype.str, x.item())
    if isinstance(x, (bytes, bytearray)):
        return "bytes(%d, %s)" % (len(x), hashlib.sha256(bytes(x)).hexdigest()[:16])
    return "%s(%r)" % (type(x).__name__, x)


def digest(text: str) -> str:
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def new_engine():
    lib = FullLib()
    saved = _ffi.lib
    _ffi.lib = lambda: lib
    try:
        from emotivoice_amd.engine import EVEngine
        eng = EVEngine()
    finally:
        _ffi.lib = saved
    return eng, lib


def attempt(lib, call, full, title):
    """One call: -> its entry, from the log entries it added."""
    n = len(lib.log)
    try:
        out = call()
    except Exception as e:      # noqa: BLE001 -- the rejection is what is recorded
        entry = dict(error=[type(e).__name__, str(e)], names=" ".join(x["name"] for x in lib.log[n:]))
        text = "raised %s: %s" % tuple(entry["error"])
    else:
        entry = dict(names=" ".join(x["name"] for x in lib.log[n:] if x["name"] != "ev_memcpy_d2h"), out=digest(describe(out)))
        text = describe(out)
    log = "\n".join(repr(x) for x in lib.log[n:])
    entry["log"] = digest(log)
    if full is not None:
        full.write("==== %s\n%s\n---- returned\n%s\n" % (title, log, text))
    return entry


def product(full=None) -> dict:
    """The cross product of the stage arguments, a fresh engine per run: 288 synthesize runs and 192 synthesize_long runs."""
    runs = {}
    for long_form in (False, True):
        flacs = ("none", "all") if long_form else tuple(FLAC)
        for dn, ld, lm, dl, i16, fl in itertools.product(DENOISE, (None, -16.0), (None, -1.0), DELIVERY, (False, True), flacs):
            kw = dict(denoise=DENOISE[dn](), loudness=ld, limiter=lm, delivery=DELIVERY[dl](), flac=FLAC[fl])
            eng, lib = new_engine()
            if long_form:
                call = lambda: eng.synthesize_long(documents(), config=StitchConfig(want_int16=i16), **kw)      # noqa: E731
            else:
                call = lambda: eng.synthesize(utterances(), want_int16=i16, **kw)      # noqa: E731
            name = "%s denoise=%s loudness=%s limiter=%s delivery=%s want_int16=%d flac=%s" % ("synthesize_long" if long_form else "synthesize", dn, ld, lm, dl, i16, fl)
            runs[name] = attempt(lib, call, full, name)
            eng.close()
    return runs


def sequences(full=None) -> dict:
    """Calls in a row on one engine each: what the setup caches make of them."""
    ulaw = DeliveryConfig(24000, "ulaw")
    steps = {
        "1 delivery setups": lambda e: [
            ("synthesize(delivery=8000)", lambda: e.synthesize(utterances(), delivery=8000)),
            ("deliver(w, 8000)", lambda: e.deliver(ramps(), 8000)),
            ("deliver(w, ulaw 24000)", lambda: e.deliver(ramps(), ulaw)),
            ("synthesize(delivery=ulaw 24000)", lambda: e.synthesize(utterances(), delivery=ulaw)),
            ("synthesize(delivery=8000) again", lambda: e.synthesize(utterances(), delivery=8000))],
        "2 denoise setups and the measured bias": lambda e: [
            ("synthesize(denoise=0.1)", lambda: e.synthesize(utterances(), denoise=0.1)),
            ("denoise(w, 0.1)", lambda: e.denoise(ramps(), 0.1)),
            ("denoise(w, 0.2)", lambda: e.denoise(ramps(), 0.2)),
            ("synthesize_long(denoise=0.2, loudness=-16.0)", lambda: e.synthesize_long(documents(), denoise=0.2, loudness=-16.0)),
            ("synthesize(denoise=True)", lambda: e.synthesize(utterances(), denoise=True))],
        "3 prosody": lambda e: [
            ("synthesize(prosody, denoise=0.1, limiter=True)", lambda: e.synthesize(utterances(), prosody=Prosody(speed=1.0), denoise=0.1, limiter=True))],
        "4 vocoder=False": lambda e: [
            ("synthesize(vocoder=False, %s)" % k, lambda k=k, v=v: e.synthesize(utterances(), vocoder=False, **{k: v}))
            for k, v in (("flac", True), ("limiter", -1.0), ("loudness", -16.0), ("delivery", 8000), ("denoise", 0.1))],
    }
    out = {}
    for title, make in steps.items():
        eng, lib = new_engine()
        out[title] = dict(steps=[dict(call=name, **attempt(lib, call, full, "%s: %s" % (title, name))) for name, call in make(eng)],
                          counts={k: len(lib.calls(k)) for k in ("ev_deliver_setup", "ev_denoise_setup", "ev_denoise_bias")})
        eng.close()
    return out


def record(full=None) -> dict:
    return dict(product=product(full), sequences=sequences(full))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--out", default=os.path.join(HERE, "chain", "transcripts.json"))
    p.add_argument("--full", default=None, help="also write the full transcripts and returned values as text (1.4 MB) to this path, outside the repository")
    args = p.parse_args(argv)
    if args.full:
        with open(args.full, "w") as f:
            got = record(f)
    else:
        got = record()
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    got = dict(recorded_from=head or "unknown", **got)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        one = lambda v: json.dumps(v, separators=(",", ":"))      # noqa: E731  one run, one line
        f.write('{"recorded_from":%s,\n"product":{\n%s\n},\n"sequences":{\n%s\n}}\n' % (
            one(got["recorded_from"]), ",\n".join("%s:%s" % (one(k), one(v)) for k, v in got["product"].items()),
            ",\n".join("%s:%s" % (one(k), one(v)) for k, v in got["sequences"].items())))
    rejected = [k for k, v in got["product"].items() if "error" in v]
    print("%d runs, %d rejected; wrote %s" % (len(got["product"]), len(rejected), args.out))


if __name__ == "__main__":
    main()
