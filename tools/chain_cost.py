#!/usr/bin/env python3
"""Host cost of the output chain per call (emotivoice_amd/output_chain.py), which bench.py does not pass through: the wall time of
``synthesize(utts, loudness=-16.0, limiter=-1.0, delivery=8000, flac=True)``, or with ``--long`` of synthesize_long of one two-sentence document
with the same stages -- per process the median of ``--calls`` calls after ``--warmup`` warm-up calls, in microseconds, min and p90 beside it.

    python tools/chain_cost.py --standin            the Python alone, against the stand-in library of tests/fake_evhip.py (no GPU)
    python tools/chain_cost.py [--long]             the real library, synthetic weights (MI355X)

``--package DIR`` takes emotivoice_amd from another checkout (with EVHIP_LIB naming this one's library): an A/B of the Python alone is one fresh
process per side and round, alternating.  profiles/output_chain_ab.txt holds one."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--standin", action="store_true")
    p.add_argument("--long", action="store_true")
    p.add_argument("--package", default=ROOT)
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--label", default="")
    args = p.parse_args(argv)
    sys.path[:0] = [os.path.abspath(args.package), os.path.join(ROOT, "tests")]
    from emotivoice_amd import _ffi
    if args.standin:
        import fake_evhip as fk
        lib = type("FullLib", (fk.DenoiseLib, fk.DeliverLib), {})()
        _ffi.lib = lambda: lib
        utts = [dict(ling=np.arange(t) + 1, speaker=b, style=np.zeros(768, np.float32), content=np.zeros(768, np.float32)) for b, t in enumerate((3, 5, 2))]
    from emotivoice_amd.engine import EVEngine
    eng = EVEngine()
    if not args.standin:
        from emotivoice_amd.packer import pack_state_dict
        from emotivoice_amd.synthetic import synth_inputs, synth_state_dict
        eng.load_blob(*pack_state_dict(synth_state_dict(0, "parity")))
        utts = synth_inputs(51, [24, 24], [3, 3] if args.long else [3, 8])
    stages = dict(loudness=-16.0, limiter=-1.0, delivery=8000, flac=True)
    call = (lambda: eng.synthesize_long([dict(utts=utts[:2], pauses=["comma"])], **stages)) if args.long else (lambda: eng.synthesize(utts, **stages))
    us = []
    for i in range(args.warmup + args.calls):
        if args.standin:
            del lib.log[:]      # the stand-in's transcript is not part of the cost
        t0 = time.perf_counter()
        call()
        us.append((time.perf_counter() - t0) * 1e6)
    us = np.sort(us[args.warmup:])
    print("%s %s median %.2f us (min %.2f, p90 %.2f) over %d calls" % (args.label or os.path.abspath(args.package), "synthesize_long" if args.long else "synthesize",
                                                                      np.median(us), us[0], us[int(0.9 * len(us))], len(us)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
