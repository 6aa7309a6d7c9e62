"""StretchLib: the stand-in library of tests/fake_evhip.py with an ev_stretch, for tests/test_stretch_chain.py.

The stand-in ev_stretch HALVES the samples and gives segment b its new length by repeating or cutting the segment (np.resize): trivial
arithmetic that tells the stage apart from the others and makes every later stage's input length visible.  FakeLib and DenoiseLib themselves keep
raising on any stretch call, so the chain without ``stretch=`` is held to the calls it made before the stage existed."""
import ctypes as C

import numpy as np

import fake_evhip as fk
from fake_evhip import _cfg, _host

HALF = np.float32(0.5)      # what the stand-in ev_stretch multiplies by


def stretched(x, lens, lens_out):
    """What the stand-in makes of the packed x."""
    offs = np.concatenate([[0], np.cumsum(lens)])
    return np.concatenate([np.resize(x[a:a + n], int(m)) * HALF for a, n, m in zip(offs[:-1], lens, lens_out)]).astype(np.float32)


class StretchLib(fk.DenoiseLib, fk.DeliverLib):
    def ev_stretch(self, h, B, wav, is_i16, lens, lens_out, cfg, flags, ref):
        ln, lo = _host(lens, C.c_int64, B), _host(lens_out, C.c_int64, B)
        x, src = self._read(wav, is_i16, ln)
        self.log.append(dict(name="ev_stretch", B=B, flags=int(flags), cfg=_cfg(cfg), lens=ln.tolist(), lens_out=lo.tolist(), is_i16=int(is_i16), src=src))
        out = stretched(x, ln, lo)
        frames = ((lo + 255) // 256).astype(np.int32)
        res = ref._obj
        res.batch, res.total = B, int(lo.sum())
        return self._fill("stretch", ref, wav=out, wav_i16=fk.to_i16(out) if cfg is not None and cfg._obj.want_int16 else None, lens_out=lo,
                          offsets=np.concatenate([[0], np.cumsum(lo)]).astype(np.int64), frames=frames,
                          frame_offsets=np.concatenate([[0], np.cumsum(frames)]).astype(np.int64), deltas=np.zeros(int(frames.sum()), np.int16),
                          edge_frames=np.arange(B, dtype=np.int32), sum_dist=np.full(B, 7, np.uint64), nonfinite=np.zeros(B, np.int64))
