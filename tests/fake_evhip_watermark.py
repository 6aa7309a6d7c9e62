"""WatermarkLib: the stand-in library of tests/fake_evhip_stretch.py with an ev_watermark, for tests/test_watermark_chain.py.

The stand-in ev_watermark TRIPLES the samples and cuts every segment to whole hops, as the real one does: trivial arithmetic that tells the stage
apart from the others.  FakeLib, DenoiseLib, DeliverLib and StretchLib themselves keep raising on any watermark call, so the chain without
``watermark=`` is held to the calls it made before the stage existed."""
import ctypes as C

import numpy as np

import fake_evhip as fk
import fake_evhip_stretch as fks
from fake_evhip import _cfg, _host

THREE = np.float32(3.0)      # what the stand-in ev_watermark multiplies by


def marked(x, lens):
    """What the stand-in makes of the packed x."""
    offs = np.concatenate([[0], np.cumsum(lens)])
    return np.concatenate([x[a:a + n // 256 * 256] * THREE for a, n in zip(offs[:-1], lens)]).astype(np.float32)


class WatermarkLib(fks.StretchLib):
    def ev_watermark(self, h, B, wav, is_i16, lens, cfg, payloads, nbits, strengths_db, flags, ref):
        ln = _host(lens, C.c_int64, B)
        x, src = self._read(wav, is_i16, ln)
        self.log.append(dict(name="ev_watermark", B=B, flags=int(flags), cfg=_cfg(cfg), lens=ln.tolist(), is_i16=int(is_i16), src=src,
                             payloads=_host(payloads, C.c_uint32, B).tolist(), nbits=_host(nbits, C.c_int32, B).tolist(),
                             strengths_db=_host(strengths_db, C.c_float, B).tolist()))
        out, lo = marked(x, ln), (ln // 256 * 256).astype(np.int64)
        res = ref._obj
        res.batch, res.total = B, int(lo.sum())
        return self._fill("watermark", ref, wav=out, wav_i16=fk.to_i16(out) if cfg is not None and cfg._obj.want_i16 else None, lens_out=lo,
                          offsets=np.concatenate([[0], np.cumsum(lo)]).astype(np.int64))
