"""A stand-in for the object ``emotivoice_amd._ffi.lib()`` returns, for CPU tests of the Python above the library (tests/test_engine_chain.py,
test_deliver_chain.py, test_denoise.py, test_chain_transcripts.py).

Only the entries of the output chain (emotivoice_amd/output_chain.py).  "Device" memory is host numpy memory kept alive in ``bufs``; every entry
appends what it was given to ``log`` (pointer arguments as (buffer, byte offset)) and fills the real _ffi result struct.  The arithmetic is
trivial and tells the stages apart: the synthesis writes ``ramp``, ev_stitch negates, ev_loudness with a target doubles, ev_limit multiplies by
gain * 3, every int16 is ``to_i16`` of its fp32, and a FLAC stream is b"fLaC" + the first 8 bytes of its segment.  One frame per token.

FakeLib has the synthesis, ev_stitch, ev_loudness, ev_limit and ev_flac, and raises (AttributeError) on any deliver or denoise call: two tests
hold the chain without those stages to exactly the calls it made before they existed.  DeliverLib adds ev_deliver, which NEGATES and keeps
every second sample; DenoiseLib adds ev_denoise, which ADDS 1/8 and cuts every utterance to whole hops, its setup and bias, and an ev_compare
with fixed sums.  A test that needs both stages subclasses both."""
import ctypes as C
import math

import numpy as np

from emotivoice_amd import _ffi

UP = 256                                     # EVShapes().upsample_factor
LOUDNESS = lambda b: -20.0 - b               # noqa: E731  what ev_loudness reports for segment b


def ramp(n):
    return ((np.arange(n) % 97 + 1) / 4096.0).astype(np.float32)


def to_i16(x):
    return np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def _addr(p):
    return p.value if isinstance(p, C.c_void_p) else p


def _host(p, ctype, n):
    """A copy of the n elements of a host array argument (a c_void_p)."""
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), (n,)).copy() if n else np.zeros(0, ctype)


def _cfg(ref):
    return None if ref is None else {k: getattr(ref._obj, k) for k, _ in ref._obj._fields_ if k != "struct_size"}


class FakeLib:
    def __init__(self):
        self.log, self.bufs = [], {}

    def names(self, skip=("ev_memcpy_d2h",)):
        return [e["name"] for e in self.log if e["name"] not in skip]

    def calls(self, name):
        return [e for e in self.log if e["name"] == name]

    def where(self, p):
        """(buffer, byte offset) of an address inside one of ``bufs``, ("host", None) for any other."""
        a = _addr(p)
        for name, buf in self.bufs.items():
            if a is not None and buf.nbytes and buf.ctypes.data <= a < buf.ctypes.data + buf.nbytes:
                return name, a - buf.ctypes.data
        return "host", None

    def _fill(self, tag, ref, **arrays):
        """Keep the arrays as ``bufs[tag.field]`` and point the result struct's fields at them (None: the field stays null)."""
        res = ref._obj
        types = dict(res._fields_)
        for k, a in arrays.items():
            if a is not None:
                a = self.bufs[tag + "." + k] = np.ascontiguousarray(a)
                setattr(res, k, a.ctypes.data if types[k] is C.c_void_p else a.ctypes.data_as(types[k]))
        return 0

    def _read(self, p, is_i16, lens):
        """The packed input of a stage, as (array, (buffer, byte offset))."""
        n = int(np.sum(lens))
        return _host(p, C.c_int16 if is_i16 else C.c_float, n), self.where(p)

    # -- handle
    def ev_default_config(self, ref):
        pass

    def ev_create(self, device_id, cfg, h):
        h._obj.value = 1
        return 0

    def ev_destroy(self, h):
        pass

    def ev_last_error(self, h):
        return b"fake_evhip has no errors"

    def ev_memcpy_d2h(self, h, dst, src, n):
        self.log.append(dict(name="ev_memcpy_d2h", src=self.where(src), nbytes=int(n)))
        C.memmove(dst, src, n)
        return 0

    def _stub(self, *args):
        self.log.append(dict(name="stub"))
        return 0

    ev_features = ev_pitch = ev_resample = _stub

    # -- synthesis
    def _synthesize(self, name, B, cu, flags, ref):
        frames = np.diff(_host(cu, C.c_int32, B + 1)).astype(np.int32)
        self.log.append(dict(name=name, B=B, flags=int(flags), tokens=frames.tolist()))
        res = ref._obj
        res.batch, res.total_tokens, res.total_frames, res.total_samples = B, int(frames.sum()), int(frames.sum()), int(frames.sum()) * UP
        wav = None if flags & _ffi.EV_FLAG_NO_VOCODER else ramp(res.total_samples)
        i16 = to_i16(wav) if wav is not None and flags & _ffi.EV_FLAG_WANT_INT16 else None
        return self._fill("synth", ref, wav=wav, wav_i16=i16, mel_lens=frames, mel_offsets=np.concatenate([[0], np.cumsum(frames)]).astype(np.int64))

    def ev_synthesize(self, h, B, ling, cu, spk, style, content, alpha, flags, ref):
        return self._synthesize("ev_synthesize", B, cu, flags, ref)

    def ev_synthesize_prosody(self, h, B, ling, cu, spk, style, content, alpha, prosody, flags, ref):
        return self._synthesize("ev_synthesize_prosody", B, cu, flags, ref)

    # -- the output stages
    def ev_stitch(self, h, S, wav, seg_offsets, seg_lens, seg_doc, pause_after, cfg, flags, ref):
        so, sl, sd = _host(seg_offsets, C.c_int64, S), _host(seg_lens, C.c_int64, S), _host(seg_doc, C.c_int32, S)
        self.log.append(dict(name="ev_stitch", B=S, flags=int(flags), cfg=_cfg(cfg), lens=sl.tolist(), offsets=so.tolist(), seg_doc=sd.tolist(),
                             src=self.where(wav)))
        x = _host(wav, C.c_float, int((so + sl).max()))
        D = int(sd.max()) + 1
        doc_lens = np.array([sl[sd == d].sum() for d in range(D)], np.int64)
        docs = -np.concatenate([x[o:o + n] for o, n in zip(so, sl)])
        pos = np.concatenate([np.cumsum(sl[sd == d]) - sl[sd == d] for d in range(D)]).astype(np.int64)
        res = ref._obj
        res.batch_docs, res.batch_segs, res.total_samples = D, S, int(sl.sum())
        return self._fill("stitch", ref, wav=docs, wav_i16=to_i16(docs) if cfg is not None and cfg._obj.want_i16 else None, doc_lens=doc_lens,
                          doc_offsets=np.concatenate([[0], np.cumsum(doc_lens)]).astype(np.int64), seg_pos=pos, seg_start=np.zeros(S, np.int64),
                          seg_end=sl, seg_peak=np.array([np.abs(x[o:o + n]).max() for o, n in zip(so, sl)], np.float32))

    def ev_loudness(self, h, B, wav, is_i16, lens, cfg, flags, ref):
        ln = _host(lens, C.c_int64, B)
        x, src = self._read(wav, is_i16, ln)
        self.log.append(dict(name="ev_loudness", B=B, flags=int(flags), cfg=_cfg(cfg), lens=ln.tolist(), is_i16=int(is_i16), src=src))
        c = cfg._obj
        measure = math.isnan(c.target_lufs)
        out = None if measure else x * np.float32(2.0)
        res = ref._obj
        res.batch, res.total = B, int(ln.sum())
        return self._fill("loudness", ref, wav=out, wav_i16=to_i16(out) if out is not None and c.want_i16 else None,
                          loudness=np.array([LOUDNESS(b) for b in range(B)], np.float64), rel_threshold=np.full(B, -30.0), gain=np.full(B, 1.0 if measure else 2.0, np.float32),
                          peak=np.full(B, 0.5, np.float32), flags=np.zeros(B, np.uint8), nonfinite=np.zeros(B, np.int64),
                          block_offsets=np.arange(B + 1, dtype=np.int64), block_ms=np.full(B, 0.25), block_state=np.full(B, 2, np.uint8))

    def ev_limit(self, h, B, wav, is_i16, lens, gains, cfg, flags, ref):
        ln = _host(lens, C.c_int64, B)
        x, src = self._read(wav, is_i16, ln)
        g = np.ones(B, np.float32) if gains is None else _host(gains, C.c_float, B)
        self.log.append(dict(name="ev_limit", B=B, flags=int(flags), cfg=_cfg(cfg), lens=ln.tolist(), is_i16=int(is_i16), src=src,
                             gains=None if gains is None else g.tolist()))
        out = x * np.repeat(g * np.float32(3.0), ln)
        res = ref._obj
        res.batch, res.total = B, int(ln.sum())
        peaks = {k: np.full(B, v, np.float32) for k, v in (("true_peak_in", 0.9), ("sample_peak_in", 0.8), ("true_peak_out", 0.7), ("sample_peak_out", 0.6), ("min_gain", 0.5))}
        return self._fill("limit", ref, wav=out, wav_i16=to_i16(out) if cfg._obj.want_i16 else None, limited=np.arange(B, dtype=np.int64),
                          nonfinite=np.zeros(B, np.int64), **peaks)

    def ev_flac(self, h, B, pcm, is_i16, lens, cfg, flags, ref):
        ln = _host(lens, C.c_int64, B)
        x, src = self._read(pcm, is_i16, ln)
        self.log.append(dict(name="ev_flac", B=B, flags=int(flags), cfg=_cfg(cfg), lens=ln.tolist(), is_i16=int(is_i16), src=src))
        offs = np.concatenate([[0], np.cumsum(ln)])
        streams = [b"fLaC" + x[offs[b]:offs[b + 1]].tobytes()[:8] for b in range(B)]
        res = ref._obj
        res.batch, res.total_bytes, res.total_frames = B, sum(len(s) for s in streams), B
        return self._fill("flac%d" % len(self.calls("ev_flac")), ref, bytes=np.frombuffer(b"".join(streams), np.uint8),
                          stream_offsets=np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64), stream_frames=np.ones(B, np.int64),
                          frame_offsets=np.arange(B + 1, dtype=np.int64), frame_kind=np.full(B, 8, np.uint8), frame_porder=np.zeros(B, np.uint8))


# -- the two later stages, each a subclass so that FakeLib itself keeps raising on any deliver or denoise call
def encode(y, encoding):
    """The stand-in's conversion: fp32, the stand-in's int16, or the int16's high byte."""
    return y.astype(np.float32) if encoding == 0 else to_i16(y) if encoding == 1 else (to_i16(y).astype(np.int32) >> 8 & 0xFF).astype(np.uint8)


class DeliverLib(FakeLib):
    setup = None

    def ev_deliver_setup(self, h, ref):
        self.setup = _cfg(ref)
        self.log.append(dict(name="ev_deliver_setup", cfg=dict(self.setup)))
        return 0

    def ev_deliver(self, h, B, wav, is_i16, lens, seeds, flags, ref):
        ln = _host(lens, C.c_int64, B)
        x, src = self._read(wav, is_i16, ln)
        self.log.append(dict(name="ev_deliver", B=B, flags=int(flags), lens=ln.tolist(), is_i16=int(is_i16), src=src, seeds=seeds))
        offs, parts, n, at = [0], [], [], 0
        for L in ln:
            y = encode(-x[at:at + L:2], self.setup["encoding"])
            at += int(L)
            raw = y.tobytes()
            parts.append(raw + b"\0" * (-len(raw) % 16))
            n.append(y.size)
            offs.append(offs[-1] + len(parts[-1]))
        res = ref._obj
        res.batch, res.total_bytes = B, offs[-1]
        return self._fill("deliver", ref, data=np.frombuffer(b"".join(parts), np.uint8), byte_offsets=np.array(offs, np.int64), n_samples=np.array(n, np.int64),
                          peak=np.full(B, 0.25, np.float32), clipped=np.arange(B, dtype=np.int64))


EIGHTH = np.float32(0.125)      # what the stand-in ev_denoise adds


class DenoiseLib(FakeLib):
    setup = None

    def ev_default_denoise_config(self, ref):
        c = ref._obj
        c.struct_size, c.n_fft, c.hop, c.strength = C.sizeof(_ffi.ev_denoise_config), 1024, 256, 0.01

    def ev_denoise_setup(self, h, ref, bias):
        self.setup = _cfg(ref)
        self.log.append(dict(name="ev_denoise_setup", cfg=dict(self.setup), bias=None if bias is None else _host(bias, C.c_float, 513).tolist()))
        if bias is None:      # measuring runs the vocoder: whatever the synthesis left is gone
            self.log.append(dict(name="ev_vocoder(zero mel)"))
            if "synth.wav" in self.bufs:
                self.bufs["synth.wav"][:] = np.nan
        return 0

    def ev_denoise_bias(self, h, out):
        self.log.append(dict(name="ev_denoise_bias"))
        half = np.full(513, 0.5, np.float32)
        C.memmove(out, half.ctypes.data, half.nbytes)
        return 0

    def ev_denoise(self, h, B, wav, is_i16, lens, strengths, flags, ref):
        ln = _host(lens, C.c_int64, B)
        x, src = self._read(wav, is_i16, ln)
        self.log.append(dict(name="ev_denoise", B=B, flags=int(flags), lens=ln.tolist(), is_i16=int(is_i16), src=src, strengths=strengths, cfg=dict(self.setup)))
        offs = np.concatenate([[0], np.cumsum(ln)])
        lo = ln // 256 * 256
        out = np.concatenate([x[a:a + n] + EIGHTH for a, n in zip(offs[:-1], lo)])
        res = ref._obj
        res.batch, res.total = B, int(lo.sum())
        return self._fill("denoise", ref, wav=out, wav_i16=to_i16(out) if self.setup["want_i16"] else None, lens_out=lo.astype(np.int64),
                          offsets=np.concatenate([[0], np.cumsum(lo)]).astype(np.int64))

    def ev_compare(self, h, B, a, b, lens, flags, ref):
        ln = _host(lens, C.c_int64, B)
        self.log.append(dict(name="ev_compare", B=B, flags=int(flags), lens=ln.tolist(), a=self.where(a), b=self.where(b)))
        z, zi = np.zeros(B), np.zeros(B, np.int64)
        res = ref._obj
        res.batch, res.total = B, int(ln.sum())
        return self._fill("compare", ref, sum_d=z, sum_d2=np.full(B, 1.0), sum_y=z, sum_y2=np.full(B, 100.0), rel_l2=z, rel_l2_ac=z, max_abs_d=np.zeros(B, np.float32),
                          argmax_d=zi, peak_y=np.zeros(B, np.float32), nonfinite=zi, chunk_offsets=np.arange(B + 1, dtype=np.int64), chunk_d2=z, chunk_y2=z)
