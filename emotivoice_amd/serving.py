"""Serving shell on top of the FFI: dynamic batching + an OpenAI-compatible ``/v1/audio/speech`` endpoint.

Reference: openaiapi.py:111-184 -- one synchronous generator call per HTTP request (B = 1), speed changed afterwards by
pyrubberband time-stretching (:170-171).  Here:
  * requests from concurrent clients are collected by ``DynamicBatcher`` for at most ``max_wait_ms`` (or until ``max_batch`` /
    ``max_tokens``) and synthesised in ONE ev_synthesize call -- the engine evaluates every utterance with B = 1 semantics, so
    batching changes latency and throughput, never the audio (tests/test_gpu_parity.py::test_batch_invariance_bit_exact);
  * ``speed`` maps to the model's own duration scale alpha = 1 / speed (GaussianUpsampling's alpha, modules/alignment.py:183)
    instead of a time-stretch of the finished waveform; requests with different speeds form separate batches -- unless the
    batcher is built with ``mixed_prosody=True``: then every request's speed / pitch / energy controls travel with it into one
    ev_synthesize_prosody call (``engine_prosody_synth_fn``), whatever the mix;
  * the text front-end (G2P) and the tokenizer are host-side callables supplied by the caller (the reference's frontend.py /
    AutoTokenizer), the style encoder is the device SimBERT (emotivoice_amd/simbert.py) or any ``text -> 768-vector`` callable.
Response formats: ``wav`` (16-bit PCM in a RIFF container) and ``pcm`` (raw little-endian int16); mp3 needs pydub / ffmpeg,
which are not part of this package.  A service built with ``delivery=`` (an emotivoice_amd.delivery.DeliveryConfig: the client's sample rate
and encoding, converted on the device by ev_deliver) answers at that rate: its utterances travel as ``bytes``, ``pcm`` / ``ulaw`` / ``alaw``
pass them through and ``wav`` wraps them in a RIFF container of the delivered encoding.
"""
from __future__ import annotations

import dataclasses
import io
import logging
import queue
import threading
import time
import wave
from concurrent.futures import Future
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from .prosody import Prosody
from .text_io import wav_float_to_int16


_log = logging.getLogger("emotivoice_amd.serving")


@dataclass
class SynthesisRequest:
    ling: np.ndarray                 # (N,) int64 phoneme ids
    speaker: int
    style: object                    # (768,) array, or the prompt TEXT when the batcher owns the embedder (embed_batch_fn)
    content: object                  # (768,) array, or the content text
    alpha: float = 1.0               # duration scale (1 / speed)
    future: Future = field(default_factory=Future)
    prosody: Optional[Prosody] = None     # per-utterance controls (mixed_prosody batchers only); its speed / alpha, if set, wins over ``alpha``
    t_submit: float = field(default_factory=time.perf_counter)
    response_format: Optional[str] = None     # "flac": the Future resolves to the stream's bytes (flac_synth_fn batchers only); else to the waveform


class DynamicBatcher:
    """Collects requests into batches for ``synth_fn(utts, alpha) -> list of float waveforms`` (one per utterance, in order).
    One worker thread owns the engine handle (the handle is not thread-safe, include/evhip.h): everything that touches the
    handle runs on that thread -- including the style / content embedding when the embedder lives on the same handle
    (``embed_batch_fn(texts) -> (len(texts), 768)``: requests then carry the TEXTS and the worker embeds a whole batch at once,
    which also batches the BERT forward).
    ``mixed_prosody=True``: requests are no longer grouped by ``alpha``; ``synth_fn(utts, prosodies)`` then receives one Prosody per
    utterance (speed folded in as its alpha) -- ``engine_prosody_synth_fn``.
    ``flac_synth_fn(utts, alpha_or_prosodies, mask) -> list`` (``engine_flac_synth_fn``): called instead of ``synth_fn`` for a batch in which
    some request was submitted with ``response_format="flac"``; it returns, per utterance, the FLAC stream (``bytes``) where ``mask`` is True
    and the float waveform elsewhere.  The encoding thus runs on the worker thread, on the same handle.  Batches without such a request call
    ``synth_fn`` exactly as before.
    ``delivery``: the DeliveryConfig the synth functions were built with (``engine_synth_fn(engine, delivery=...)``): they then return the
    delivered ``bytes`` of every utterance, which resolve the Futures as they are; ``response_format`` "ulaw" / "alaw" needs it."""

    def __init__(self, synth_fn: Callable[[List[dict], float], Sequence[np.ndarray]], max_batch: int = 32, max_wait_ms: float = 5.0,
                 max_tokens: int = 16384, embed_batch_fn: Optional[Callable[[List[str]], np.ndarray]] = None,
                 n_vocab: Optional[int] = None, n_speaker: Optional[int] = None, max_len: int = 4096, mixed_prosody: bool = False,
                 flac_synth_fn: Optional[Callable[[List[dict], object, List[bool]], Sequence[object]]] = None, delivery=None):
        from .delivery import delivery_config
        self.delivery = delivery_config(delivery)
        self.mixed_prosody = mixed_prosody
        self.flac_synth_fn = flac_synth_fn
        self.synth_fn, self.max_batch, self.max_wait, self.max_tokens = synth_fn, max_batch, max_wait_ms * 1e-3, max_tokens
        self.embed_batch_fn, self.n_vocab, self.n_speaker, self.max_len = embed_batch_fn, n_vocab, n_speaker, max_len
        self._q: "queue.Queue[Optional[SynthesisRequest]]" = queue.Queue()
        self._carry: List[SynthesisRequest] = []
        self.batches: List[int] = []          # sizes of the batches formed so far (observability / tests)
        self.retried: int = 0                 # batches that failed as a whole and were re-run one request at a time
        self.loop_errors: int = 0             # exceptions the worker loop itself swallowed to stay alive (should stay 0)
        self._stop = False
        self._lock = threading.Lock()         # orders submit's (closed? -> enqueue) against close's (closed := True -> sentinel)
        self._thread = threading.Thread(target=self._loop, name="ev-batcher", daemon=True)
        self._thread.start()

    def submit(self, ling, speaker: int, style, content, alpha: float = 1.0, prosody: Optional[Prosody] = None,
               response_format: Optional[str] = None) -> Future:
        """Validation happens HERE (ValueError -> the handler's 400), so that one malformed request cannot take the requests
        batched with it down: the reference serves every request on its own (openaiapi.py:159-184)."""
        ling = np.asarray(ling, np.int64).reshape(-1)
        if ling.size == 0:
            raise ValueError("empty phoneme sequence")
        if ling.size > self.max_len:
            raise ValueError("phoneme sequence too long (%d > %d)" % (ling.size, self.max_len))
        if ling.min() < 0 or (self.n_vocab is not None and ling.max() >= self.n_vocab):
            raise ValueError("phoneme id out of range")
        if int(speaker) < 0 or (self.n_speaker is not None and int(speaker) >= self.n_speaker):
            raise ValueError("speaker id out of range")
        if not (alpha > 0 and np.isfinite(alpha)):
            raise ValueError("alpha must be positive")
        if response_format == "flac" and self.flac_synth_fn is None:
            raise ValueError("response_format 'flac' needs a batcher with flac_synth_fn (engine_flac_synth_fn): FLAC is encoded on the device")
        if response_format in ("ulaw", "alaw") and (self.delivery is None or self.delivery.encoding != response_format):
            raise ValueError("response_format %r needs a batcher with delivery= of that encoding (emotivoice_amd.delivery.DeliveryConfig): "
                             "G.711 is encoded on the device" % response_format)
        if prosody is not None:
            if not self.mixed_prosody:
                raise ValueError("prosody controls need a batcher with mixed_prosody=True")
            from .prosody import pack_prosody
            pack_prosody([prosody], [ling.size], alpha)        # validation only: a bad control fails its own request, not the batch

        def emb(x):
            if isinstance(x, str):
                if self.embed_batch_fn is None:
                    raise ValueError("text embeddings need a batcher with embed_batch_fn")
                return x
            x = np.asarray(x, np.float32).reshape(-1)
            if not np.isfinite(x).all():
                raise ValueError("embedding is not finite")
            return x
        req = SynthesisRequest(ling, int(speaker), emb(style), emb(content), float(alpha), prosody=prosody, response_format=response_format)
        with self._lock:
            if self._stop:
                raise RuntimeError("batcher is closed")
            self._q.put(req)
        return req.future

    def close(self, timeout: float = 30.0) -> bool:
        """Stop accepting requests, let the worker drain what it has, and fail whatever is left.  Returns True when the worker has exited.
        False = the join timed out: the worker is still inside ``synth_fn`` (a hung device call, say).  Its queued and carried requests then stay
        with it -- it fails or serves them if it ever returns; a client must not wait on such a Future without its own timeout (``TTSService.speech``
        passes one), and the owner of the batcher decides what a wedged engine means for the process (the reference's server has no such state:
        one synchronous call per request, openaiapi.py:159-184).  ``close`` can be called again later to collect the worker."""
        with self._lock:
            if not self._stop:
                self._stop = True
                self._q.put(None)
        self._thread.join(timeout=timeout)
        if self._thread.is_alive():
            # the worker is still inside a batch (join timed out): it owns the queue and _carry; the sentinel stays queued, so it exits after
            # draining what it has, and nothing is taken from under it here
            _log.error("DynamicBatcher.close: the worker did not finish within %.1f s; %d request(s) stay queued behind it", timeout, self._q.qsize())
            return False
        # the worker has exited (or died): whatever is still queued or carried must not leave its client waiting
        left = list(self._carry)
        self._carry = []
        while True:
            try:
                r = self._q.get_nowait()
            except queue.Empty:
                break
            if r is not None:
                left.append(r)
        for r in left:
            _resolve(r.future, exception=RuntimeError("batcher closed"))
        return True

    def _take_batch(self) -> List[SynthesisRequest]:
        """Block for the first request, then keep collecting until the batch is full, the token budget is reached or
        ``max_wait`` has passed since the first request arrived.  Requests with another alpha are carried to the next batch."""
        first = self._carry.pop(0) if self._carry else self._q.get()
        if first is None:
            return []
        batch = [first]
        cur = first                                         # the request whose fields are being looked at (the one to blame if that raises)
        try:
            tokens = len(first.ling)
            deadline = time.perf_counter() + self.max_wait
            keep = []
            for r in self._carry:                           # carried requests first (they have waited longest)
                cur = r
                if (self.mixed_prosody or r.alpha == first.alpha) and len(batch) < self.max_batch and tokens + len(r.ling) <= self.max_tokens:
                    batch.append(r); tokens += len(r.ling)
                else:
                    keep.append(r)
            self._carry = keep
            while len(batch) < self.max_batch and tokens < self.max_tokens:
                timeout = deadline - time.perf_counter()
                if timeout <= 0:
                    break
                try:
                    r = self._q.get(timeout=timeout)
                except queue.Empty:
                    break
                if r is None:
                    self._q.put(None)
                    break
                batch.append(r)                             # (taken off the queue: from here on it is somebody's responsibility)
                cur = r
                if (self.mixed_prosody or r.alpha == first.alpha) and tokens + len(r.ling) <= self.max_tokens:
                    tokens += len(r.ling)
                else:
                    batch.pop()
                    self._carry.append(r)
            return batch
        except Exception:
            # a malformed request (e.g. no usable ``ling``) blew up the collection: what was already taken off the queue / the carry list goes
            # back to the carry list, minus the offender, which fails alone -- nobody is left waiting
            rest = [r for r in batch if r is not cur]
            self._carry = rest + [r for r in self._carry if r is not cur and all(r is not x for x in rest)]
            _resolve(cur.future, exception=RuntimeError("request could not be batched (malformed fields)"))
            raise

    def _run(self, batch: List[SynthesisRequest]):
        if self.embed_batch_fn is not None:
            texts = sorted({x for r in batch for x in (r.style, r.content) if isinstance(x, str)})
            if texts:
                vec = np.asarray(self.embed_batch_fn(texts), np.float32)
                if vec.shape[0] != len(texts):
                    raise RuntimeError("embed_batch_fn returned %d vectors for %d texts" % (vec.shape[0], len(texts)))
                table = {t: vec[i] for i, t in enumerate(texts)}
                for r in batch:
                    r.style = table[r.style] if isinstance(r.style, str) else r.style
                    r.content = table[r.content] if isinstance(r.content, str) else r.content
        utts = [dict(ling=r.ling, speaker=r.speaker, style=r.style, content=r.content) for r in batch]
        control = [_request_prosody(r) for r in batch] if self.mixed_prosody else batch[0].alpha
        mask = [r.response_format == "flac" for r in batch]
        if any(mask):
            if self.flac_synth_fn is None:
                raise RuntimeError("a flac request reached a batcher without flac_synth_fn")
            wavs = self.flac_synth_fn(utts, control, mask)
        else:
            wavs = self.synth_fn(utts, control)
        if len(wavs) != len(batch):
            raise RuntimeError("synth_fn returned %d waveforms for %d requests" % (len(wavs), len(batch)))
        for r, w, m in zip(batch, wavs, mask):
            if m:
                if not isinstance(w, (bytes, bytearray)):
                    raise RuntimeError("flac_synth_fn returned %s where a FLAC stream was asked for" % type(w).__name__)
                _resolve(r.future, result=bytes(w))
            elif self.delivery is not None:
                if not isinstance(w, (bytes, bytearray)):
                    raise RuntimeError("synth_fn returned %s where delivered bytes were expected" % type(w).__name__)
                _resolve(r.future, result=bytes(w))
            else:
                _resolve(r.future, result=np.array(w, np.float32, copy=True))

    @staticmethod
    def _claim(r: "SynthesisRequest") -> bool:
        """True if the request's Future could be moved to RUNNING.  A Future its client has cancelled, or already resolved behind the
        batcher's back (set_exception / set_result as the client's own timeout handling -- set_running_or_notify_cancel raises on a
        FINISHED Future), drops ONLY itself: the requests co-batched with it must still be served."""
        try:
            return (not r.future.done()) and r.future.set_running_or_notify_cancel()
        except Exception:
            return False

    def _loop(self):
        consecutive = 0
        while True:
            batch: List[SynthesisRequest] = []
            try:
                batch = self._take_batch()
                if not batch:
                    if self._stop and not self._carry:
                        return
                    continue
                # a client may cancel or resolve its Future while it waits: such requests are dropped here one by one, and a Future that is
                # cancelled later (mid-batch) is simply not resolved (_resolve) -- neither may take the worker thread or its batch-mates down
                batch = [r for r in batch if self._claim(r)]
                if not batch:
                    continue
                self.batches.append(len(batch))
                try:
                    self._run(batch)
                except Exception as e:
                    if len(batch) == 1:
                        _resolve(batch[0].future, exception=e)
                        continue
                    # a batch failed as a whole: re-run its requests one at a time so that only the offender fails
                    self.retried += 1
                    for r in batch:
                        if r.future.done():
                            continue
                        try:
                            self._run([r])
                        except Exception as e1:
                            _resolve(r.future, exception=e1)
                consecutive = 0
            except Exception as e:     # nothing a single request does may end the thread every later request depends on
                self.loop_errors += 1
                consecutive += 1
                _log.exception("DynamicBatcher worker: unexpected error (%d in a row)", consecutive)
                for r in batch:        # ... and nobody may be left waiting on a batch that was dropped half-way
                    _resolve(r.future, exception=e)
                time.sleep(min(0.5, 0.01 * consecutive))      # a persistent failure (e.g. in _take_batch) must not spin a core


def _request_prosody(r: SynthesisRequest) -> Prosody:
    """The controls a request travels with: its Prosody, with the request's alpha where the Prosody sets no speed of its own."""
    p = r.prosody if r.prosody is not None else Prosody()
    if p.speed is None and p.alpha is None:
        p = dataclasses.replace(p, alpha=r.alpha)
    return p


def _resolve(future: Future, result=None, exception: Optional[BaseException] = None):
    """set_result / set_exception that tolerates a Future its client has cancelled or that was resolved already."""
    try:
        if future.done():
            return
        if exception is not None:
            future.set_exception(exception)
        else:
            future.set_result(result)
    except Exception:            # concurrent.futures.InvalidStateError (cancelled between the check and the set)
        pass


def _chain_settings(loudness, limiter, delivery, denoise, flac=None, watermark=None):
    """The shared part of the engine_*_synth_fn factories.  ``loudness``, ``limiter``, ``delivery``, ``denoise`` and ``watermark`` are what EVEngine.synthesize takes
    (emotivoice_amd/output_chain.py): service-level settings, not request fields, so that a batch stays homogeneous and the request schema stays
    the reference's (``delivery`` is to be given to the DynamicBatcher as well).  delivery, denoise, watermark and ``flac`` (a FlacConfig or True: the
    service encodes FLAC) are checked here, when the service is built.  -> (the keywords for synthesize: the settings that are not None -- all
    None: synthesize is called exactly as before; the key of its result that holds the audio; what turns an utterance of it into what the
    batcher resolves a Future with)."""
    from .output_chain import resolve
    plan = resolve(16000, None, denoise=denoise, delivery=delivery, flac=flac, watermark=watermark)
    kw = {k: v for k, v in (("loudness", loudness), ("limiter", limiter), ("denoise", plan.denoise), ("delivery", plan.delivery),
                            ("watermark", plan.watermark)) if v is not None}
    return (kw, "wav_list", lambda w: w) if plan.delivery is None else (kw, "delivered_list", lambda w: w.tobytes())


def engine_synth_fn(engine, loudness=None, limiter=None, delivery=None, denoise=None, watermark=None) -> Callable[[List[dict], float], Sequence[np.ndarray]]:
    """``synth_fn`` of a DynamicBatcher for an EVEngine.  ``loudness``: every utterance normalised on the device (ev_loudness); ``limiter``: its
    true peak held at a ceiling (ev_limit); ``delivery``: every utterance converted to the client's rate and encoding on the device (ev_deliver)
    and returned as ``bytes``; ``denoise``: the vocoder's stationary bias removed from every utterance on the device (ev_denoise), first in the chain;
    ``watermark``: every utterance marked on the device with the service's key (ev_watermark, before ev_loudness; a key, 'KEY[:PAYLOAD:NBITS]' or
    an emotivoice_amd.watermark.WatermarkConfig with one payload, length and strength for every utterance)."""
    kw, key, conv = _chain_settings(loudness, limiter, delivery, denoise, watermark=watermark)
    return lambda utts, alpha: [conv(w) for w in engine.synthesize(utts, alpha=alpha, **kw)[key]]


def engine_prosody_synth_fn(engine, loudness=None, limiter=None, delivery=None, denoise=None, watermark=None) -> Callable[[List[dict], List[Prosody]], Sequence[np.ndarray]]:
    """``synth_fn`` of a ``mixed_prosody=True`` DynamicBatcher for an EVEngine: one ev_synthesize_prosody call per batch.  ``loudness``,
    ``limiter``, ``delivery``, ``denoise`` and ``watermark``: as ``engine_synth_fn``."""
    kw, key, conv = _chain_settings(loudness, limiter, delivery, denoise, watermark=watermark)
    return lambda utts, prosodies: [conv(w) for w in engine.synthesize(utts, prosody=prosodies, **kw)[key]]


def engine_flac_synth_fn(engine, loudness=None, limiter=None, flac_config=None, delivery=None, denoise=None, watermark=None) -> Callable[[List[dict], object, List[bool]], Sequence[object]]:
    """``flac_synth_fn`` of a DynamicBatcher for an EVEngine: one synthesize call per batch; the utterances ``mask`` selects are encoded on the
    device (ev_flac, from the fp32 waveform with the wrapping conversion) and come back as ``bytes``, the others as float waveforms.  The
    second argument is the batch's alpha, or with ``mixed_prosody=True`` its list of Prosody.  ``loudness``: as ``engine_synth_fn``; the
    streams then carry the normalised int16 (the clamping conversion).  ``limiter``: as ``engine_synth_fn``; the streams carry the limiter's int16.
    ``flac_config``: an emotivoice_amd.flac.FlacConfig for every stream of this service (LPC order, precision, MD5, block size), like ``loudness``
    a service-level setting; a batch is then encoded whole and the utterances outside ``mask`` still come back as waveforms.
    ``delivery``: as ``engine_synth_fn``, with the encoding "s16": the streams carry ev_deliver's int16 at the delivered rate, the other
    utterances come back as its ``bytes``.  ``denoise``: as ``engine_synth_fn``; the streams carry the denoised audio.  ``watermark``: as ``engine_synth_fn``;
    the streams carry the marked audio."""
    if flac_config is not None:
        flac_config.validate()
    lkw, key, conv = _chain_settings(loudness, limiter, delivery, denoise, flac=flac_config or True, watermark=watermark)

    def fn(utts, control, mask):
        kw = dict(prosody=control) if isinstance(control, (list, tuple)) else dict(alpha=control)
        out = engine.synthesize(utts, flac=list(mask) if flac_config is None else flac_config, **kw, **lkw)
        return [f if m else conv(w) for f, w, m in zip(out["flac_list"], out[key], mask)]
    return fn


def engine_embed_batch_fn(engine, tokenize: Callable[[str], Sequence[int]]) -> Callable[[List[str]], np.ndarray]:
    """``embed_batch_fn`` of a DynamicBatcher for the device SimBERT living on ``engine`` (ev_style_embed on the SAME handle as
    ev_synthesize -- which is why it has to run on the batcher's thread): ``tokenize(text) -> [CLS] ... [SEP]`` ids
    (emotivoice_amd.wordpiece or the reference's AutoTokenizer, simbert.py / inference_am_vocoder_joint.py:25-38)."""
    return lambda texts: engine.style_embed([np.asarray(tokenize(t), np.int64) for t in texts])


def encode_audio(wav_f32, response_format: str, sample_rate: int, delivery=None) -> bytes:
    """``flac``: the stream was encoded on the device (a batcher with ``flac_synth_fn``) and arrives as ``bytes``, which pass through.
    ``delivery``: the DeliveryConfig of a service whose utterances were converted on the device (ev_deliver) and arrive as ``bytes``: ``pcm``
    (encoding "s16"), ``ulaw`` and ``alaw`` pass them through when the encoding is theirs, ``wav`` wraps them with
    emotivoice_amd.delivery.wav_container at the delivered rate."""
    if response_format == "flac":
        if isinstance(wav_f32, (bytes, bytearray)):
            return bytes(wav_f32)
        raise ValueError("response_format 'flac' is encoded on the device: it needs a batcher with flac_synth_fn (engine_flac_synth_fn)")
    if response_format in ("ulaw", "alaw") and delivery is None:
        raise ValueError("response_format %r needs a service with delivery= of that encoding: G.711 is encoded on the device" % response_format)
    if delivery is not None and isinstance(wav_f32, (bytes, bytearray)):
        from .delivery import wav_container
        if response_format == "wav":
            return wav_container(bytes(wav_f32), delivery.sample_rate, delivery.encoding)
        if response_format in ("pcm", "ulaw", "alaw"):
            if delivery.encoding != {"pcm": "s16"}.get(response_format, response_format):
                raise ValueError("response_format %r: this service delivers %r" % (response_format, delivery.encoding))
            return bytes(wav_f32)
        raise ValueError("response_format %r is not available (wav, pcm, ulaw, alaw, flac); mp3 needs pydub / ffmpeg" % response_format)
    if isinstance(wav_f32, (bytes, bytearray)):
        raise ValueError("an encoded stream cannot be re-encoded as %r" % response_format)
    pcm = wav_float_to_int16(wav_f32)              # the reference's int16 epilogue (openaiapi.py:147-148)
    if response_format == "pcm":
        return pcm.tobytes()
    if response_format == "wav":
        buf = io.BytesIO()
        with wave.open(buf, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(sample_rate)
            w.writeframes(pcm.tobytes())
        return buf.getvalue()
    raise ValueError("response_format %r is not available (wav, pcm, flac); mp3 needs pydub / ffmpeg" % response_format)


class TTSService:
    """text -> audio: G2P, token / speaker lookup, style + content embedding, batched synthesis.  All host-side pieces are
    injected: ``g2p(text) -> phoneme string`` (the reference's frontend.g2p_cn_en), ``embed(text) -> (768,)`` (the device SimBERT
    through a tokenizer, or a placeholder)."""

    def __init__(self, batcher: DynamicBatcher, token2id: Dict[str, int], speaker2id: Dict[str, int], g2p: Callable[[str], str],
                 embed: Optional[Callable[[str], np.ndarray]] = None, sample_rate: int = 16000):
        """``embed`` runs on the CALLER's thread (FastAPI's handler pool): it must be thread-safe and must not share an engine
        handle with the batcher.  For the device SimBERT on the generator's own handle leave it None and give the BATCHER an
        ``embed_batch_fn``: the texts then travel with the request and are embedded on the worker thread, a batch at a time."""
        self.batcher, self.token2id, self.speaker2id, self.g2p, self.embed, self.sample_rate = batcher, token2id, speaker2id, g2p, embed, sample_rate
        self.delivery = getattr(batcher, "delivery", None)      # a delivery-configured batcher: the service answers at its rate
        if self.delivery is not None:
            self.sample_rate = int(self.delivery.sample_rate)
        if embed is None and batcher.embed_batch_fn is None:
            raise ValueError("TTSService needs embed= or a batcher with embed_batch_fn=")

    def submit(self, text: str, voice: str, prompt: str = "", speed: float = 1.0, pitch_shift: float = 0.0, pitch_scale: float = 1.0,
               energy_scale: float = 1.0, response_format: Optional[str] = None) -> Future:
        """``response_format="flac"`` travels with the request (a batcher with ``flac_synth_fn``); every other value is encoded by ``speech``.
        ``pitch_shift`` / ``pitch_scale`` / ``energy_scale`` (extension fields, in the predictor's normalised units; include/evhip.h
        ev_prosody): anything but the identity needs a batcher with ``mixed_prosody=True``."""
        if not (0.25 <= speed <= 4.0):
            raise ValueError("speed must be within [0.25, 4]")
        prosody = None
        if (pitch_shift, pitch_scale, energy_scale) != (0.0, 1.0, 1.0):
            prosody = Prosody(pitch_shift=float(pitch_shift), pitch_scale=float(pitch_scale), energy_scale=float(energy_scale))
        ling = np.array([self.token2id[ph] for ph in self.g2p(text).split()], np.int64)       # KeyError like openaiapi.py:128
        if ling.size == 0:
            raise ValueError("input has no phonemes")
        extra = dict(response_format=response_format) if response_format in ("flac", "ulaw", "alaw") else {}
        if self.embed is None:
            return self.batcher.submit(ling, self.speaker2id[voice], prompt, text, alpha=1.0 / speed, prosody=prosody, **extra)
        return self.batcher.submit(ling, self.speaker2id[voice], self.embed(prompt), self.embed(text), alpha=1.0 / speed, prosody=prosody, **extra)

    def speech(self, text: str, voice: str, prompt: str = "", speed: float = 1.0, response_format: str = "wav", timeout: float = 120.0,
               pitch_shift: float = 0.0, pitch_scale: float = 1.0, energy_scale: float = 1.0) -> bytes:
        fut = self.submit(text, voice, prompt, speed, pitch_shift, pitch_scale, energy_scale, response_format=response_format)
        if self.delivery is None:
            return encode_audio(fut.result(timeout=timeout), response_format, self.sample_rate)
        return encode_audio(fut.result(timeout=timeout), response_format, self.sample_rate, self.delivery)


try:          # the request schema lives at module level: FastAPI resolves the handler's annotations in the module namespace
    from pydantic import BaseModel as _BaseModel

    class SpeechRequest(_BaseModel):
        """openaiapi.py:150-157 (default response_format here is wav: mp3 needs pydub / ffmpeg)."""
        input: str
        voice: str = "8051"
        prompt: Optional[str] = ""
        language: Optional[str] = "zh_us"
        model: Optional[str] = "emoti-voice"
        response_format: Optional[str] = "wav"
        speed: Optional[float] = 1.0
        # extensions (not in the reference schema): prosody controls in the predictor's normalised units, identity by default
        pitch_shift: Optional[float] = 0.0
        pitch_scale: Optional[float] = 1.0
        energy_scale: Optional[float] = 1.0
except ImportError:          # pydantic / fastapi are only needed by create_app
    SpeechRequest = None


def create_app(service: TTSService):
    """FastAPI application with the reference's route and request schema (openaiapi.py:150-184)."""
    from fastapi import FastAPI, HTTPException, Response

    app = FastAPI()

    @app.post("/v1/audio/speech")
    def text_to_speech(req: SpeechRequest):
        try:
            data = service.speech(req.input, req.voice, req.prompt or "", req.speed or 1.0, req.response_format or "wav",
                                  pitch_shift=req.pitch_shift if req.pitch_shift is not None else 0.0,
                                  pitch_scale=req.pitch_scale if req.pitch_scale is not None else 1.0,
                                  energy_scale=req.energy_scale if req.energy_scale is not None else 1.0)
        except KeyError as e:
            raise HTTPException(status_code=400, detail="unknown voice or phoneme: %s" % e)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        return Response(content=data, media_type="audio/%s" % (req.response_format or "wav"))

    return app
