"""The output chain of EVEngine.synthesize / synthesize_long: denoise -> stretch -> watermark -> loudness -> limiter -> delivery -> FLAC, as one
plan and one runner.

``resolve`` turns the public arguments (``denoise=``, ``stretch=``, ``watermark=``, ``loudness=``, ``limiter=``, ``delivery=``, ``flac=``) into a ChainPlan and
makes every argument check, before any library call (what only the lengths can decide -- a stretch ratio outside [0.5, 2] -- is checked by the
host rule once the source's lengths are known, still before ev_stretch is called).  ``run`` takes the packed fp32 device waveform of the SOURCE -- the synthesis, or ev_stitch in the long
form -- through the stages of the plan and returns a ChainOutput.  The rules, which hold for every combination:

Order.  ev_denoise first (on the source's waveform, so that the later stages measure and shape the audio that is delivered; its output has whole
hops, so it may shorten a segment), then ev_stretch (it changes every length; the stages after it see the new ones), then ev_watermark (a stretch would move its
tiles, so it runs after it; loudness and the limiter then measure and bound what is delivered, and a gain does not change the detector's
signs; its output has whole hops, like ev_denoise's), then ev_loudness, then ev_limit: the WAVEFORM stages, each reading the device fp32 output of the one before.
ev_deliver follows them and ev_flac comes last.  loudness followed by a limiter is a MEASURE-only stage: ev_loudness runs with a NaN target and
writes no audio, the pre-gain to the target is worked out on the host (emotivoice_amd.limiter.pre_gain: the gain rule without its sample-peak
step) and goes into ev_limit, which scales and limits in its one pass; the ``loudness`` figures then hold the measurement and, as ``gain`` /
``flags``, the host's values.  The loudness is not measured again after the limiter.

Who makes the int16.  Only the LAST waveform stage (the source when there is none: ``ChainPlan.staged`` tells it to make none itself), by the
clamping rule, when the caller wants it or FLAC will read it -- and nobody when the response is delivered: ev_deliver reads fp32.

What is copied to the host.  Only the last stage's audio (with ``int16_only`` and a stage that made int16, the int16 alone); of every other
stage only its figures.  A delivered response copies ev_deliver's bytes and nothing of the 16 kHz waveform.

What a FLAC stream decodes to.  No stage: the wrapping conversion of the source's fp32 (wav_float_to_int16(wav_list[b])), or the source's own
int16 when it made one (ev_stitch's documents).  Waveform stages: the last stage's clamped int16 (wav_int16_list[b] / the int16 documents).
Delivered (encoding "s16" only): ev_deliver's int16 at the delivered rate, delivered_list[b].  ev_flac takes its segments back to back, so the
selected segments of a packed waveform go in as runs of neighbours, and those of a delivery result -- each on its own 16-byte boundary -- one
call each.

The figures of every stage sit in ``ChainOutput.figures`` under the stage's argument name; ``denoise`` holds lens_out / offsets and, with
``report=True``, removed_db: the removed energy relative to the input, from ev_compare on the two device waveforms; ``stretch`` holds lens_in,
lens_out, offsets, speed (lens_in / lens_out), frames, edge_frames and sum_dist; ``watermark`` holds lens_out, offsets, key, payload, nbits and
strength_db."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional

import numpy as np

from . import _ffi
from .delivery import DeliveryConfig, delivery_config
from .denoise import DenoiseConfig, denoise_config, removed_db
from .engine_audio import offsets_of
from .flac import FlacConfig
from .limiter import LimiterConfig, as_config as limiter_config, pre_gain
from .loudness import LoudnessConfig, as_config as loudness_config
from .stretch import StretchConfig, stretch_config
from .watermark import WatermarkConfig, watermark_config

AUDIO_KEYS = ("wav", "wav_list", "wav_i16", "wav_i16_list")      # what ``*_to_numpy`` calls the audio of a waveform stage


@dataclasses.dataclass(frozen=True)
class ChainPlan:
    """The validated stage configs of one call (None: the stage is off).  ``flac``: None, True (every segment) or one boolean per segment;
    ``flac_config`` is set with it and carries the rate FLAC reads at, the delivered one under a delivery."""
    sample_rate: int
    denoise: Optional[DenoiseConfig] = None
    loudness: Optional[LoudnessConfig] = None
    limiter: Optional[LimiterConfig] = None
    delivery: Optional[DeliveryConfig] = None
    flac: object = None
    flac_config: Optional[FlacConfig] = None
    stretch: Optional[StretchConfig] = None
    watermark: Optional[WatermarkConfig] = None

    @property
    def staged(self) -> bool:
        """The audio is a stage's: the source makes no int16 itself and its waveform stays on the device."""
        return not (self.denoise is None and self.stretch is None and self.watermark is None and self.loudness is None and self.limiter is None and self.delivery is None)

    def waveform_stages(self) -> list:
        """(stage, config) in the order they run; loudness in front of a limiter is "measure"."""
        stages = (("denoise", self.denoise), ("stretch", self.stretch), ("watermark", self.watermark), ("measure" if self.limiter is not None else "loudness", self.loudness),
                  ("limiter", self.limiter))
        return [(name, cfg) for name, cfg in stages if cfg is not None]


def resolve(sample_rate: int, segments: Optional[int], denoise=None, loudness=None, limiter=None, delivery=None, flac=None, vocoder: bool = True,
            flac_convert: Optional[str] = None, stretch=None, watermark=None) -> ChainPlan:
    """The public stage arguments -> a ChainPlan, or ValueError.  sample_rate: the engine's; segments: how many a per-segment ``flac`` mask must
    have (None: ``flac`` is a switch, any true value selects every segment); flac_convert: overrides the ``convert`` of a given FlacConfig."""
    sr = int(sample_rate)
    if flac is None or flac is False or (segments is None and not flac):
        sel = None
    elif flac is True or isinstance(flac, FlacConfig) or segments is None:
        sel = True
    else:
        sel = np.asarray(flac, bool)
        if sel.shape != (segments,):
            raise ValueError("flac: True or one entry per utterance (%d), got shape %s" % (segments, sel.shape))
    for name, given in (("flac", sel), ("limiter", limiter), ("loudness", loudness), ("delivery", delivery), ("denoise", denoise), ("stretch", stretch),
                        ("watermark", watermark)):
        if given is not None and not vocoder:
            raise ValueError("%s needs the vocoder's waveform" % name)
    lc = None if loudness is None else loudness_config(loudness, sr)
    mc = None if limiter is None else limiter_config(limiter, sr)
    dc = delivery_config(delivery, sr)
    nc = denoise_config(denoise, sr)
    tc = stretch_config(stretch, sr)
    if tc is not None and segments is not None:
        tc.per_segment(segments, sr)      # one entry per segment, at most one of speed / seconds / samples each
    wc = watermark_config(watermark, sr)
    if wc is not None and segments is not None:
        wc.per_segment(segments)      # one payload, length and strength per segment
    if dc is not None and sel is not None and dc.encoding != "s16":
        raise ValueError("flac needs delivery's encoding 's16', not %r" % dc.encoding)
    fc = None
    if sel is not None:
        kw = dict(sample_rate=sr if dc is None else int(dc.sample_rate), **({} if flac_convert is None else dict(convert=flac_convert)))
        fc = dataclasses.replace(flac, **kw).validate() if isinstance(flac, FlacConfig) else FlacConfig(**kw)
    return ChainPlan(sr, nc, lc, mc, dc, sel, fc, tc, wc)


@dataclasses.dataclass
class ChainOutput:
    audio: Dict[str, object]                  # the last stage's, under AUDIO_KEYS; delivered: delivered_list, delivered_rate, delivery
    figures: Dict[str, Dict[str, object]]     # "denoise" / "stretch" / "watermark" / "loudness" / "limiter" -> that stage's host figures
    last: object = None                       # the result struct of the last waveform stage, whose int16 FLAC reads (None: the source's)
    delivered: object = None                  # the ev_deliver_result, which FLAC reads instead
    flac_list: Optional[List[Optional[bytes]]] = None

    def into(self, out: Dict[str, object], names) -> Dict[str, object]:
        """Adds the chain's output to an entry point's result: the audio under that entry point's ``names`` ((key here, key there) pairs), a
        delivered response and the figures under their own."""
        if "denoise" in self.figures:
            out["denoise"] = self.figures["denoise"]
        if self.delivered is not None:
            out.update(self.audio)
        out.update((name, self.audio[k]) for k, name in names if k in self.audio)
        out.update((k, v) for k, v in self.figures.items() if k != "denoise")
        if self.flac_list is not None:
            out["flac_list"] = self.flac_list
        return out


def _removed_db(eng, res, got, wav_ptr: int, lens) -> np.ndarray:
    """denoise's report: ev_compare of its device output against its device input, in one call, or utterance by utterance when a length was cut
    to whole hops and the two packings differ."""
    dev, B = _ffi.EV_FLAG_DEVICE_INPUTS, len(lens)
    if np.array_equal(got["lens_out"], np.asarray(lens, np.int64)):
        cmp = eng.compare_to_numpy(eng.compare_raw(B, res.wav, wav_ptr, lens, dev))
        return removed_db(cmp["sum_d2"], cmp["sum_y2"])
    offs_in, rd = offsets_of(lens), []
    for b in range(B):
        cmp = eng.compare_to_numpy(eng.compare_raw(1, res.wav + 4 * int(got["offsets"][b]), wav_ptr + 4 * int(offs_in[b]), got["lens_out"][b:b + 1], dev))
        rd.append(removed_db(cmp["sum_d2"], cmp["sum_y2"])[0])
    return np.array(rd, np.float64)


def _flac(eng, plan: ChainPlan, wav_ptr: int, lens, pcm_i16: Optional[int], delivered) -> List[Optional[bytes]]:
    """The selected segments as FLAC streams (None for the others), read where the module docstring says."""
    dev, fc = _ffi.EV_FLAG_DEVICE_INPUTS, plan.flac_config
    sel = np.ones(len(lens), bool) if plan.flac is True else plan.flac
    out: List[Optional[bytes]] = [None] * len(sel)
    if delivered is not None:
        for b in np.flatnonzero(sel).tolist():
            fr = eng.flac_raw(1, delivered.data + int(delivered.byte_offsets[b]), True, [int(delivered.n_samples[b])], fc, dev)
            out[b] = eng.flac_to_numpy(fr)["streams"][0]
        return out
    offsets = offsets_of(lens)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], sel, [0]]).astype(np.int8)))      # where a run begins, where it ends, ...
    for b, e in zip(edges[::2].tolist(), edges[1::2].tolist()):
        src = pcm_i16 + 2 * int(offsets[b]) if pcm_i16 else wav_ptr + 4 * int(offsets[b])
        fr = eng.flac_raw(e - b, src, bool(pcm_i16), np.diff(offsets[b:e + 1]), fc, dev)
        out[b:e] = eng.flac_to_numpy(fr)["streams"]
    return out


def run(eng, plan: ChainPlan, wav_ptr: int, lens, want_int16: bool = False, int16_only: bool = False, source_i16: Optional[int] = None) -> ChainOutput:
    """The stages of ``plan`` on the source's packed device fp32 waveform ``wav_ptr`` (``lens`` samples per segment; ``source_i16``: its int16,
    where the source made one that FLAC may read).  want_int16: the caller wants the last waveform stage's int16 (or FLAC will read it);
    int16_only: as ``*_to_numpy`` reads it.  eng: the EVEngine, whose setup caches the stages share with its host-array calls."""
    dev, B = _ffi.EV_FLAG_DEVICE_INPUTS, len(lens)
    stages = plan.waveform_stages()
    figures, last, got, gains = {}, None, {}, None
    for i, (stage, cfg) in enumerate(stages):
        is_last = i == len(stages) - 1 and plan.delivery is None      # the one decision: this stage's audio is the response
        cfg = dataclasses.replace(cfg, want_int16=bool(is_last and (cfg.want_int16 or want_int16)))
        copy = dict(int16_only=int16_only, skip_wav=not is_last)
        if stage == "denoise":
            eng._setup_for("denoise", cfg.validate().key(), cfg)
            last = eng.denoise_raw(B, wav_ptr, False, lens, None, dev)
            got = figures["denoise"] = eng.denoise_to_numpy(last, **copy)
            if cfg.report:
                got["removed_db"] = _removed_db(eng, last, got, wav_ptr, lens)
            wav_ptr, lens = last.wav, got["lens_out"]      # denoise may change the lengths
        elif stage == "stretch":
            lens_in = np.asarray(lens, np.int64).copy()
            last = eng.stretch_raw(B, wav_ptr, False, lens_in, cfg.lengths(lens_in, plan.sample_rate), cfg, dev)
            got = figures["stretch"] = eng.stretch_to_numpy(last, **copy)
            got["lens_in"], got["speed"] = lens_in, lens_in / got["lens_out"]
            wav_ptr, lens = last.wav, got["lens_out"]      # the later stages read the new lengths
        elif stage == "watermark":
            last = eng.watermark_raw(B, wav_ptr, False, lens, cfg, dev)
            got = figures["watermark"] = eng.watermark_to_numpy(last, **copy)
            payloads, nbits, strengths = cfg.per_segment(B)
            got.update(key=int(cfg.key), payload=payloads, nbits=nbits, strength_db=strengths)
            wav_ptr, lens = last.wav, got["lens_out"]      # whole hops: the mark may shorten a segment, as denoise may
        elif stage == "measure":      # no audio out: the limiter reads what this stage read
            res = eng.loudness_raw(B, wav_ptr, False, lens, dataclasses.replace(cfg, target_lufs=float("nan")), dev)
            got = figures["loudness"] = eng.loudness_to_numpy(res, **copy)
            pairs = [pre_gain(float(l), plan.loudness) for l in got["loudness"]]
            gains = np.array([g for g, _ in pairs], np.float32)
            got["gain"], got["flags"] = gains.copy(), np.array([f for _, f in pairs], np.uint8)
        elif stage == "loudness":
            last = eng.loudness_raw(B, wav_ptr, False, lens, cfg, dev)
            got = figures["loudness"] = eng.loudness_to_numpy(last, **copy)
            wav_ptr = last.wav
        else:
            last = eng.limit_raw(B, wav_ptr, False, lens, gains, cfg, dev)
            got = figures["limiter"] = eng.limit_to_numpy(last, **copy)
            wav_ptr = last.wav
    out = ChainOutput({k: got.pop(k) for k in AUDIO_KEYS if k in got}, figures, last)
    if plan.delivery is not None:
        eng._setup_for("deliver", plan.delivery.key(plan.sample_rate), plan.delivery, plan.sample_rate)
        out.delivered = eng.deliver_raw(B, wav_ptr, False, lens, None, dev)
        got = eng.deliver_to_numpy(out.delivered, plan.delivery)
        out.audio = dict(delivered_list=got["delivered_list"], delivered_rate=int(plan.delivery.sample_rate),
                         delivery=dict(peak=got["peak"], clipped=got["clipped"], n_samples=got["n_samples"], encoding=plan.delivery.encoding))
    if plan.flac is not None:
        out.flac_list = _flac(eng, plan, wav_ptr, lens, last.wav_i16 if last is not None else source_i16, out.delivered)
    return out
