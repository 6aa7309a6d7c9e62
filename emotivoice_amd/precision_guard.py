"""Guard a checkpoint's precision at load time: measure the cheap modes against ``strict`` on the device and take the cheapest one that holds the bar.

``strict`` is within 5e-6 of the fp32 reference on the device (tests/test_gpu_parity.py), so it serves as the yardstick where no oracle exists: a
rung of the ladder is synthesised on a probe batch with the yardstick's durations forced (EV_FLAG_FORCED_DURATIONS: equal lengths, frame for
frame comparable) and its device waveform goes into ``ev_compare`` beside the yardstick's -- no waveform is copied to the host.  The first rung
whose worst ``rel_l2_ac`` over the probe is at most ``bar * guard`` and that holds no non-finite sample wins; ``strict`` ends every ladder and
is accepted without a measurement.

    report = choose_precision(shapes, blob)              # blob: packer.pack_state_dict(...)
    EVEngine(shapes, precision=report.chosen, **report.chosen_kwargs)

``JETSGeneratorHIP.load_state_dict(sd, verify=True)`` runs this and rebuilds its engine on the chosen rung.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from .engine import EVEngine, EVError

Rung = Tuple[str, dict]

# in cost order: the default mode, the same with an fp32 residual stream (about +8 % time), split precision
LADDER: List[Rung] = [("mx", {}), ("mx", {"mx_residual": "fp32"}), ("strict", {})]
PROBE_SEED, PROBE_LENGTHS = 0, [64, 64, 96, 28]


def default_probe(shapes=None) -> List[dict]:
    from .synthetic import synth_inputs
    return synth_inputs(PROBE_SEED, PROBE_LENGTHS, shapes=shapes)


def is_yardstick(rung: Rung) -> bool:
    return rung[0] == "strict" and not rung[1]


@dataclass
class PrecisionReport:
    bar: float
    guard: float
    rungs: List[dict] = field(default_factory=list)      # one entry per rung tried, in ladder order
    chosen: Optional[str] = None
    chosen_kwargs: dict = field(default_factory=dict)
    chosen_index: int = -1

    @property
    def limit(self) -> float:
        return self.bar * self.guard

    @property
    def escalated(self) -> bool:
        return self.chosen_index > 0

    def as_dict(self) -> dict:
        return dict(bar=self.bar, guard=self.guard, limit=self.limit, chosen=self.chosen, chosen_kwargs=dict(self.chosen_kwargs),
                    chosen_index=self.chosen_index, escalated=self.escalated, rungs=[_jsonable(r) for r in self.rungs])

    def line(self) -> str:
        """One line for a log: every rung tried with its worst rel_l2_ac, and the choice."""
        parts = []
        for r in self.rungs:
            tag = r["name"] + ("(%s)" % ",".join("%s=%s" % kv for kv in sorted(r["kwargs"].items())) if r["kwargs"] else "")
            if not r["measured"]:
                parts.append("%s: yardstick" % tag)
            else:
                parts.append("%s: worst rel_l2_ac %.3g%s -> %s" % (tag, r["worst_rel_l2_ac"], ", %d non-finite" % r["nonfinite"] if r["nonfinite"] else "",
                                                                "ok" if r["accepted"] else "rejected"))
        return "precision guard (limit %.3g): %s; chosen %s %s" % (self.limit, "; ".join(parts), self.chosen, self.chosen_kwargs or "")


def _jsonable(x):
    if isinstance(x, dict):
        return {str(k): _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple, np.ndarray)):
        return [_jsonable(v) for v in (x.tolist() if isinstance(x, np.ndarray) else x)]
    if isinstance(x, (np.floating, float)):
        return float(x)
    if isinstance(x, (np.integer, int)) and not isinstance(x, bool):
        return int(x)
    return x


def worst_chunk(cmp: Dict[str, object]) -> dict:
    """The chunk with the largest sqrt(chunk_d2 / max(chunk_y2, floor)) of an EVEngine.compare result: (utterance, element offset, ratio)."""
    d2, y2, offs = np.asarray(cmp["chunk_d2"]), np.asarray(cmp["chunk_y2"]), np.asarray(cmp["chunk_offsets"])
    ratio = np.sqrt(d2) / np.sqrt(np.maximum(y2, _ffi.EV_COMPARE_FLOOR))
    c = int(np.argmax(ratio))
    u = int(np.searchsorted(offs, c, side="right") - 1)
    return dict(utterance=u, offset=int((c - offs[u]) * _ffi.EV_COMPARE_CHUNK), ratio=float(ratio[c]))


class DeviceMeasure:
    """``measure`` of choose_precision on the device: holds the strict yardstick engine and its result on the probe; every call builds one
    candidate engine, runs it with the yardstick's durations and compares on the device.  ``measure(None)`` compares the yardstick with itself
    (it counts the yardstick's own non-finite samples).  Close it when done."""

    def __init__(self, shapes, blob, probe: Optional[Sequence[dict]] = None, device: int = 0):
        self.shapes, self.device = shapes, device
        self.blob = blob if isinstance(blob, tuple) else (blob, None)
        self.probe = list(probe) if probe is not None else default_probe(shapes)
        self.yard = EVEngine(shapes, device, precision="strict")
        try:
            self.yard.load_blob(*self.blob)
            self.res, _ = self.yard._synthesize_call(self.probe, 1.0, 0, None, None)
            B = self.res.batch
            up = self.yard.shapes.upsample_factor
            mel_lens = np.array([self.res.mel_lens[b] for b in range(B)], np.int64)
            self.wav_lens, self.mel_elems = mel_lens * up, mel_lens * self.yard.shapes.n_mels
            self.durations = self.yard.d2h(self.res.durations, (self.res.total_tokens,), np.int64)
            if (mel_lens < 1).any():
                raise EVError("precision guard: the yardstick gives an empty utterance on the probe (durations all zero)")
        except Exception:
            self.yard.close()
            raise

    def close(self):
        self.yard.close()

    def _stats(self, res, own_mismatch: int) -> dict:
        B, dev = self.res.batch, _ffi.EV_FLAG_DEVICE_INPUTS
        wav = self.yard.compare_to_numpy(self.yard.compare_raw(B, res.wav, self.res.wav, self.wav_lens, dev))
        mel = self.yard.compare_to_numpy(self.yard.compare_raw(B, res.mel, self.res.mel, self.mel_elems, dev))
        return dict(rel_l2_ac=wav["rel_l2_ac"].tolist(), max_abs_d=wav["max_abs_d"].tolist(), mel_rel_l2=mel["rel_l2"].tolist(),
                    nonfinite=int(wav["nonfinite"].sum() + mel["nonfinite"].sum()), worst_chunk=worst_chunk(wav), duration_mismatch=own_mismatch)

    def __call__(self, rung: Optional[Rung]) -> dict:
        if rung is None:
            return self._stats(self.res, 0)
        name, kwargs = rung
        eng = EVEngine(self.shapes, self.device, precision=name, **kwargs)
        try:
            eng.load_blob(*self.blob)
            # the rung's own durations, from an unforced run of its acoustic model alone (no vocoder): what it would have used
            own, _ = eng._synthesize_call(self.probe, 1.0, _ffi.EV_FLAG_NO_VOCODER, None, None)
            mismatch = int((eng.d2h(own.durations, (own.total_tokens,), np.int64) != self.durations).sum())
            res, _ = eng._synthesize_call(self.probe, 1.0, 0, self.durations, None)
            return self._stats(res, mismatch)
        finally:
            eng.close()


def choose_precision(shapes, blob, probe: Optional[Sequence[dict]] = None, bar: float = 1e-3, guard: float = 1.0,
                     ladder: Sequence[Rung] = LADDER, device: int = 0, measure: Optional[Callable[[Optional[Rung]], dict]] = None) -> PrecisionReport:
    """The cheapest rung of ``ladder`` whose waveform stays within ``bar * guard`` (worst rel_l2_ac over the probe utterances, the yardstick's
    mean removed) of the ``strict`` engine on the same device, and holds no non-finite value.

    blob: the packed checkpoint, ``(bytes, manifest)`` as packer.pack_state_dict returns it, or the bytes.  probe: utterance dicts as
    EVEngine.synthesize takes them (default: synthetic.synth_inputs(0, [64, 64, 96, 28]); real text gives a measurement on real prosody).
    ladder: (precision name, EVEngine keyword arguments) in cost order; it must end on ("strict", {}), which is accepted by construction.
    measure: ``(rung) -> dict(rel_l2_ac=[per utterance], max_abs_d=[...], mel_rel_l2=[...], nonfinite=int, worst_chunk=dict,
    duration_mismatch=int)``, with ``measure(None)`` = the yardstick against itself; default: DeviceMeasure, which keeps one candidate engine
    alive beside the yardstick at any time.  A yardstick with non-finite output raises EVError: nothing can be judged against it."""
    ladder = [(str(n), dict(k)) for n, k in ladder]
    if not ladder or not is_yardstick(ladder[-1]):
        raise ValueError('the ladder must end on ("strict", {}): the rung that needs no measurement')
    if not (math.isfinite(bar) and bar > 0 and math.isfinite(guard) and guard > 0):
        raise ValueError("bar and guard must be positive and finite")
    own = measure is None
    if own:
        measure = DeviceMeasure(shapes, blob, probe, device)
    try:
        report = PrecisionReport(bar=float(bar), guard=float(guard))
        base = measure(None)
        if int(base["nonfinite"]) != 0:
            raise EVError("precision guard: the strict yardstick holds %d non-finite values on the probe; no mode can be judged against it"
                          % int(base["nonfinite"]))
        for i, (name, kwargs) in enumerate(ladder):
            if is_yardstick((name, kwargs)):
                report.rungs.append(dict(name=name, kwargs=kwargs, measured=False, accepted=True))
                report.chosen, report.chosen_kwargs, report.chosen_index = name, kwargs, i
                break
            st = dict(measure((name, kwargs)))
            worst = max(float(v) for v in st["rel_l2_ac"])
            ok = int(st["nonfinite"]) == 0 and worst <= report.limit      # a NaN ratio compares false
            st.update(name=name, kwargs=kwargs, measured=True, accepted=ok, worst_rel_l2_ac=worst)
            report.rungs.append(st)
            if ok:
                report.chosen, report.chosen_kwargs, report.chosen_index = name, kwargs, i
                break
        return report
    finally:
        if own:
            measure.close()
