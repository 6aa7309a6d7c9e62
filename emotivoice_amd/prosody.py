"""Per-utterance prosody controls for ev_synthesize_prosody (include/evhip.h: semantics, units, validation).

For utterance b and its token j the engine embeds ``pitch_scale * p_src[j] + pitch_shift`` (p_src = the override where one is
given and not NaN, else the predicted pitch), the same for energy, and upsamples with ``d_src[j]`` (the override where it is
``>= 0``, else the predicted duration) scaled by ``alpha``.  Units are the predictor's own: the checkpoint's normalised tracks.
``ev_result.pitch / .energy / .durations`` keep returning the predictions, so the round trip is: synthesise, edit those arrays,
synthesise again with them as overrides.

``pack_prosody`` validates on the host (``ValueError`` naming the field) and builds the ``ev_prosody`` struct plus the arrays it
points to.  Per-token arrays may be torch device tensors when the call passes ``EV_FLAG_DEVICE_INPUTS`` (``device=True``); their
values are then not range-checked here (the kernels treat non-finite pitch / energy and negative durations as "predicted" and clamp
durations at ``EV_PROSODY_MAX_DURATION``), but floating-point durations must hold whole numbers, as on the host.  The engine reads
device arrays on its own stream, which has no ordering against torch's: ``pack_prosody(device=True)`` therefore synchronises torch's
current stream of that device before it returns, so that the packed arrays -- and whatever the caller computed them from on that
stream -- are complete.  Tensors produced on another stream are the caller's to synchronise.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np

from . import _ffi

MAX_DURATION = _ffi.EV_PROSODY_MAX_DURATION


@dataclass
class Prosody:
    """Controls of one utterance.  ``speed`` and ``alpha`` are two spellings of the duration scale (alpha = 1 / speed); give at most
    one, neither = the call's alpha.  Per-token arrays have one value per phoneme of the utterance: ``pitch`` / ``energy`` (NaN =
    predicted), ``durations`` in mel frames (-1 = predicted)."""
    speed: Optional[float] = None
    alpha: Optional[float] = None
    pitch_scale: float = 1.0
    pitch_shift: float = 0.0
    energy_scale: float = 1.0
    energy_shift: float = 0.0
    pitch: Optional[object] = None
    energy: Optional[object] = None
    durations: Optional[object] = None

    def duration_scale(self) -> Optional[float]:
        """alpha of this utterance, or None when it leaves the call's alpha in place."""
        if self.speed is not None and self.alpha is not None:
            raise ValueError("give speed or alpha, not both")
        if self.speed is not None:
            s = float(self.speed)
            if not (math.isfinite(s) and s > 0):
                raise ValueError("speed %r must be > 0 and finite" % (self.speed,))
            return 1.0 / s
        if self.alpha is not None:
            a = float(self.alpha)
            if not (math.isfinite(a) and a > 0):
                raise ValueError("alpha %r must be > 0 and finite" % (self.alpha,))
            return a
        return None


class PackedProsody:
    """An ``ev_prosody`` struct and the arrays it points to (kept alive here for the duration of the call)."""

    def __init__(self, struct: _ffi.ev_prosody, device: bool, keep: List[object]):
        self.struct, self.device, self._keep = struct, device, keep


def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _ptr(a) -> int:
    return a.data_ptr() if _is_torch(a) else a.ctypes.data


def _per_token(items, lengths, field, dtype, fill, device, torch_device):
    """Packed (total_tokens,) array of one per-token field, or None when no utterance gives it."""
    if all(getattr(p, field) is None for p in items):
        return None
    parts = []
    for b, (p, n) in enumerate(zip(items, lengths)):
        v = getattr(p, field)
        if v is None:
            parts.append(np.full(n, fill, dtype))
            continue
        if _is_torch(v):
            if not device:
                v = v.detach().cpu().numpy()
            else:
                import torch
                if v.dim() != 1 or v.numel() != n:
                    raise ValueError("prosody[%d].%s: expected %d values, got shape %s" % (b, field, n, tuple(v.shape)))
                if dtype == np.int64:
                    if v.is_floating_point():
                        if not bool((torch.isfinite(v) & (v == v.round())).all()):
                            raise ValueError("prosody[%d].durations: values must be whole numbers of frames" % b)
                    elif v.is_complex() or v.dtype == torch.bool:
                        raise ValueError("prosody[%d].durations: integer values expected" % b)
        if not _is_torch(v):
            v = np.asarray(v)
            if v.ndim != 1 or v.size != n:
                raise ValueError("prosody[%d].%s: expected %d values, got shape %s" % (b, field, n, v.shape))
            if dtype == np.int64:
                if v.dtype.kind == "f":
                    if not np.isfinite(v).all() or not np.array_equal(v, np.round(v)):
                        raise ValueError("prosody[%d].durations: values must be whole numbers of frames" % b)
                elif v.dtype.kind not in "iu":
                    raise ValueError("prosody[%d].durations: integer values expected" % b)
                if not device and ((v < -1).any() or (v > MAX_DURATION).any()):
                    raise ValueError("prosody[%d].durations: values must lie in [-1, %d] (-1 = predicted)" % (b, MAX_DURATION))
            v = v.astype(dtype)
            if dtype == np.float32 and not device and np.isinf(v).any():
                raise ValueError("prosody[%d].%s: infinite value in fp32 (NaN = predicted)" % (b, field))
        parts.append(v)
    if not device:
        return np.ascontiguousarray(np.concatenate(parts), dtype)
    import torch
    tdt = torch.int64 if dtype == np.int64 else torch.float32
    return torch.cat([torch.as_tensor(x).to(device=torch_device, dtype=tdt).reshape(-1) for x in parts]).contiguous()


def pack_prosody(prosody: Union[Prosody, Sequence[Optional[Prosody]]], lengths: Sequence[int], alpha: float = 1.0,
                 device: bool = False, forced: bool = False, torch_device=None) -> PackedProsody:
    """``prosody``: one Prosody per utterance (None = identity), or a single Prosody for every utterance.  ``lengths``: phonemes per
    utterance.  ``alpha``: the call's duration scale (the default of utterances without speed / alpha).  ``device``: the call passes
    EV_FLAG_DEVICE_INPUTS, so the per-token arrays are packed as torch tensors on ``torch_device`` (default: the current CUDA
    device).  ``forced``: the call also uses EV_FLAG_FORCED_DURATIONS, which the engine rejects together with prosody."""
    with np.errstate(over="ignore"):          # a value beyond fp32's range becomes inf in the cast and is rejected as such
        return _pack(prosody, lengths, alpha, device, forced, torch_device)


def _pack(prosody, lengths, alpha, device, forced, torch_device) -> PackedProsody:
    if forced:
        raise ValueError("prosody cannot be combined with forced durations: use Prosody.durations")
    lengths = [int(n) for n in lengths]
    B = len(lengths)
    items = [prosody] * B if isinstance(prosody, Prosody) else list(prosody)
    if len(items) != B:
        raise ValueError("%d prosody entries for %d utterances" % (len(items), B))
    items = [p if p is not None else Prosody() for p in items]
    for b, p in enumerate(items):
        if not isinstance(p, Prosody):
            raise ValueError("prosody[%d] is %s, not a Prosody" % (b, type(p).__name__))
    if not (math.isfinite(alpha) and alpha > 0):
        raise ValueError("alpha %r must be > 0 and finite" % (alpha,))
    scales = []
    for b, p in enumerate(items):
        try:
            scales.append(p.duration_scale())
        except ValueError as e:
            raise ValueError("prosody[%d]: %s" % (b, e)) from None
        if scales[-1] is not None and not np.float32(scales[-1]) > 0:
            raise ValueError("prosody[%d]: duration scale %r is 0 in fp32" % (b, scales[-1]))
        for f in ("pitch_scale", "pitch_shift", "energy_scale", "energy_shift"):
            if not np.isfinite(np.float32(getattr(p, f))):
                raise ValueError("prosody[%d].%s = %r is not finite in fp32" % (b, f, getattr(p, f)))
    keep: List[object] = []
    st = _ffi.ev_prosody()
    st.struct_size = C.sizeof(_ffi.ev_prosody)
    if any(a is not None for a in scales):
        a = np.array([alpha if x is None else x for x in scales], np.float32)
        keep.append(a)
        st.alpha = a.ctypes.data
    for f in ("pitch_scale", "pitch_shift", "energy_scale", "energy_shift"):
        a = np.array([float(getattr(p, f)) for p in items], np.float32)
        keep.append(a)
        setattr(st, f, a.ctypes.data)
    if device and torch_device is None:
        import torch
        torch_device = torch.device("cuda", torch.cuda.current_device())
    for f, dt, fill in (("pitch", np.float32, np.nan), ("energy", np.float32, np.nan), ("durations", np.int64, -1)):
        a = _per_token(items, lengths, f, dt, fill, device, torch_device)
        if a is not None:
            keep.append(a)
            setattr(st, f, _ptr(a))
    if device:
        # the concatenations / casts above (and the caller's own work on this stream) run asynchronously on torch's current stream; the
        # engine copies the arrays on its own stream, which does not wait for that one (the fence generator._forward_device takes too)
        import torch
        torch.cuda.current_stream(torch_device).synchronize()
    return PackedProsody(st, device, keep)
