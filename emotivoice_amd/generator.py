"""Drop-in mirror of the reference's ``JETSGenerator`` object protocol on top of libevhip.so.

The reference boundary for the hot path is a Python object:
``JETSGenerator(conf).to(device)``, ``.load_state_dict(ckpt['generator'])``, ``.eval()`` and
``generator(inputs_ling=..., inputs_style_embedding=..., input_lengths=..., inputs_content_embedding=...,
inputs_speaker=..., alpha=1.0)`` returning a dict whose ``wav_predictions`` the callers scale to int16
(models/prompt_tts_modified/jets.py:26-71, inference_am_vocoder_joint.py:70-74,122-131).
``JETSGeneratorHIP`` keeps names, argument meaning, return keys and error behaviour; everything between is
the C ABI of include/evhip.h.  Only the inference branch exists: ``mel_targets`` must be None.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _ffi
from .config import EVShapes, from_reference_config
from .engine import EVEngine, EVError
from .packer import pack_state_dict

_IGNORED_PREFIXES = ("am.alignment_module.",)      # present in checkpoints, unused at inference


class _DevArray:
    """Expose a raw device pointer through __cuda_array_interface__ so torch can wrap it without a copy."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


# precision of the drop-in object when the caller names none (the one-line swap of INTEGRATION.md): the mode that meets north_star's 1e-3 on
# every fixture; __graft_entry__.smoke()'s first leg and bench.py's `value` run the same mode
DEFAULT_PRECISION = "mx"


class JETSGeneratorHIP:
    def __init__(self, config=None, decoder_precision: Optional[str] = None, keep_stages: bool = False, pe_len: int = 4096,
                 precision: Optional[str] = None, vocoder_precision: Optional[str] = None):
        """``precision``: "mx" (the contract mode: waveform within 1e-3 of the reference on every fixture; one fp16 MFMA + two
        block-scaled fp4 MFMAs per product), "fast" (fp16 MFMA operands and activations: 2x the speed, 2.4e-3 on zero-mean audio) or
        "strict" (split precision, ~1e-6).  With no precision argument at all the drop-in object runs "mx", so that the one-line swap
        described in INTEGRATION.md meets the 1e-3 contract without a flag (EVEngine() and the C ABI's ev_default_config resolve to the same mode since ABI 5).
        See engine.resolve_precision."""
        if precision is None and decoder_precision is None and vocoder_precision is None:
            precision = DEFAULT_PRECISION
        self.config = config
        self.shapes: EVShapes = from_reference_config(config)
        self.segment_size = self.shapes.segment_size
        self.upsample_factor = self.shapes.upsample_factor
        self._precision, self._dec_prec, self._voc_prec = precision, decoder_precision, vocoder_precision
        self._requested = (precision, decoder_precision, vocoder_precision)      # a verified load may move the three above to another rung
        self._keep, self._pe_len = keep_stages, pe_len
        self._device_id: Optional[int] = None
        self._engine: Optional[EVEngine] = None
        self._blob = None
        self._stream_ptr = 0            # 0 = the engine's own stream
        self._engine_kwargs: dict = {}  # EVEngine switches of the rung a verified load chose (load_state_dict(verify=...)); empty otherwise
        self.precision_report = None    # the PrecisionReport of the last verified load
        self.training = False

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    # ---- nn.Module-like surface used by the reference callers
    def to(self, device):
        dev_id = device if isinstance(device, int) else None
        if dev_id is None:
            s = str(device)
            if s == "cpu":
                raise EVError("JETSGeneratorHIP has no CPU path: it needs a HIP device (cuda:N)")
            dev_id = int(s.split(":")[1]) if ":" in s else 0
        if self._engine is not None and dev_id != self._device_id:
            self._engine.close()
            self._engine = None
        self._device_id = dev_id
        self._ensure_engine()
        return self

    def cuda(self, device=0):
        return self.to(device if isinstance(device, int) else str(device))

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("training is out of scope: JETSGeneratorHIP implements the inference branch of jets.py:61-66")
        return self

    def _ensure_engine(self):
        if self._engine is None:
            self._engine = EVEngine(self.shapes, self._device_id or 0, decoder_precision=self._dec_prec, keep_stages=self._keep,
                                    vocoder_precision=self._voc_prec, precision=self._precision, **self._engine_kwargs)
            self._stream_ptr = 0
            if self._blob is not None:
                self._engine.load_blob(*self._blob)
        return self._engine

    def load_state_dict(self, state_dict, strict: bool = True, verify=None):
        """Accepts ``ckpt['generator']`` (422 tensors, ``am.*`` / ``generator.*``; torch>=2.1 parametrization keys or the
        legacy weight_g / weight_v keys).  strict=True mirrors torch: a missing tensor raises KeyError.
        verify: None = load only.  True, or a dict of precision_guard.choose_precision keyword arguments (probe, bar, guard, ladder): after
        packing, an object that runs "mx" measures its waveform against a strict engine on the device and moves to the cheapest rung of
        the ladder that holds the bar (one warning when that is not the first); the report stays in ``precision_report``.  "fast" and
        "strict" objects are explicit opt-ins and load as without it.  Needs the device at load time.  The rung and the report belong to
        the weights they were measured on: a later load without ``verify`` (or ``load_packed``) returns the object to the precision it was
        constructed with and clears ``precision_report``."""
        if strict:
            known = ("am.", "generator.", "module.am.", "module.generator.")
            bad = [k for k in state_dict if not k.startswith(known)]
            if bad:
                raise RuntimeError("Unexpected key(s) in state_dict: " + ", ".join(bad[:5]))
        self._blob = pack_state_dict(state_dict, self.shapes, self._pe_len)
        if verify is None or verify is False:
            moved = self._move_to(self._requested, {})
            self.precision_report = None
        else:
            moved = self._verify_precision({} if verify is True else dict(verify))
        if self._engine is not None and not moved:      # an engine rebuilt on another rung has loaded the blob already
            self._engine.load_blob(*self._blob)
        return self

    def _move_to(self, precisions, engine_kwargs) -> bool:
        """Puts the object on (precision, decoder_precision, vocoder_precision) + EVEngine switches; True when that replaced a live engine
        (the new one has loaded the blob).  Its stream is the engine's own again until the next forward with device tensors attaches torch's."""
        from .engine import resolve_precision
        if resolve_precision(*precisions) == resolve_precision(self._precision, self._dec_prec, self._voc_prec) and engine_kwargs == self._engine_kwargs:
            return False
        had_engine = self._engine is not None
        self.close()
        (self._precision, self._dec_prec, self._voc_prec), self._engine_kwargs = precisions, dict(engine_kwargs)
        if had_engine:
            self._ensure_engine()
        return had_engine

    def _verify_precision(self, kwargs) -> bool:
        """Runs the precision guard on the packed blob and moves the object to the chosen rung; True when that replaced a live engine."""
        from .engine import resolve_precision
        from .precision_guard import choose_precision
        self.precision_report = None
        if resolve_precision(*self._requested) != ("mx", "mx"):
            return self._move_to(self._requested, {})
        kwargs.setdefault("device", self._device_id or 0)
        rep = choose_precision(self.shapes, self._blob, **kwargs)
        self.precision_report = rep
        if rep.escalated:
            import warnings
            warnings.warn("this checkpoint misses the precision bar in the default mode; running %s %s instead.  %s"
                          % (rep.chosen, rep.chosen_kwargs or "", rep.line()), RuntimeWarning, stacklevel=3)
        return self._move_to((rep.chosen, None, None), rep.chosen_kwargs)

    def load_packed(self, blob: bytes, manifest_json: Optional[str] = None):
        self._blob = (blob, manifest_json)
        moved = self._move_to(self._requested, {})
        self.precision_report = None
        if self._engine is not None and not moved:
            self._engine.load_blob(blob, manifest_json)
        return self

    # ---- forward
    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    def forward(self, inputs_ling, input_lengths, inputs_speaker, inputs_style_embedding, inputs_content_embedding,
                mel_targets=None, output_lengths=None, pitch_targets=None, energy_targets=None, alpha=1.0, cut_flag=True):
        if mel_targets is not None:
            raise NotImplementedError("teacher-forced / training branch (mel_targets) is out of scope")
        if self._blob is None:
            raise EVError("load_state_dict() must be called before forward()")
        if self._device_id is None:
            raise EVError("call .to('cuda:N') first: there is no CPU path")
        eng = self._ensure_engine()
        is_torch = hasattr(inputs_ling, "detach")
        if is_torch and inputs_ling.is_cuda:
            return self._forward_device(eng, inputs_ling, input_lengths, inputs_speaker, inputs_style_embedding, inputs_content_embedding)
        if self._stream_ptr:
            eng.set_stream(0)
            self._stream_ptr = 0

        def host(x, dt):
            if hasattr(x, "detach"):
                x = x.detach().cpu().numpy()
            return np.ascontiguousarray(np.asarray(x), dtype=dt)

        ling = host(inputs_ling, np.int64)
        if ling.ndim == 1:
            ling = ling[None]
        lengths = host(input_lengths, np.int64).reshape(-1)
        B, Nmax = ling.shape
        if lengths.shape[0] != B or lengths.max() > Nmax or lengths.min() <= 0:
            raise ValueError("input_lengths inconsistent with inputs_ling")
        if ling.min() < 0 or ling.max() >= self.shapes.n_vocab:
            raise IndexError("phoneme id out of range")          # nn.Embedding raises IndexError as well
        spk = host(inputs_speaker, np.int64).reshape(-1)
        if spk.min() < 0 or spk.max() >= self.shapes.n_speaker:
            raise IndexError("speaker id out of range")
        style = host(inputs_style_embedding, np.float32).reshape(B, -1)
        content = host(inputs_content_embedding, np.float32).reshape(B, -1)
        packed = np.ascontiguousarray(np.concatenate([ling[b, :lengths[b]] for b in range(B)]))
        cu = np.zeros(B + 1, np.int32)
        cu[1:] = np.cumsum(lengths)
        # alpha: the reference's inference branch calls the length regulator without it (model_open_source.py:142; alpha only
        # reaches GaussianUpsampling in the teacher-forced branch :138), so any value gives the alpha = 1 result there, and
        # here.  Speed control is available on the engine (EVEngine.synthesize(alpha=...), ev_synthesize's alpha).
        del alpha
        res = eng.synthesize_raw(B, packed.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data, 1.0, 0)
        T = np.array([res.mel_lens[b] for b in range(B)], np.int64)
        offs = np.array([res.mel_offsets[b] for b in range(B + 1)], np.int64)
        up = self.upsample_factor
        if is_torch:
            out = self._gather_torch(eng, res, B, Nmax, lengths, cu, T, offs, up)
            # host inputs run on the engine's own stream; the copies above were queued on torch's current stream and read the
            # handle's arena, which the next call may overwrite: finish them before returning
            import torch
            torch.cuda.current_stream(torch.device("cuda", self._device_id)).synchronize()
        else:
            out = self._gather_numpy(eng, res, B, Nmax, lengths, cu, T, offs, up)
        out.update(mel_targets=None, postnet_outputs=None, pitch_targets=None, energy_targets=None, duration_targets=None,
                   input_lengths=input_lengths, output_lengths=None, log_p_attn=None, bin_loss=None, z_start_idxs=None,
                   segment_size=self.segment_size)
        return out

    def _forward_device(self, eng, inputs_ling, input_lengths, inputs_speaker, inputs_style_embedding, inputs_content_embedding):
        """The reference's own call pattern (inference_am_vocoder_joint.py:115-129): every input already a CUDA tensor.  Nothing
        is staged through the host: the engine reads the tensors in place (EV_FLAG_DEVICE_INPUTS) and, when torch's current stream
        is a real stream, runs ON it (ev_set_stream), the outputs are cloned on the same stream, and ordering against later torch
        work is the stream's.  When the current stream is the DEFAULT stream (handle 0, which ev_set_stream maps to the engine's own
        non-blocking stream: no implicit ordering against the null stream), the call is fenced by hand instead: the input
        preparation is finished before the engine starts, and the output clones before the arena can be reused.  One small
        device -> host copy remains, the lengths (the reference synchronises too, alignment.py:195).
        Ids are not range-checked on this path (that would be a second sync): the kernels clamp them to the tables."""
        import torch
        dev = inputs_ling.device
        if dev.index is not None and self._device_id is not None and dev.index != self._device_id:
            raise EVError("inputs live on cuda:%d, the generator on cuda:%d" % (dev.index, self._device_id))
        stream = torch.cuda.current_stream(dev)
        if stream.cuda_stream != self._stream_ptr:
            eng.set_stream(stream.cuda_stream)
            self._stream_ptr = stream.cuda_stream
        ling = inputs_ling.long()
        if ling.dim() == 1:
            ling = ling[None]
        B, Nmax = ling.shape
        lengths = (input_lengths.detach().reshape(-1).to("cpu") if hasattr(input_lengths, "detach")
                   else torch.as_tensor(np.asarray(input_lengths)).reshape(-1)).to(torch.int64).numpy()
        if lengths.shape[0] != B or lengths.max() > Nmax or lengths.min() <= 0:
            raise ValueError("input_lengths inconsistent with inputs_ling")
        if B == 1 and int(lengths[0]) == Nmax:
            packed = ling.reshape(-1).contiguous()
        else:
            packed = torch.cat([ling[b, :int(lengths[b])] for b in range(B)]).contiguous()
        as_dev = lambda x, dt: (x if hasattr(x, "detach") else torch.as_tensor(np.asarray(x))).to(dev, dt)   # noqa: E731
        spk = as_dev(inputs_speaker, torch.int64).reshape(-1).contiguous()
        style = as_dev(inputs_style_embedding, torch.float32).reshape(B, -1).contiguous()
        content = as_dev(inputs_content_embedding, torch.float32).reshape(B, -1).contiguous()
        cu = np.zeros(B + 1, np.int32)
        cu[1:] = np.cumsum(lengths)
        fenced = stream.cuda_stream == 0
        if fenced:
            stream.synchronize()            # the cat / casts above were queued on the null stream; the engine's stream does not wait for it
        res = eng.synthesize_raw(B, packed.data_ptr(), cu, spk.data_ptr(), style.data_ptr(), content.data_ptr(), 1.0,
                                 _ffi.EV_FLAG_DEVICE_INPUTS)
        T = np.array([res.mel_lens[b] for b in range(B)], np.int64)
        offs = np.array([res.mel_offsets[b] for b in range(B + 1)], np.int64)
        out = self._gather_torch(eng, res, B, Nmax, lengths, cu, T, offs, self.upsample_factor)
        if fenced:
            stream.synchronize()            # the clones read the handle's arena, which the next call overwrites
        out.update(mel_targets=None, postnet_outputs=None, pitch_targets=None, energy_targets=None, duration_targets=None,
                   input_lengths=input_lengths, output_lengths=None, log_p_attn=None, bin_loss=None, z_start_idxs=None,
                   segment_size=self.segment_size)
        return out

    def _gather_numpy(self, eng, res, B, Nmax, lengths, cu, T, offs, up):
        r = eng.result_to_numpy(res)
        Tm = int(T.max())
        wav = np.zeros((B, 1, Tm * up), np.float32)
        mel = np.zeros((B, Tm, self.shapes.n_mels), np.float32)
        dur = np.zeros((B, Nmax), np.int64)
        pit = np.zeros((B, Nmax), np.float32)
        ene = np.zeros((B, Nmax), np.float32)
        for b in range(B):
            wav[b, 0, :T[b] * up] = r["wav_list"][b]
            mel[b, :T[b]] = r["mel_list"][b]
            dur[b, :lengths[b]] = r["durations"][cu[b]:cu[b + 1]]
            pit[b, :lengths[b]] = r["pitch"][cu[b]:cu[b + 1]]
            ene[b, :lengths[b]] = r["energy"][cu[b]:cu[b + 1]]
        return dict(wav_predictions=wav, dec_outputs=mel, log_duration_predictions=dur, pitch_predictions=pit.squeeze(),
                    energy_predictions=ene.squeeze())

    def _gather_torch(self, eng, res, B, Nmax, lengths, cu, T, offs, up):
        import torch
        dev = torch.device("cuda", self._device_id)
        try:
            wav_flat = torch.as_tensor(_DevArray(res.wav, (res.total_samples,), "<f4"), device=dev)
            mel_flat = torch.as_tensor(_DevArray(res.mel, (res.total_frames, self.shapes.n_mels), "<f4"), device=dev)
            dur_flat = torch.as_tensor(_DevArray(res.durations, (res.total_tokens,), "<i8"), device=dev)
            pit_flat = torch.as_tensor(_DevArray(res.pitch, (res.total_tokens,), "<f4"), device=dev)
            ene_flat = torch.as_tensor(_DevArray(res.energy, (res.total_tokens,), "<f4"), device=dev)
        except Exception:       # no __cuda_array_interface__ support in this torch build: stage through the host
            r = eng.result_to_numpy(res)
            wav_flat, mel_flat = torch.from_numpy(r["wav"]).to(dev), torch.from_numpy(r["mel"]).to(dev)
            dur_flat, pit_flat, ene_flat = (torch.from_numpy(r[k]).to(dev) for k in ("durations", "pitch", "energy"))
        Tm = int(T.max())
        if B == 1:               # the reference's only call pattern: plain views + clone, no padding work
            wav = wav_flat.clone().view(1, 1, -1)
            mel = mel_flat.clone().view(1, Tm, -1)
            dur, pit, ene = dur_flat.clone().view(1, -1), pit_flat.clone().view(1, -1), ene_flat.clone().view(1, -1)
        else:
            wav = torch.zeros(B, 1, Tm * up, device=dev)
            mel = torch.zeros(B, Tm, self.shapes.n_mels, device=dev)
            dur = torch.zeros(B, Nmax, dtype=torch.int64, device=dev)
            pit, ene = torch.zeros(B, Nmax, device=dev), torch.zeros(B, Nmax, device=dev)
            for b in range(B):
                wav[b, 0, :T[b] * up] = wav_flat[offs[b] * up:offs[b + 1] * up]
                mel[b, :T[b]] = mel_flat[offs[b]:offs[b + 1]]
                dur[b, :lengths[b]] = dur_flat[cu[b]:cu[b + 1]]
                pit[b, :lengths[b]] = pit_flat[cu[b]:cu[b + 1]]
                ene[b, :lengths[b]] = ene_flat[cu[b]:cu[b + 1]]
        return dict(wav_predictions=wav, dec_outputs=mel, log_duration_predictions=dur, pitch_predictions=pit.squeeze(),
                    energy_predictions=ene.squeeze())
