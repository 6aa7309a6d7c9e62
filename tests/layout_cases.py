"""Model layouts other than the default that ev_create accepts, and what the CPU side knows about each (no GPU import).

ev_create takes a family of layouts and make_voc_plan (ev_engine.cpp) turns one into a schedule through a dozen layout-dependent decisions.
LAYOUTS is a short list of generator layouts, each chosen for the planner arm it reaches; AM_LAYOUTS two acoustic-model layouts on the default
generator.  tests/test_layout_cases.py keeps these tables honest without a GPU; tests/test_gpu_layouts.py runs every one on the device.

What the helpers restate:
  accepted()           ev_create's layout rules, with ev_create's own messages (minus the "ev_create: " prefix)
  predicted_planes()   the packer's shape rules for the fp4 plane entries (.wmx / .wcmx / .wpmx) of the generator: the planner's choices hang on them
  oracle64()           hifigan_forward with every floating tensor in float64: the reference of the waveform bounds
  fp16_level()         tools/precision_study.emulate with fp16 weights, operands and storage everywhere, scored against oracle64 on the DC-free
                       measure: the level the fp16 mode is expected at for THIS layout and mel (the tanh and the layout's depth are in it)
"""
from __future__ import annotations

import dataclasses
import importlib.util
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from emotivoice_amd.config import EVShapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP, MEL_PAD = 4, 96          # ev_engine.cpp: gap rows between utterances, n_mels padded

TOL_STRICT = 2e-5             # tests/test_gpu_parity.py: every frame-rate quantity in the split-precision mode
TOL_MX = 1e-3                 # ... the contract mode, on every fixture
TOL_OUT = 1e-3                # ... north_star's bound for mel and waveform
FAST_ZDC = 3e-3               # ... fp16 operands on a zero-mean waveform (measured 2.2e-3)

# name -> EVShapes overrides.  Order: nearest to the default first (a fault far out must not hide the results nearer in).
_D = ((1, 3, 5),) * 3
LAYOUT_CHANGES: Dict[str, dict] = {
    "default": dict(),
    "perm": dict(rb_kernels=(11, 3, 7)),
    "wide": dict(rb_dils=((1, 3, 9), (1, 3, 9), (1, 3, 6))),
    "two": dict(rb_kernels=(3, 11), rb_dils=_D[:2]),
    "one4": dict(rb_kernels=(7,), rb_dils=((1, 2, 4, 8),)),
    "odd": dict(rb_kernels=(5, 9, 3), rb_dils=((1, 2), (1, 3), (2, 6))),
    "s4": dict(up_rates=(4, 4, 4, 4), up_kernels=(8, 8, 8, 8), rb_dils=((1, 3, 5), (1, 3, 5), (1, 2, 3))),
    "up3": dict(up_rates=(8, 4, 4), up_kernels=(16, 8, 8), up_init_ch=256, hop=128),
    "up1": dict(up_rates=(16,), up_kernels=(32,), up_init_ch=64, hop=16),
}
LAYOUTS: Dict[str, EVShapes] = {k: EVShapes(**v) for k, v in LAYOUT_CHANGES.items()}
# synth_state_dict gains where the default ones (rb_gain 2.2, post_gain = voc_gain 1.2) saturate the reference's tanh (SATURATION_MAX below).
# one4: a single ResBlock has no MRF mean over three branches to average its output down: reference std 0.88 with the default gains.
LAYOUT_GAINS: Dict[str, dict] = {"one4": dict(rb_gain=1.6, post_gain=0.6)}

_AM = dict(n_mels=64, enc_layers=2, dec_layers=3, dur_layers=3, pitch_layers=2, var_kernel=5, var_embed_kernel=3)
AM_LAYOUTS: Dict[str, EVShapes] = {"ffn5": EVShapes(ffn_kernel=5, **_AM), "ffn7": EVShapes(ffn_kernel=7, **_AM)}

# layouts one step outside the accepted family: (shapes, what ev_create's message must name)
NEAR_MISSES = {
    "halo_stage0": EVShapes(up_rates=(2, 2, 8, 8), up_kernels=(4, 4, 16, 16)),
    "ch512_up3": EVShapes(up_rates=(8, 8, 4), up_kernels=(16, 16, 8), up_init_ch=512),
    "span72": EVShapes(rb_kernels=(3, 7, 13), rb_dils=((1, 3, 5), (1, 3, 5), (1, 3, 6))),
}

MEL_LENS = (1, 5, 37)         # the ragged batch: fewer frames than any conv has taps, a few, and more than one tile at every stage
BIG_LEN, BIG_COPIES = 230, 9  # 9 x (230 + GAP) + GAP = 2110 frame rows -> 2304 > the plan's 2048-row small-batch limit; alone: 256 rows
SATURATION_MAX = 0.01         # fewer than 1 % of a layout's reference samples may have |x| > 0.99: a tanh that saturates hides errors


def accepted(s: EVShapes) -> str:
    """"ok", or the message ev_create refuses this layout with (its rules in its order)."""
    n_up, n_rb = len(s.up_rates), len(s.rb_kernels)
    n_dil = len(s.rb_dils[0]) if s.rb_dils else 0
    if s.hidden != 384 or s.heads != 8:
        return "only hidden=384 / heads=8 (d_k=48) kernels are built"
    if s.hidden % 128 or s.n_mels > MEL_PAD:
        return "unsupported shape"
    if not (1 <= n_up <= 4 and 1 <= n_rb <= 3 and 1 <= n_dil <= 4) or len(s.rb_dils) != n_rb or any(len(r) != n_dil for r in s.rb_dils) \
            or len(s.up_kernels) != n_up:
        return "generator layout outside the built range (n_up 1-4, n_rb 1-3, dilations 1-4)"
    for i in range(n_up):
        if s.up_kernels[i] != 2 * s.up_rates[i] or s.up_rates[i] & (s.up_rates[i] - 1):
            return "upsample stage %d must have kernel = 2*stride and a power-of-two stride" % i
    if (s.up_init_ch >> n_up) != 32 or s.up_init_ch & (s.up_init_ch - 1):
        return "upsample_initial_channel / 2^n_up must be 32 (got %d / 2^%d)" % (s.up_init_ch, n_up)
    if (s.ffn_kernel - 1) // 2 > GAP or (s.var_embed_kernel - 1) // 2 > GAP or (s.var_kernel - 1) // 2 > GAP or not s.ffn_kernel & 1 \
            or not s.var_embed_kernel & 1:
        return "token / frame-rate conv kernels must be odd and <= %d taps" % (2 * GAP + 1)
    U = 1
    for i in range(n_up):
        U *= s.up_rates[i]          # the cumulative stride INCLUDING this stage: its ResBlocks run at the stage's output rate
        for j in range(n_rb):
            for d in range(n_dil):
                k, dil = s.rb_kernels[j], s.rb_dils[j][d]
                span = (k - 1) * dil
                if not k & 1 or k < 1 or dil < 1 or span > 64 or span // 2 > GAP * U:
                    return "ResBlock kernel %d / dilation %d at stage %d exceeds the staged halo" % (k, dil, i)
    return "ok"


def generator_convs(s: EVShapes):
    """(blob name, N, K, taps) of every generator conv the packer lays out as a GEMM weight [N][taps][K] (packer.py)."""
    out = []
    ch, nk = s.up_init_ch, len(s.rb_kernels)
    for i, u in enumerate(s.up_rates):
        out.append(("voc.up%d" % i, u * (ch // 2), ch, 3))          # ConvTranspose1d(k = 2s) as a 3-tap polyphase conv
        ch //= 2
        for j, k in enumerate(s.rb_kernels):
            for d in range(len(s.rb_dils[j])):
                for c in ("c1", "c2"):
                    out.append(("voc.rb%d.%s.%d" % (i * nk + j, c, d), ch, ch, k))
    return out


def predicted_planes(s: EVShapes) -> set:
    """The voc.* plane entries the packer's shape rules give this layout: .wmx (N, K % 128 == 0; conv_gemm_mx_kernel), .wcmx (N = K = 64;
    conv_c64_mx_kernel and the fused C = 64 pair), .wpmx (ResBlock convs with N = K = 32; the fused C = 32 pair), each at 3 / 7 / 11 taps."""
    out = set()
    for name, N, K, taps in generator_convs(s):
        if taps not in (3, 7, 11):
            continue
        if N % 128 == 0 and K % 128 == 0:
            out.add(name + ".wmx")
        if N == 64 and K == 64:
            out.add(name + ".wcmx")
        if N == 32 and K == 32 and ".rb" in name:
            out.add(name + ".wpmx")
    return out


def rel_l2(a, b) -> float:
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rel_l2_ac(a, b) -> float:
    """relative L2 after removing the mean of the reference: the synthetic generator's waveform carries a DC offset of about three times its
    AC amplitude, which flatters the plain measure by that factor (tests/test_gpu_parity.py has the same definition)."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b - b.mean()), 1e-30))


_SD64: list = [None, None]          # one slot: (the fp32 dict it was made from, its float64 copy)


def _sd64(sd):
    if _SD64[0] is not sd:
        _SD64[0], _SD64[1] = sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items() if k.startswith("generator.")}
    return _SD64[1]


def oracle64(sd, mel, shapes: EVShapes, taps: Optional[dict] = None) -> np.ndarray:
    """hifigan_forward in float64.  sd: torch state dict (fp32), mel: (n_mels, T) array or tensor.  taps: as hifigan_forward fills them."""
    from oracle.jets_oracle import hifigan_forward
    with torch.no_grad():
        return hifigan_forward(_sd64(sd), torch.as_tensor(np.asarray(mel)).double(), shapes, taps).numpy()


_EMU = []


def _emulate():
    if not _EMU:
        spec = importlib.util.spec_from_file_location("ev_precision_study", os.path.join(ROOT, "tools", "precision_study.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _EMU.append(mod.emulate)
    return _EMU[0]


def fp16_wave(sd, mel, shapes: EVShapes) -> np.ndarray:
    """The waveform of the generator with fp16 weights, fp16 MFMA operands and fp16 storage at conv_pre and every stage (CPU emulation)."""
    recipe = [dict(w=1, a=1, s=1)] * (len(shapes.up_rates) + 1)
    gen = {k: v for k, v in sd.items() if k.startswith("generator.")}
    with torch.no_grad():
        return _emulate()(gen, torch.as_tensor(np.asarray(mel)).float(), shapes, recipe).numpy()


def fp16_level(sd, mel, shapes: EVShapes, ref64: Optional[np.ndarray] = None) -> float:
    return rel_l2_ac(fp16_wave(sd, mel, shapes), oracle64(sd, mel, shapes) if ref64 is None else ref64)


def make_mels(n_mels: int = 80) -> List[np.ndarray]:
    """The three short mels of the ragged batch and the long one, in the distribution of test_vocoder_only_and_int16."""
    rng = np.random.default_rng(5)
    return [(1.25 * rng.standard_normal((n_mels, T)) + 0.08).astype(np.float32) for T in MEL_LENS + (BIG_LEN,)]


@dataclasses.dataclass
class Case:
    name: str
    shapes: EVShapes
    sd: dict                        # torch fp32: generator.* only for a generator layout (the acoustic model is the default's), everything for an AM layout
    manifest: dict
    blob: Optional[bytes]          # with manifest_json: what EVEngine.load_blob takes
    manifest_json: str
    mels: List[np.ndarray]          # MEL_LENS + (BIG_LEN,)
    refs: List[np.ndarray]          # oracle64 of each mel
    levels: Optional[List[float]] = None      # fp16_level of each short mel, then of the three pooled
    level_big: Optional[float] = None

    def fp16_levels(self) -> List[float]:
        """fp16_level of each short mel and, last, of the ragged batch as a whole (the three waveforms end to end)."""
        if self.levels is None:
            waves = [fp16_wave(self.sd, m, self.shapes) for m in self.mels[:3]]
            self.levels = [rel_l2_ac(w, r) for w, r in zip(waves, self.refs[:3])]
            self.levels.append(rel_l2_ac(np.concatenate(waves), np.concatenate(self.refs[:3])))
        return self.levels

    def fp16_level_big(self) -> float:
        if self.level_big is None:
            self.level_big = fp16_level(self.sd, self.mels[3], self.shapes, self.refs[3])
        return self.level_big

    def saturation(self) -> float:
        x = np.concatenate(self.refs)
        return float((np.abs(x) > 0.99).mean())


def build_case(name: str, keep_blob: bool = True) -> Case:
    """Weights (synth_state_dict(0, "parity") at the layout, with the layout's gains), the packed blob, the mels and their float64 references."""
    import json
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    from oracle.jets_oracle import to_torch_sd
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    am = name in AM_LAYOUTS
    shapes = AM_LAYOUTS[name] if am else LAYOUTS[name]
    sd = synth_state_dict(0, "parity", shapes=shapes, **LAYOUT_GAINS.get(name, {}))
    blob, man = pack_state_dict(sd, shapes)
    tsd = to_torch_sd(sd if am else {k: v for k, v in sd.items() if k.startswith("generator.")})
    mels = make_mels(shapes.n_mels)
    refs = [] if am else [oracle64(tsd, m, shapes) for m in mels]
    return Case(name, shapes, tsd, json.loads(man), blob if keep_blob else None, man, mels, refs)
