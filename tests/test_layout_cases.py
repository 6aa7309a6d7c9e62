"""CPU checks of tests/layout_cases.py: every listed layout is accepted by the restated ev_create rules, packs, gets exactly the fp4 plane
entries the packer's shape rules predict (the planner's choices hang on them), has a reference waveform away from the tanh's saturation, and an
fp32 oracle that sits far inside the strict bound -- so that what tests/test_gpu_layouts.py measures on the device is about the device."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import layout_cases as L  # noqa: E402

PLANE_SUFFIXES = ("wmx", "wcmx", "wpmx")


@pytest.fixture(scope="module", params=list(L.LAYOUTS))
def case(request):
    return L.build_case(request.param, keep_blob=False)


def test_tables_hold_the_listed_layouts():
    assert list(L.LAYOUTS) == ["default", "perm", "wide", "two", "one4", "odd", "s4", "up3", "up1"]
    for name, s in L.LAYOUTS.items():
        assert s.n_mels == 80 and s.upsample_factor == s.hop, name
        assert len(s.up_rates) == len(s.up_kernels) and len(s.rb_kernels) == len(s.rb_dils), name
    assert L.LAYOUTS["up3"].upsample_factor == 128 and L.LAYOUTS["up1"].upsample_factor == 16
    for s in L.AM_LAYOUTS.values():
        assert s.n_mels == 64 and (s.up_rates, s.rb_kernels, s.rb_dils) == (L.EVShapes().up_rates, L.EVShapes().rb_kernels, L.EVShapes().rb_dils)
    # the big call's padded frame rows exceed the plan's small-batch limit, the long mel alone stays below it
    rows = lambda lens: -(-(L.GAP + sum(n + L.GAP for n in lens)) // 256) * 256  # noqa: E731
    assert rows([L.BIG_LEN] * L.BIG_COPIES) > 2048 >= rows([L.BIG_LEN]) and rows(L.MEL_LENS) <= 2048


@pytest.mark.parametrize("name", list(L.LAYOUTS) + list(L.AM_LAYOUTS))
def test_accepted(name):
    assert L.accepted(L.LAYOUTS.get(name) or L.AM_LAYOUTS[name]) == "ok"


@pytest.mark.parametrize("name,names", [("halo_stage0", "ResBlock kernel 7 / dilation 3 at stage 0 exceeds the staged halo"),
                                        ("ch512_up3", "upsample_initial_channel / 2^n_up must be 32 (got 512 / 2^3)"),
                                        ("span72", "ResBlock kernel 13 / dilation 6 at stage 0 exceeds the staged halo")])
def test_near_misses_are_refused_with_a_reason(name, names):
    assert L.accepted(L.NEAR_MISSES[name]) == names


def test_plane_entries_are_the_predicted_ones(case):
    got = {k for k in case.manifest if k.startswith("voc.") and k.rsplit(".", 1)[1] in PLANE_SUFFIXES}
    want = L.predicted_planes(case.shapes)
    assert got == want, (case.name, sorted(got ^ want))
    # what the table says about single layouts
    if case.name == "up1":
        assert not any(k.endswith((".wmx", ".wcmx")) for k in got) and any(k.endswith(".wpmx") for k in got)
    if case.name == "odd":          # k = 5 / 9 have no planes at any width; the k = 3 ResBlock (the third) has them at every stage
        assert all(k.startswith("voc.up") or int(k.split(".")[1][2:]) % 3 == 2 for k in got) and "voc.up0.wmx" in got
    if case.name == "s4":           # the last up-conv (N = 128, K = 64) has neither plane kind
        assert not any(k.startswith("voc.up3.") for k in got) and "voc.up2.wmx" in got
    if case.name == "up3":
        assert "voc.up1.wmx" in got and not any(k.startswith("voc.up2.") for k in got)


def test_reference_is_not_saturated(case):
    assert [len(r) for r in case.refs] == [n * case.shapes.upsample_factor for n in L.MEL_LENS + (L.BIG_LEN,)]
    assert case.saturation() < L.SATURATION_MAX, (case.name, case.saturation())


def test_fp32_oracle_is_far_inside_the_strict_bound(case):
    from oracle.jets_oracle import hifigan_forward
    with torch.no_grad():
        errs = [L.rel_l2_ac(hifigan_forward(case.sd, torch.from_numpy(m), case.shapes).numpy(), r) for m, r in zip(case.mels, case.refs)]
    assert max(errs) < L.TOL_STRICT / 4, (case.name, errs)


def test_fp16_level_is_a_waveform_level(case):
    """the emulated fp16 level of every layout is of the size the project measured for its fp16 mode (2.2e-3 on zero-mean audio), never zero"""
    lv = case.fp16_levels()
    assert len(lv) == 4 and all(2e-4 < v < 1e-2 for v in lv), (case.name, lv)
    assert np.isfinite(lv).all()


@pytest.mark.parametrize("name", list(L.AM_LAYOUTS))
def test_am_layouts_pack_and_run_on_the_oracle(name):
    """ffn5 has no conv-FFN planes (5 taps), ffn7 has them; to_mel and voc.pre are zero-padded from 64 to MEL_PAD mels"""
    from oracle import am_forward, synth_inputs
    case = L.build_case(name, keep_blob=False)
    ffn = {k for k in case.manifest if k.startswith("dec.") and ".ffn" in k and k.endswith(".wmx")}
    assert ffn == ({"dec.%d.ffn%d.wmx" % (i, j) for i in range(3) for j in (1, 2)} if name == "ffn7" else set())
    assert case.manifest["to_mel.w32"]["shape"][0] == L.MEL_PAD and case.manifest["voc.pre.w16"]["shape"][2] == L.MEL_PAD
    assert "enc.2.qkv.b" not in case.manifest and "dec.2.qkv.b" in case.manifest and "dec.3.qkv.b" not in case.manifest
    utt = synth_inputs(51, [20], [9], shapes=case.shapes)[0]
    dur = torch.tensor([0, 3, 0, 0, 7, 1, 2, 0, 5, 4, 0, 0, 0, 6, 2, 2, 1, 0, 9, 3])
    with torch.no_grad():
        out = am_forward(case.sd, torch.from_numpy(utt["ling"]), 9, torch.from_numpy(utt["style"]), torch.from_numpy(utt["content"]), case.shapes, durations=dur)
    assert tuple(out["dec_outputs"].shape) == (int(dur.sum()), 64)


@pytest.mark.parametrize("dil", [0, 9, 32])
def test_fp16_c64_pair_refuses_a_dilation_its_slab_cannot_hold(dil):
    """resblock_pair_c64_kernel stages 272 rows per tile and conv1's 256 output rows read up to row 255 + 2 dil: dil <= 8.  ev_create accepts a
    C = 64, k = 3 conv up to dil = 32, so the planner runs wider ones layer by layer (layout "wide") and the per-kernel entry refuses them, before
    anything is launched."""
    import ctypes as C
    from emotivoice_amd import _ffi
    d = _ffi.ev_res_pair_desc()
    d.k, d.dil, d.M, d.ldx = 3, dil, 256, 64
    assert _ffi.lib().ev_op_resblock_pair_c64(C.byref(d), None) == -2
