"""MI355X: ev_synthesize_prosody -- per-utterance speed / pitch / energy controls and per-token overrides (include/evhip.h).  Identity
controls and round trips are bit-identical to ev_synthesize, a mixed batch equals separate calls, the controlled forward matches the CPU
oracle (tests/test_prosody.py::am_forward_prosody), device inputs, rejected inputs, and the plain call's launches."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_inputs, synth_state_dict
    from oracle.jets_oracle import to_torch_sd
    sd = synth_state_dict(0, "parity")
    blob, man = pack_state_dict(sd)
    engs = {}
    for prec in ("mx", "strict"):
        engs[prec] = EVEngine(precision=prec)
        engs[prec].load_blob(blob, man)
    yield dict(engs=engs, sd=to_torch_sd(sd), utts=synth_inputs(81, [37, 64], [3, 4]))
    for e in engs.values():
        e.close()


def _same(a, b, keys=("wav", "mel", "durations", "mel_lens", "pitch", "energy", "log_durations")):
    for k in keys:
        if k in a or k in b:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def _identity_list(utts):
    from emotivoice_amd.prosody import Prosody
    return [Prosody(
        alpha=1.0, pitch_scale=1.0, pitch_shift=0.0, energy_scale=1.0, energy_shift=0.0, pitch=np.full(len(u["ling"]), np.nan),
        energy=np.full(len(u["ling"]), np.nan), durations=np.full(len(u["ling"]), -1)) for u in utts]


def test_identity_controls_are_bitwise_ev_synthesize(ctx):
    from emotivoice_amd.prosody import Prosody
    utts = ctx["utts"]
    for prec, eng in ctx["engs"].items():
        base = eng.synthesize(utts)
        _same(eng.synthesize(utts, prosody=[None, None]), base)               # every pointer NULL
        _same(eng.synthesize(utts, prosody=_identity_list(utts)), base)     # explicit identity values
        cu = base["cu_seqlens"].astype(np.int64)
        spk = np.array([u["speaker"] for u in utts], np.int64)
        ling = np.concatenate([u["ling"] for u in utts])
        style = np.stack([u["style"] for u in utts]); content = np.stack([u["content"] for u in utts])
        res = eng.synthesize_prosody_raw(2, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data, 1.0, None, 0)
        _same(eng.result_to_numpy(res), base)                                # prosody == NULL
        # alpha[b] equal to the call's scalar alpha
        base13 = eng.synthesize(utts, alpha=1.3)
        _same(eng.synthesize(utts, alpha=1.3, prosody=[Prosody(alpha=1.3), Prosody()]), base13)
        # -0.0 shift / scale 1 is the identity too
        _same(eng.synthesize(utts, prosody=Prosody(pitch_shift=-0.0, energy_shift=-0.0)), base)


def test_identity_transform_copies_the_track_bits(ctx):
    """An utterance whose transform is the identity gets its source track bit for bit: an override of -0.0 stays -0.0 (fmaf(1, -0.0, +0.0)
    would give +0.0), read back through the "pitch_eff" / "energy_eff" taps; a real transform is one fmaf; without prosody the taps hold the
    predictions.  Host and device overrides alike."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.prosody import Prosody, pack_prosody
    from emotivoice_amd.synthetic import synth_state_dict
    eng = EVEngine(keep_stages=True)
    eng.load_blob(*pack_state_dict(synth_state_dict(0, "parity")))
    try:
        utts = ctx["utts"]
        n0, n1 = (len(u["ling"]) for u in utts)
        base = eng.synthesize(utts, vocoder=False)
        assert np.array_equal(eng.get_stage("pitch_eff"), base["pitch"]) and np.array_equal(eng.get_stage("energy_eff"), base["energy"])
        assert np.array_equal(eng.get_stage("dur_eff"), base["durations"])
        p0 = np.full(n0, np.nan, np.float32); p0[[2, 5, 11]] = -0.0
        e1 = np.full(n1, np.nan, np.float32); e1[[0, 7]] = -0.0
        pr = [Prosody(pitch=p0, pitch_scale=1.0, pitch_shift=0.0), Prosody(energy=e1, energy_shift=0.0, pitch_scale=2.0, pitch_shift=0.25)]
        want_p = base["pitch"].copy(); want_p[[2, 5, 11]] = -0.0
        want_p[n0:] = (np.float64(2.0) * base["pitch"][n0:].astype(np.float64) + 0.25).astype(np.float32)     # exact in fp64, one rounding like fmaf
        want_e = base["energy"].copy(); want_e[[n0, n0 + 7]] = -0.0
        host = eng.synthesize(utts, prosody=pr, vocoder=False)
        got_p, got_e = eng.get_stage("pitch_eff"), eng.get_stage("energy_eff")
        assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)) and np.array_equal(got_e.view(np.uint32), want_e.view(np.uint32))
        assert np.signbit(got_p[[2, 5, 11]]).all() and np.signbit(got_e[[n0, n0 + 7]]).all()
        ling, cu, spk, style, content = _device_args(utts)
        dpr = [Prosody(pitch=torch.from_numpy(p0).cuda()), Prosody(energy=torch.from_numpy(e1).cuda(), pitch_scale=2.0, pitch_shift=0.25)]
        res = eng.synthesize_prosody_raw(2, ling.data_ptr(), cu, spk.data_ptr(), style.data_ptr(), content.data_ptr(), 1.0,
                                         pack_prosody(dpr, [n0, n1], device=True), _ffi.EV_FLAG_DEVICE_INPUTS | _ffi.EV_FLAG_NO_VOCODER)
        _same(eng.result_to_numpy(res), host)
        assert np.array_equal(eng.get_stage("pitch_eff").view(np.uint32), want_p.view(np.uint32))
        assert np.array_equal(eng.get_stage("energy_eff").view(np.uint32), want_e.view(np.uint32))
    finally:
        eng.close()


def test_round_trip_of_the_returned_tracks_is_bitwise(ctx):
    from emotivoice_amd.prosody import Prosody
    utts = ctx["utts"]
    for prec, eng in ctx["engs"].items():
        base = eng.synthesize(utts)
        cu = base["cu_seqlens"]
        pr = [Prosody(pitch=base["pitch"][cu[b]:cu[b + 1]], energy=base["energy"][cu[b]:cu[b + 1]], durations=base["durations"][cu[b]:cu[b + 1]])
              for b in range(len(utts))]
        _same(eng.synthesize(utts, prosody=pr), base)


def _mixed_controls():
    from emotivoice_amd.prosody import Prosody
    alphas = [0.5, 1.0, 1.3, 2.0, 0.8, 1.0, 1.7, 1.0]
    return [Prosody(alpha=a, pitch_shift=0.1 * (i - 3), pitch_scale=1.0 + 0.05 * (i % 3), energy_scale=1.0 - 0.1 * (i % 4),
                    energy_shift=0.05 * (i % 2)) for i, a in enumerate(alphas)], alphas


def test_mixed_batch_equals_separate_calls_bitwise(ctx):
    from emotivoice_amd.prosody import Prosody
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["engs"]["mx"]
    utts = synth_inputs(85, [20, 33, 41, 28, 57, 16, 45, 30], [1, 2, 3, 4, 5, 6, 7, 8])
    ctrls, alphas = _mixed_controls()
    out = eng.synthesize(utts, prosody=ctrls)
    cu = out["cu_seqlens"]
    for b, u in enumerate(utts):
        one = eng.synthesize([u], prosody=[ctrls[b]])
        assert int(one["mel_lens"][0]) == int(out["mel_lens"][b]), b
        assert np.array_equal(one["mel"], out["mel_list"][b]) and np.array_equal(one["wav"], out["wav_list"][b]), b
        assert np.array_equal(one["durations"], out["durations"][cu[b]:cu[b + 1]]), b
    # per-utterance alpha alone == ev_synthesize(alpha = alpha_b)
    out = eng.synthesize(utts, prosody=[Prosody(alpha=a) for a in alphas])
    for b, (u, a) in enumerate(zip(utts, alphas)):
        ref = eng.synthesize([u], alpha=a)
        assert np.array_equal(ref["mel"], out["mel_list"][b]) and np.array_equal(ref["wav"], out["wav_list"][b]), (b, a)


def _oracle_cases(n):
    from emotivoice_amd.prosody import Prosody
    p_part = np.full(n, np.nan, np.float32)
    p_part[3:12] = np.linspace(-1.0, 2.5, 9)
    d_part = np.full(n, -1, np.int64)
    d_part[[0, 5, 9]] = 0
    d_part[[2, 14, 30]] = 12
    return {"pitch +0.5 x1.3": Prosody(pitch_shift=0.5, pitch_scale=1.3), "energy x0.7": Prosody(energy_scale=0.7),
            "partial pitch": Prosody(pitch=p_part), "partial durations": Prosody(durations=d_part),
            "durations all 0": Prosody(durations=np.zeros(n, np.int64)), "speed 0.5": Prosody(speed=0.5), "speed 2": Prosody(speed=2.0)}


def test_controls_match_the_oracle(ctx):
    from test_prosody import am_forward_prosody, effective_tracks
    from oracle import EVShapes
    from oracle.jets_oracle import hifigan_forward
    u = ctx["utts"][0]
    sd, shapes = ctx["sd"], EVShapes()
    pred = am_forward_prosody(sd, u["ling"], u["speaker"], u["style"], u["content"], shapes)
    base_mel = ctx["engs"]["mx"].synthesize([u], vocoder=True)["mel"]
    for name, pr in _oracle_cases(len(u["ling"])).items():
        p, e, d, a = effective_tracks(pred["pitch_predictions"].numpy(), pred["energy_predictions"].numpy(),
                                      pred["log_duration_predictions"].numpy(), pr)
        ref = am_forward_prosody(sd, u["ling"], u["speaker"], u["style"], u["content"], shapes, pitch=p, energy=e, durations=d, duration_scale=a)
        with torch.no_grad():
            wav_ref = hifigan_forward(sd, ref["dec_outputs"].t().contiguous(), shapes).numpy().astype(np.float64)
        for prec, tol_wav in (("mx", 1e-3), ("strict", 1e-4)):
            out = ctx["engs"][prec].synthesize([u], prosody=[pr])
            assert int(out["mel_lens"][0]) == int(ref["mel_len"]), (name, prec)
            assert np.array_equal(out["durations"], pred["log_duration_predictions"].numpy()), (name, prec)     # ev_result: the predictions
            assert np.array_equal(ctx["engs"][prec].get_stage("dur_eff"), d), (name, prec)                        # ... and what was upsampled
            e_mel = rel_l2(out["mel"], ref["dec_outputs"].numpy())
            diff = out["wav"].astype(np.float64) - wav_ref
            e_ac = float(np.linalg.norm(diff) / np.linalg.norm(wav_ref - wav_ref.mean()))        # the DC-free measure of smoke()
            print("%s %s: mel %.2e wav_ac %.2e frames %d" % (name, prec, e_mel, e_ac, int(out["mel_lens"][0])))
            assert e_mel < 1e-3 and e_ac < tol_wav, (name, prec, e_mel, e_ac)
            if prec == "mx" and out["mel"].shape == base_mel.shape:
                assert rel_l2(out["mel"], base_mel) > 1e-3, name        # the control really changes the output
    # the all-zero guard: every token one frame
    out = ctx["engs"]["mx"].synthesize([u], prosody=[_oracle_cases(len(u["ling"]))["durations all 0"]], vocoder=False)
    assert int(out["mel_lens"][0]) == len(u["ling"])


def _device_args(utts):
    ling = torch.from_numpy(np.concatenate([u["ling"] for u in utts])).cuda()
    spk = torch.tensor([u["speaker"] for u in utts], dtype=torch.int64).cuda()
    style = torch.from_numpy(np.stack([u["style"] for u in utts])).cuda()
    content = torch.from_numpy(np.stack([u["content"] for u in utts])).cuda()
    cu = np.zeros(len(utts) + 1, np.int32)
    cu[1:] = np.cumsum([len(u["ling"]) for u in utts])
    return ling, cu, spk, style, content


def test_device_per_token_arrays_equal_host_arrays(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.prosody import Prosody, pack_prosody
    eng, utts = ctx["engs"]["mx"], ctx["utts"]
    n0, n1 = (len(u["ling"]) for u in utts)
    pitch = np.full(n0, np.nan, np.float32); pitch[4:9] = 1.5
    dur = np.full(n1, -1, np.int64); dur[[1, 7]] = [0, 9]
    host_pr = [Prosody(pitch=pitch, pitch_shift=0.2, speed=1.25), Prosody(durations=dur, energy=np.linspace(0, 1, n1), energy_scale=0.9)]
    host = eng.synthesize(utts, prosody=host_pr)
    ling, cu, spk, style, content = _device_args(utts)
    dev_pr = [Prosody(pitch=torch.from_numpy(pitch).cuda(), pitch_shift=0.2, speed=1.25),
              Prosody(durations=torch.from_numpy(dur).cuda(), energy=torch.from_numpy(np.linspace(0, 1, n1).astype(np.float32)).cuda(), energy_scale=0.9)]
    pk = pack_prosody(dev_pr, [n0, n1], device=True)
    res = eng.synthesize_prosody_raw(2, ling.data_ptr(), cu, spk.data_ptr(), style.data_ptr(), content.data_ptr(), 1.0, pk, _ffi.EV_FLAG_DEVICE_INPUTS)
    _same(eng.result_to_numpy(res), host)
    # device values the host would reject: non-finite pitch / energy = predicted, negative durations = predicted, durations clamped at the cap
    odd_p = pitch.copy(); odd_p[[0, 1, 2]] = [np.inf, -np.inf, np.nan]
    odd_d = dur.copy(); odd_d[[3, 4]] = [-7, _ffi.EV_PROSODY_MAX_DURATION + 500]
    want_d = dur.copy(); want_d[4] = _ffi.EV_PROSODY_MAX_DURATION
    host = eng.synthesize(utts, prosody=[Prosody(pitch=pitch, speed=1.25), Prosody(durations=want_d)], vocoder=False)
    pk = pack_prosody([Prosody(pitch=torch.from_numpy(odd_p).cuda(), speed=1.25), Prosody(durations=torch.from_numpy(odd_d).cuda())], [n0, n1], device=True)
    res = eng.synthesize_prosody_raw(2, ling.data_ptr(), cu, spk.data_ptr(), style.data_ptr(), content.data_ptr(), 1.0, pk,
                                     _ffi.EV_FLAG_DEVICE_INPUTS | _ffi.EV_FLAG_NO_VOCODER)
    _same(eng.result_to_numpy(res), host)
    # device floating-point durations: whole numbers are accepted like on the host, others are not
    pk = pack_prosody([None, Prosody(durations=torch.from_numpy(dur.astype(np.float32)).cuda())], [n0, n1], device=True)
    res = eng.synthesize_prosody_raw(2, ling.data_ptr(), cu, spk.data_ptr(), style.data_ptr(), content.data_ptr(), 1.0, pk,
                                     _ffi.EV_FLAG_DEVICE_INPUTS | _ffi.EV_FLAG_NO_VOCODER)
    _same(eng.result_to_numpy(res), eng.synthesize(utts, prosody=[None, Prosody(durations=dur)], vocoder=False))
    with pytest.raises(ValueError, match="whole numbers"):
        pack_prosody([None, Prosody(durations=torch.full((n1,), 2.5, device="cuda"))], [n0, n1], device=True)
    with pytest.raises(ValueError, match="packed for host"):
        eng.synthesize_prosody_raw(2, ling.data_ptr(), cu, spk.data_ptr(), style.data_ptr(), content.data_ptr(), 1.0,
                                   pack_prosody([None, None], [n0, n1]), _ffi.EV_FLAG_DEVICE_INPUTS)


def test_device_overrides_computed_just_before_the_call_are_complete(ctx):
    """pack_prosody(device=True) fences torch's current stream: overrides that torch is still computing when the call is made (here behind a
    chain of large matmuls on the default stream) are read complete by the engine's own stream."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.prosody import Prosody, pack_prosody
    eng, utts = ctx["engs"]["mx"], ctx["utts"]
    n0, n1 = (len(u["ling"]) for u in utts)
    pitch = np.full(n0, np.nan, np.float32); pitch[::3] = np.linspace(-1.0, 2.0, len(pitch[::3]))
    dur = np.full(n1, -1, np.int64); dur[::5] = 7
    host = eng.synthesize(utts, prosody=[Prosody(pitch=pitch), Prosody(durations=dur)], vocoder=False)
    ling, cu, spk, style, content = _device_args(utts)
    torch.cuda.synchronize()
    for _ in range(3):
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(24):
            big = torch.tanh(big @ big * 1e-3)
        p_dev = torch.from_numpy(pitch).cuda() + 0.0 * big[0, :n0]          # the values are the host ones; their writes come last
        d_dev = torch.from_numpy(dur).cuda() + (0.0 * big[1, :n1]).long()
        pk = pack_prosody([Prosody(pitch=p_dev), Prosody(durations=d_dev)], [n0, n1], device=True)
        res = eng.synthesize_prosody_raw(2, ling.data_ptr(), cu, spk.data_ptr(), style.data_ptr(), content.data_ptr(), 1.0, pk,
                                         _ffi.EV_FLAG_DEVICE_INPUTS | _ffi.EV_FLAG_NO_VOCODER)
        _same(eng.result_to_numpy(res), host)


def test_rejected_inputs_name_the_field_and_leave_the_handle_usable(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVError
    from emotivoice_amd.prosody import PackedProsody
    eng, utts = ctx["engs"]["mx"], ctx["utts"]
    before = eng.synthesize(utts)
    ling = np.concatenate([u["ling"] for u in utts]); NT = ling.size
    spk = np.array([u["speaker"] for u in utts], np.int64)
    style = np.stack([u["style"] for u in utts]); content = np.stack([u["content"] for u in utts])
    cu = before["cu_seqlens"]

    def raw(flags=0, call_alpha=1.0, size=None, reserved=0, **arrays):
        st = _ffi.ev_prosody()
        st.struct_size = C.sizeof(_ffi.ev_prosody) if size is None else size
        st.reserved0 = reserved
        keep = []
        for k, v in arrays.items():
            a = np.ascontiguousarray(v, np.int64 if k == "durations" else np.float32)
            keep.append(a)
            setattr(st, k, a.ctypes.data)
        return eng.synthesize_prosody_raw(2, ling.ctypes.data, cu, spk.ctypes.data, style.ctypes.data, content.ctypes.data, call_alpha,
                                          PackedProsody(st, False, keep), flags)

    d_bad = np.full(NT, -1); d_bad[5] = -2
    d_big = np.full(NT, -1); d_big[7] = _ffi.EV_PROSODY_MAX_DURATION + 1
    p_inf = np.full(NT, np.nan); p_inf[3] = np.inf
    e_inf = np.full(NT, np.nan); e_inf[9] = -np.inf
    cases = [(dict(alpha=[1.0, 0.0]), r"prosody\.alpha\[1\]"), (dict(alpha=[np.nan, 1.0]), r"prosody\.alpha\[0\]"),
             (dict(alpha=[-1.0, 1.0]), r"prosody\.alpha\[0\]"), (dict(call_alpha=0.0), r"alpha 0 must be > 0"),
             (dict(pitch_scale=[1.0, np.inf]), r"prosody\.pitch_scale\[1\]"), (dict(pitch_shift=[np.nan, 0.0]), r"prosody\.pitch_shift\[0\]"),
             (dict(energy_scale=[np.inf, 1.0]), r"prosody\.energy_scale\[0\]"), (dict(energy_shift=[0.0, -np.inf]), r"prosody\.energy_shift\[1\]"),
             (dict(pitch=p_inf), r"prosody\.pitch\[3\]"), (dict(energy=e_inf), r"prosody\.energy\[9\]"),
             (dict(durations=d_bad), r"prosody\.durations\[5\] = -2"), (dict(durations=d_big), r"prosody\.durations\[7\] = 1025"),
             (dict(size=8), r"struct_size"), (dict(reserved=1), r"reserved0")]
    for kw, match in cases:
        with pytest.raises(EVError, match=match):
            raw(**kw)
        _same(eng.synthesize(utts), before)
    eng.set_forced_durations(before["durations"])
    with pytest.raises(EVError, match="EV_FLAG_FORCED_DURATIONS"):
        raw(flags=_ffi.EV_FLAG_FORCED_DURATIONS)
    _same(eng.synthesize(utts), before)


def test_plain_call_launches_nothing_new_and_prosody_cost_is_listed(ctx):
    eng, utts = ctx["engs"]["mx"], ctx["utts"]
    names = ("prosody_tracks", "durations_prosody")
    eng.set_profiling(True)
    try:
        eng.synthesize(utts)
        plain = eng.launch_records()
        t_plain = eng.timings()["variance"]
        eng.synthesize(utts, prosody=[None, None])
        pros = eng.launch_records()
        t_pros = eng.timings()["variance"]
    finally:
        eng.set_profiling(False)
    assert not [r for r in plain if r["name"] in names]
    assert [r["name"] for r in plain].count("durations") == 1
    extra = [r for r in pros if r["name"] in names]
    assert sorted(r["name"] for r in extra) == sorted(names) and "durations" not in [r["name"] for r in pros]
    assert len(pros) == len(plain) + 1                  # one launch more: the tracks kernel; durations runs its prosody instantiation
    print("prosody launches: %s; variance %.4f ms plain, %.4f ms with identity prosody" %
          (", ".join("%s %.4f ms" % (r["name"], r["ms"]) for r in extra), t_plain, t_pros))
