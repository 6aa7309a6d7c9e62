"""Prosody controls (ev_synthesize_prosody, emotivoice_amd/prosody.py) without a GPU: packing and validation, the ABI surface, the
CPU oracle of the controlled forward, and the opt-in mixed-prosody batcher."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

from emotivoice_amd import _ffi
from emotivoice_amd.prosody import MAX_DURATION, Prosody, pack_prosody
from emotivoice_amd.serving import DynamicBatcher, TTSService
from oracle.jets_oracle import duration_from_log, encoder_stack, gaussian_upsampling, predictor_trunk


# --------------------------------------------------------------------------- oracle of the controlled forward

def am_forward_prosody(sd, ling, speaker, style, content, shapes, pitch=None, energy=None, durations=None, duration_scale=1.0):
    """model_open_source.py:102-147 (inference branch) with the EFFECTIVE tracks fed where the predictions go, the way the teacher-forced
    branch feeds ps / es / ds (:113-139): ``pitch`` / ``energy`` (N,) fp32 into pitch_embed / energy_embed, ``durations`` (N,) int64 into
    the Gaussian upsampling with ``duration_scale`` (GaussianUpsampling's alpha).  None = the prediction.  Built from the oracle's
    public functions only; the returned *_predictions are the predictions, as ev_result returns them."""
    with torch.no_grad():
        ling = torch.as_tensor(ling).long()
        style, content = torch.as_tensor(style).float(), torch.as_tensor(content).float()
        tok = sd["am.src_word_emb.weight"][ling]
        x = encoder_stack(tok, sd, "am.encoder", shapes.enc_layers, shapes.heads)
        N = x.shape[0]
        spk = sd["am.spk_tokenizer.weight"][int(speaker)]
        cat = torch.cat([x, spk.expand(N, -1), style.expand(N, -1), content.expand(N, -1)], dim=-1)
        x = F.linear(cat, sd["am.embed_projection1.weight"], sd["am.embed_projection1.bias"])
        p_outs = predictor_trunk(x, sd, "am.pitch_predictor", shapes.pitch_layers)
        e_outs = predictor_trunk(x, sd, "am.energy_predictor", shapes.energy_layers)
        log_d = predictor_trunk(x, sd, "am.duration_predictor", shapes.dur_layers)
        d_outs = duration_from_log(log_d)
        p = p_outs if pitch is None else torch.as_tensor(np.asarray(pitch, np.float32))
        e = e_outs if energy is None else torch.as_tensor(np.asarray(energy, np.float32))
        d = d_outs if durations is None else torch.as_tensor(np.asarray(durations, np.int64))
        kp = sd["am.pitch_embed.0.weight"].shape[-1]
        p_emb = F.conv1d(p.view(1, 1, -1), sd["am.pitch_embed.0.weight"], sd["am.pitch_embed.0.bias"], padding=(kp - 1) // 2).squeeze(0).t()
        e_emb = F.conv1d(e.view(1, 1, -1), sd["am.energy_embed.0.weight"], sd["am.energy_embed.0.bias"], padding=(kp - 1) // 2).squeeze(0).t()
        x = x + p_emb + e_emb
        up, T = gaussian_upsampling(x, d, duration_scale)
        y = encoder_stack(up, sd, "am.decoder", shapes.dec_layers, shapes.heads)
        mel = F.linear(y, sd["am.to_mel.weight"], sd["am.to_mel.bias"])
    return dict(dec_outputs=mel, pitch_predictions=p_outs, energy_predictions=e_outs, log_duration_predictions=d_outs, mel_len=T)


def effective_tracks(pred_pitch, pred_energy, pred_dur, p: Prosody, call_alpha=1.0):
    """include/evhip.h's semantics on the host: (pitch, energy, durations, alpha) the engine embeds and upsamples for one utterance."""
    def track(pred, ovr, scale, shift):
        src = np.asarray(pred, np.float32).copy()
        if ovr is not None:
            o = np.asarray(ovr, np.float32)
            src = np.where(np.isnan(o), src, o).astype(np.float32)
        if scale == 1.0 and shift == 0.0:
            return src
        return (np.float64(np.float32(scale)) * src.astype(np.float64) + np.float64(np.float32(shift))).astype(np.float32)
    d = np.asarray(pred_dur, np.int64).copy()
    if p.durations is not None:
        o = np.asarray(p.durations, np.int64)
        d = np.where(o >= 0, np.minimum(o, MAX_DURATION), d)
    a = p.duration_scale()
    return (track(pred_pitch, p.pitch, p.pitch_scale, p.pitch_shift), track(pred_energy, p.energy, p.energy_scale, p.energy_shift), d,
            float(np.float32(call_alpha if a is None else a)))


@pytest.fixture(scope="module")
def oracle_ctx():
    from emotivoice_amd.synthetic import synth_inputs, synth_state_dict
    from oracle import EVShapes
    from oracle.jets_oracle import to_torch_sd
    return dict(sd=to_torch_sd(synth_state_dict(0, "parity")), shapes=EVShapes(), u=synth_inputs(81, [23], [3])[0])


def _run_oracle(ctx, **kw):
    u = ctx["u"]
    return am_forward_prosody(ctx["sd"], u["ling"], u["speaker"], u["style"], u["content"], ctx["shapes"], **kw)


def test_oracle_identity_controls_equal_am_forward_bitwise(oracle_ctx):
    from oracle.jets_oracle import am_forward
    u = oracle_ctx["u"]
    with torch.no_grad():
        ref = am_forward(oracle_ctx["sd"], torch.as_tensor(u["ling"]), u["speaker"], torch.as_tensor(u["style"]), torch.as_tensor(u["content"]),
                         oracle_ctx["shapes"])
    for alpha in (1.0, 1.3):
        with torch.no_grad():
            ref_a = ref if alpha == 1.0 else am_forward(oracle_ctx["sd"], torch.as_tensor(u["ling"]), u["speaker"], torch.as_tensor(u["style"]),
                                                         torch.as_tensor(u["content"]), oracle_ctx["shapes"], duration_scale=alpha)
        got = _run_oracle(oracle_ctx, duration_scale=alpha)
        assert got["mel_len"] == ref_a["mel_len"]
        assert torch.equal(got["dec_outputs"], ref_a["dec_outputs"])
        assert torch.equal(got["log_duration_predictions"], ref_a["log_duration_predictions"])
    # the host statement of the semantics: identity controls reproduce the predictions bit for bit
    n = len(u["ling"])
    ident = Prosody(pitch=np.full(n, np.nan), energy=np.full(n, np.nan), durations=np.full(n, -1))
    p, e, d, a = effective_tracks(ref["pitch_predictions"].numpy(), ref["energy_predictions"].numpy(), ref["log_duration_predictions"].numpy(), ident)
    assert np.array_equal(p, ref["pitch_predictions"].numpy()) and np.array_equal(e, ref["energy_predictions"].numpy())
    assert np.array_equal(d, ref["log_duration_predictions"].numpy()) and a == 1.0


def test_oracle_fed_its_own_predictions_changes_nothing(oracle_ctx):
    base = _run_oracle(oracle_ctx)
    fed = _run_oracle(oracle_ctx, pitch=base["pitch_predictions"].numpy(), energy=base["energy_predictions"].numpy(),
                      durations=base["log_duration_predictions"].numpy())
    assert fed["mel_len"] == base["mel_len"] and torch.equal(fed["dec_outputs"], base["dec_outputs"])
    # ... while an edited track does change the mel
    shifted = _run_oracle(oracle_ctx, pitch=base["pitch_predictions"].numpy() + 0.5)
    assert not torch.equal(shifted["dec_outputs"], base["dec_outputs"])


# --------------------------------------------------------------------------- packing and validation

def test_pack_fills_defaults_and_packs_like_ling():
    pk = pack_prosody([Prosody(speed=2.0, pitch=[1.0, np.nan, 3.0], pitch_shift=0.25), None], [3, 2], alpha=1.3)
    st = pk.struct
    assert st.struct_size == C.sizeof(_ffi.ev_prosody) and st.reserved0 == 0
    alpha = np.ctypeslib.as_array(C.cast(st.alpha, C.POINTER(C.c_float)), (2,))
    assert alpha.tolist() == [0.5, np.float32(1.3)]                # speed -> 1 / speed; no speed -> the call's alpha
    shift = np.ctypeslib.as_array(C.cast(st.pitch_shift, C.POINTER(C.c_float)), (2,))
    assert shift.tolist() == [0.25, 0.0]
    pitch = np.ctypeslib.as_array(C.cast(st.pitch, C.POINTER(C.c_float)), (5,))
    assert pitch[0] == 1.0 and pitch[2] == 3.0 and np.isnan(pitch[[1, 3, 4]]).all()      # utterance 1 gave none: all predicted
    assert st.energy is None and st.durations is None                                     # nobody gave them: NULL
    # no speed anywhere: alpha stays NULL (the call's scalar); a single Prosody applies to every utterance
    pk = pack_prosody(Prosody(pitch_scale=1.5), [4, 7])
    assert pk.struct.alpha is None
    assert np.ctypeslib.as_array(C.cast(pk.struct.pitch_scale, C.POINTER(C.c_float)), (2,)).tolist() == [1.5, 1.5]
    d = pack_prosody([Prosody(durations=[0, -1, 12]), Prosody()], [3, 1]).struct.durations
    assert np.ctypeslib.as_array(C.cast(d, C.POINTER(C.c_int64)), (4,)).tolist() == [0, -1, 12, -1]


@pytest.mark.parametrize("bad, match", [
    (dict(pitch=[1.0, 2.0]), r"prosody\[0\]\.pitch: expected 3 values"),
    (dict(energy=np.zeros((3, 1))), r"prosody\[0\]\.energy: expected 3 values"),
    (dict(durations=[1, 2, 3, 4]), r"prosody\[0\]\.durations: expected 3 values"),
    (dict(pitch=[0.0, np.inf, 0.0]), r"pitch: infinite"),
    (dict(energy=[0.0, 0.0, -np.inf]), r"energy: infinite"),
    (dict(pitch=[0.0, 1e39, 0.0]), r"pitch: infinite"),
    (dict(pitch_scale=np.nan), r"pitch_scale"),
    (dict(pitch_shift=np.inf), r"pitch_shift"),
    (dict(energy_scale=1e40), r"energy_scale"),
    (dict(energy_shift=-np.inf), r"energy_shift"),
    (dict(durations=[0, -2, 1]), r"durations: values must lie in \[-1, 1024\]"),
    (dict(durations=[0, MAX_DURATION + 1, 1]), r"durations: values must lie"),
    (dict(durations=[0.5, 1, 1]), r"whole numbers"),
    (dict(speed=0.0), r"speed"),
    (dict(speed=-1.0), r"speed"),
    (dict(speed=np.inf), r"speed"),
    (dict(alpha=np.nan), r"alpha"),
    (dict(alpha=1e-50), r"duration scale"),
    (dict(speed=1.0, alpha=1.0), r"not both"),
])
def test_pack_rejects_bad_controls(bad, match):
    with pytest.raises(ValueError, match=match):
        pack_prosody([Prosody(**bad), None], [3, 2])


def test_pack_rejects_count_mismatch_call_alpha_and_forced_durations():
    with pytest.raises(ValueError, match="3 prosody entries for 2 utterances"):
        pack_prosody([None, None, None], [3, 2])
    with pytest.raises(ValueError, match="alpha"):
        pack_prosody([None], [3], alpha=0.0)
    with pytest.raises(ValueError, match="forced durations"):
        pack_prosody([Prosody()], [3], forced=True)
    with pytest.raises(ValueError, match="not a Prosody"):
        pack_prosody([dict(speed=2.0)], [3])
    # host validation accepts the boundaries: NaN (predicted), -1 (predicted), 0 and the cap
    pack_prosody([Prosody(pitch=[np.nan, 0.0, -3.0], durations=[-1, 0, MAX_DURATION])], [3])


# --------------------------------------------------------------------------- C ABI surface

def _header():
    return open(os.path.join(ROOT, "include", "evhip.h")).read()


def test_ev_synthesize_prosody_is_declared_exported_and_bound():
    assert "ev_synthesize_prosody" in _ffi.SIGNATURES
    assert "int ev_synthesize_prosody(" in _header()
    assert hasattr(_ffi.lib(), "ev_synthesize_prosody")
    assert "EV_PROSODY_MAX_DURATION %d " % _ffi.EV_PROSODY_MAX_DURATION in _header()


def test_ev_prosody_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not installed")
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evhip.h"\n'
                   'int main(){printf("%zu %zu %zu %zu\\n", sizeof(ev_prosody), offsetof(ev_prosody, alpha), offsetof(ev_prosody, pitch), '
                   'offsetof(ev_prosody, durations));return 0;}')
    exe = tmp_path / "p"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = _ffi.ev_prosody
    assert got == [C.sizeof(P), P.alpha.offset, P.pitch.offset, P.durations.offset]


# --------------------------------------------------------------------------- serving: opt-in mixed-prosody batching

def _fake_prosody_synth(log):
    def fn(utts, prosodies):
        log.append([(p.duration_scale(), p.pitch_shift, p.energy_scale) for p in prosodies])
        return [np.full(int(256 * len(u["ling"]) * p.duration_scale()), float(u["speaker"]) + p.pitch_shift, np.float32)
                for u, p in zip(utts, prosodies)]
    return fn


def test_mixed_prosody_batcher_forms_one_batch_and_routes_controls():
    log = []
    b = DynamicBatcher(_fake_prosody_synth(log), max_batch=16, max_wait_ms=300, mixed_prosody=True)
    alphas = [1.0, 2.0, 0.5, 1.25, 2.0, 0.8]
    futs = []
    for i, a in enumerate(alphas):
        pr = Prosody(pitch_shift=0.1 * i, energy_scale=1.0 + i) if i % 2 else None
        futs.append(b.submit(np.arange(4 + i), speaker=i, style=np.zeros(768), content=np.zeros(768), alpha=a, prosody=pr))
    # a Prosody with a speed of its own wins over the request's alpha
    futs.append(b.submit(np.arange(4), speaker=9, style=np.zeros(768), content=np.zeros(768), alpha=3.0, prosody=Prosody(speed=2.0)))
    outs = [f.result(timeout=10) for f in futs]
    b.close()
    assert b.batches == [7] and len(log) == 1                      # mixed speeds: ONE batch
    for i, a in enumerate(alphas):
        shift = 0.1 * i if i % 2 else 0.0
        assert outs[i].shape == (int(256 * (4 + i) * a),) and np.allclose(outs[i], i + shift)     # each client: its own audio and controls
        assert log[0][i] == (a, shift, 1.0 + i if i % 2 else 1.0)
    assert outs[6].shape == (int(256 * 4 * 0.5),) and log[0][6][0] == 0.5


def test_default_batcher_still_groups_by_alpha_and_refuses_prosody():
    calls = []

    def fn(utts, alpha):
        calls.append((len(utts), alpha))
        return [np.zeros(4, np.float32) for _ in utts]

    b = DynamicBatcher(fn, max_batch=16, max_wait_ms=300)
    with pytest.raises(ValueError, match="mixed_prosody"):
        b.submit(np.arange(3), 1, np.zeros(768), np.zeros(768), prosody=Prosody(pitch_shift=1.0))
    futs = [b.submit(np.arange(3), i, np.zeros(768), np.zeros(768), alpha=a) for i, a in enumerate([1.0, 2.0, 1.0, 2.0, 1.0])]
    [f.result(timeout=10) for f in futs]
    b.close()
    assert len(calls) >= 2 and sum(n for n, _ in calls) == 5
    assert {a for _, a in calls} == {1.0, 2.0}


def test_mixed_batcher_validates_each_request_on_its_own():
    b = DynamicBatcher(_fake_prosody_synth([]), mixed_prosody=True)
    with pytest.raises(ValueError, match="pitch: expected 3 values"):
        b.submit(np.arange(3), 1, np.zeros(768), np.zeros(768), prosody=Prosody(pitch=[0.0]))
    b.close()


def test_tts_service_prosody_fields():
    log = []
    g2p = lambda text: " ".join(text)                              # noqa: E731  one "phoneme" per character
    token2id = {ch: i for i, ch in enumerate("abcdefgh")}
    embed = lambda text: np.zeros(768, np.float32)                 # noqa: E731
    mixed = DynamicBatcher(_fake_prosody_synth(log), max_wait_ms=1, mixed_prosody=True)
    svc = TTSService(mixed, token2id, {"v": 7}, g2p, embed)
    w = svc.submit("abcd", "v", speed=2.0, pitch_shift=0.5, pitch_scale=1.2, energy_scale=0.7).result(timeout=10)
    assert w.shape == (int(256 * 4 * 0.5),) and np.allclose(w, 7.5)
    assert log[-1] == [(0.5, 0.5, np.float64(0.7))]
    mixed.close()
    plain_calls = []

    def fn(utts, alpha):
        plain_calls.append(alpha)
        return [np.zeros(8, np.float32) for _ in utts]

    plain = DynamicBatcher(fn, max_wait_ms=1)
    svc = TTSService(plain, token2id, {"v": 7}, g2p, embed)
    assert svc.submit("ab", "v", speed=2.0).result(timeout=10).shape == (8,)     # identity controls: today's call
    assert plain_calls == [0.5]
    with pytest.raises(ValueError, match="mixed_prosody"):
        svc.submit("ab", "v", pitch_shift=0.5)
    plain.close()
