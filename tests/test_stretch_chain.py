"""The stretch stage of the output chain (emotivoice_amd/output_chain.py) against the stand-in library: where it runs, what the later stages
receive, what is copied to the host, what FLAC reads, the checks before any library call, the long form's scaled times and synthesize_fit."""
import numpy as np
import pytest

import fake_evhip as fk
import fake_evhip_stretch as fks
from emotivoice_amd import _ffi
from emotivoice_amd.denoise import DenoiseConfig
from emotivoice_amd.stretch import StretchConfig

DEV = _ffi.EV_FLAG_DEVICE_INPUTS
TOKENS = (3, 5, 2)
LENS = [t * fk.UP for t in TOKENS]                 # 768, 1280, 512
SPEEDS = [1.25, 0.8, None]
NEW = [614, 1600, 512]                             # rint(768 / 1.25) = rint(614.4), 1280 / 0.8, speed 1
N = int(np.sum(LENS))
BIAS = np.ones(513, np.float32)


def utterances():
    return [dict(ling=np.arange(t) + 1, speaker=b, style=np.zeros(768, np.float32), content=np.zeros(768, np.float32)) for b, t in enumerate(TOKENS)]


@pytest.fixture
def eng(monkeypatch):
    lib = fks.StretchLib()
    monkeypatch.setattr(_ffi, "lib", lambda: lib)
    from emotivoice_amd.engine import EVEngine
    e = EVEngine()
    e.fake = lib
    yield e
    e.close()


def test_stretch_runs_second_and_the_later_stages_receive_the_new_lengths(eng):
    lib = eng.fake
    out = eng.synthesize(utterances(), denoise=DenoiseConfig(bias=BIAS), stretch=SPEEDS, loudness=-16.0, limiter=-1.0, want_int16=True, flac=True)
    assert lib.names() == ["ev_synthesize", "ev_denoise_setup", "ev_denoise", "ev_stretch", "ev_loudness", "ev_limit", "ev_flac"]
    (st,), (ld,), (lim,), (fl,) = (lib.calls("ev_" + k) for k in ("stretch", "loudness", "limit", "flac"))
    assert (st["B"], st["flags"], st["lens"], st["lens_out"], st["is_i16"], st["src"]) == (3, DEV, LENS, NEW, 0, ("denoise.wav", 0))
    assert st["cfg"] == dict(want_int16=0) and lib.calls("ev_denoise")[0]["cfg"]["want_i16"] == 0      # not the last stage: no int16
    assert ld["src"] == lim["src"] == ("stretch.wav", 0) and ld["lens"] == lim["lens"] == NEW and lim["cfg"]["want_i16"] == 1
    assert fl["src"] == ("limit.wav_i16", 0) and fl["lens"] == NEW
    # only the last stage's audio is copied
    assert sorted(e["src"][0] for e in lib.calls("ev_memcpy_d2h")) == ["flac1.bytes", "limit.wav", "limit.wav_i16"]
    assert [w.size for w in out["wav_list"]] == NEW == [w.size for w in out["wav_int16_list"]] and out["wav"].size == sum(NEW)
    fig = out["stretch"]
    assert fig["lens_in"].tolist() == LENS and fig["lens_out"].tolist() == NEW and fig["offsets"].tolist() == [0, 614, 2214, 2726]
    assert fig["speed"].tolist() == [768 / 614, 0.8, 1.0] and fig["frames"].tolist() == [3, 7, 2] and fig["edge_frames"].tolist() == [0, 1, 2]
    assert fig["sum_dist"].tolist() == [7, 7, 7] and not any(k in fig for k in ("wav", "wav_list", "wav_i16"))
    assert out["mel_lens"].tolist() == list(TOKENS) and out["denoise"]["lens_out"].tolist() == LENS      # the model's clock stays


def test_stretch_alone_is_the_last_stage_and_flac_reads_its_int16(eng):
    lib = eng.fake
    out = eng.synthesize(utterances(), stretch=StretchConfig(samples=[700, None, 1000]), flac=[True, False, True])
    assert lib.names() == ["ev_synthesize", "ev_stretch", "ev_flac", "ev_flac"]
    (st,) = lib.calls("ev_stretch")
    new = [700, 1280, 1000]
    assert st["src"] == ("synth.wav", 0) and st["lens_out"] == new and st["cfg"] == dict(want_int16=1)      # FLAC will read it
    assert lib.calls("ev_synthesize")[0]["flags"] & _ffi.EV_FLAG_WANT_INT16 == 0      # the source makes no int16 of its own
    want = fks.stretched(fk.ramp(N), LENS, new)
    assert np.array_equal(out["wav"], want) and [w.size for w in out["wav_list"]] == new
    assert [(e["src"], e["lens"]) for e in lib.calls("ev_flac")] == [(("stretch.wav_i16", 0), [700]), (("stretch.wav_i16", 2 * 1980), [1000])]
    assert out["flac_list"][1] is None and out["flac_list"][2] == b"fLaC" + fk.to_i16(want)[1980:].tobytes()[:8]
    # want_int16 without FLAC, and a delivery that reads the stretched fp32
    out = eng.synthesize(utterances(), stretch=2.0, want_int16=True)
    assert [w.size for w in out["wav_int16_list"]] == [384, 640, 256] and lib.calls("ev_stretch")[-1]["cfg"] == dict(want_int16=1)
    out = eng.synthesize(utterances(), stretch=0.5, delivery=8000)
    assert lib.calls("ev_deliver")[-1]["src"] == ("stretch.wav", 0) and lib.calls("ev_deliver")[-1]["lens"] == [1536, 2560, 1024]
    assert lib.calls("ev_stretch")[-1]["cfg"] == dict(want_int16=0) and "wav" not in out and [d.size for d in out["delivered_list"]] == [768, 1280, 512]


def test_the_checks_come_before_any_library_call(eng):
    lib = eng.fake
    with pytest.raises(ValueError, match="^stretch needs the vocoder's waveform$"):
        eng.synthesize(utterances(), stretch=1.25, vocoder=False)
    for bad, text in (([1.25, 0.8], "one entry per segment \\(3\\), got 2"), (0.0, "not finite and > 0"), ("fast", "stretch: None, a speed"),
                      (StretchConfig(speed=2.0, samples=5), "only one of"), (StretchConfig(speed=[1.0, None, 2.0], seconds=[None, None, 1.0]), "segment 2: only one of")):
        with pytest.raises(ValueError, match=text):
            eng.synthesize(utterances(), stretch=bad)
    with pytest.raises(ValueError, match="one entry per segment \\(2\\), got 3"):
        eng.synthesize_long([dict(utts=utterances()[:2]), (utterances()[2:], None)], stretch=[1.0, 1.0, 1.0])
    assert lib.names() == []
    # what only the lengths decide is refused by the host rule, before ev_stretch is called
    with pytest.raises(ValueError, match="segment 1: 1280 -> 512 samples lies outside the ratios"):
        eng.synthesize(utterances(), stretch=[1.0, 2.5, 1.0])
    assert lib.names() == ["ev_synthesize"]


def test_without_stretch_the_transcript_is_the_one_of_the_library_without_it(monkeypatch):
    """stretch=None, the default, issues exactly the calls it issued before: the stand-in WITHOUT ev_stretch (it would raise on any call of it)
    logs the same entries with the same arguments."""
    class Before(fk.DenoiseLib, fk.DeliverLib):
        pass
    logs = []
    for lib in (Before(), fks.StretchLib()):
        monkeypatch.setattr(_ffi, "lib", lambda lib=lib: lib)
        from emotivoice_amd.engine import EVEngine
        e = EVEngine()
        e.synthesize(utterances(), denoise=DenoiseConfig(bias=BIAS), loudness=-16.0, limiter=-1.0, want_int16=True, flac=True)
        e.synthesize(utterances(), stretch=None, delivery=8000, flac=[True, False, True])
        e.synthesize_long([dict(utts=utterances())], flac=True, stretch=None)
        logs.append([repr(x) for x in lib.log])
        e.close()
    assert logs[0] == logs[1] and not any("stretch" in x for x in logs[1])


def test_synthesize_long_stretches_per_document_and_scales_the_times(eng):
    lib = eng.fake
    u = utterances()
    plain = eng.synthesize_long([dict(utts=u[:2]), (u[2:], None)])
    n = len(lib.log)
    out = eng.synthesize_long([dict(utts=u[:2]), (u[2:], None)], stretch=[2.0, None], limiter=-1.0)
    assert [e["name"] for e in lib.log[n:] if e["name"] != "ev_memcpy_d2h"] == ["ev_synthesize", "ev_stitch", "ev_stretch", "ev_limit"]
    (st,) = lib.calls("ev_stretch")
    assert st["src"] == ("stitch.wav", 0) and st["lens"] == [2048, 512] and st["lens_out"] == [1024, 512]
    assert lib.calls("ev_limit")[0]["lens"] == [1024, 512] and lib.calls("ev_limit")[0]["src"] == ("stretch.wav", 0)
    assert out["doc_lens"].tolist() == [1024, 512] and out["doc_offsets"].tolist() == [0, 1024, 1536] and [d.size for d in out["documents"]] == [1024, 512]
    # the times of a document are its times before the stretch times L_out / L_in; the positions stay on the clock before it
    assert out["sentence_times"][0] == [(a * 0.5, b * 0.5) for a, b in plain["sentence_times"][0]] == [(0.0, 0.024), (0.024, 0.064)]
    assert out["sentence_times"][1] == plain["sentence_times"][1] and out["stretch"]["speed"].tolist() == [2.0, 1.0]
    for k in ("seg_pos", "seg_start", "seg_end"):
        assert np.array_equal(out[k], plain[k])


def test_synthesize_fit_scales_the_model_and_closes_the_rest_with_the_stretch(eng):
    from emotivoice_amd.prosody import Prosody
    lib = eng.fake
    out = eng.synthesize_fit(utterances(), [0.06, 0.04, 0.064], want_int16=True)
    assert lib.names() == ["ev_synthesize", "ev_synthesize_prosody", "ev_stretch"]
    first, second = lib.calls("ev_synthesize")[0], lib.calls("ev_synthesize_prosody")[0]
    assert first["flags"] & _ffi.EV_FLAG_NO_VOCODER and not second["flags"] & _ffi.EV_FLAG_NO_VOCODER
    target = [960, 640, 1024]                          # round(seconds * 16000)
    assert lib.calls("ev_stretch")[0]["lens_out"] == target and [w.size for w in out["wav_list"]] == target == [w.size for w in out["wav_int16_list"]]
    fit = out["fit"]
    assert fit["natural_samples"].tolist() == LENS == fit["model_samples"].tolist() and fit["target_samples"].tolist() == target
    assert fit["alpha"].tolist() == [1.25, 0.5, 2.0]   # 960 / 768, 640 / 1280, 1024 / 512; the stand-in's model ignores them
    assert fit["residual_speed"].tolist() == [0.8, 2.0, 0.5]
    # the caller's prosody keeps its pitch and energy; a duration scale of its own is refused before any call
    n = len(lib.log)
    eng.synthesize_fit(utterances(), 0.05, prosody=Prosody(pitch_scale=1.1))
    assert [e["name"] for e in lib.log[n:] if e["name"] != "ev_memcpy_d2h"] == ["ev_synthesize_prosody", "ev_synthesize_prosody", "ev_stretch"]
    n = len(lib.log)
    for bad in (Prosody(speed=1.2), [None, Prosody(alpha=0.9), None]):
        with pytest.raises(ValueError, match="speed or alpha of its own"):
            eng.synthesize_fit(utterances(), 0.05, prosody=bad)
    with pytest.raises(ValueError, match="sets stretch itself"):
        eng.synthesize_fit(utterances(), 0.05, stretch=1.0)
    assert len(lib.log) == n
