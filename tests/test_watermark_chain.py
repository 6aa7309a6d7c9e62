"""The watermark stage of the output chain (emotivoice_amd/output_chain.py) against the stand-in library: where it runs, what it reads and what the
later stages receive, who makes the int16, what is copied to the host, what FLAC reads, the checks before any library call, the long form, the
serving factories and the command-line flag."""
import numpy as np
import pytest

import fake_evhip as fk
import fake_evhip_stretch as fks
import fake_evhip_watermark as fkw
from emotivoice_amd import _ffi
from emotivoice_amd.denoise import DenoiseConfig
from emotivoice_amd.watermark import WatermarkConfig

DEV = _ffi.EV_FLAG_DEVICE_INPUTS
TOKENS = (3, 5, 2)
LENS = [t * fk.UP for t in TOKENS]                 # 768, 1280, 512
NEW = [614, 1600, 512]                             # after stretch=[1.25, 0.8, None]
MARKED = [512, 1536, 512]                          # ... cut to whole hops by the mark
N = int(np.sum(LENS))
BIAS = np.ones(513, np.float32)


def utterances():
    return [dict(ling=np.arange(t) + 1, speaker=b, style=np.zeros(768, np.float32), content=np.zeros(768, np.float32)) for b, t in enumerate(TOKENS)]


@pytest.fixture
def eng(monkeypatch):
    lib = fkw.WatermarkLib()
    monkeypatch.setattr(_ffi, "lib", lambda: lib)
    from emotivoice_amd.engine import EVEngine
    e = EVEngine()
    e.fake = lib
    yield e
    e.close()


def test_the_mark_runs_third_and_the_later_stages_read_it(eng):
    lib = eng.fake
    wc = WatermarkConfig(key=0xC0FFEE, payload=[1, 2, 3], nbits=[2, 2, 2], strength_db=[0.5, 1.0, 2.0])
    out = eng.synthesize(utterances(), denoise=DenoiseConfig(bias=BIAS), stretch=[1.25, 0.8, None], watermark=wc, loudness=-16.0, limiter=-1.0,
                         want_int16=True, flac=True)
    assert lib.names() == ["ev_synthesize", "ev_denoise_setup", "ev_denoise", "ev_stretch", "ev_watermark", "ev_loudness", "ev_limit", "ev_flac"]
    (wm,), (ld,), (lim,), (fl,) = (lib.calls("ev_" + k) for k in ("watermark", "loudness", "limit", "flac"))
    assert (wm["B"], wm["flags"], wm["lens"], wm["is_i16"], wm["src"]) == (3, DEV, NEW, 0, ("stretch.wav", 0))
    assert (wm["payloads"], wm["nbits"], wm["strengths_db"]) == ([1, 2, 3], [2, 2, 2], [0.5, 1.0, 2.0])
    assert wm["cfg"]["key"] == 0xC0FFEE and wm["cfg"]["want_i16"] == 0 and lib.calls("ev_stretch")[0]["cfg"] == dict(want_int16=0)      # not the last stage
    assert ld["src"] == lim["src"] == ("watermark.wav", 0) and ld["lens"] == lim["lens"] == MARKED and lim["cfg"]["want_i16"] == 1
    assert fl["src"] == ("limit.wav_i16", 0) and fl["lens"] == MARKED
    assert sorted(e["src"][0] for e in lib.calls("ev_memcpy_d2h")) == ["flac1.bytes", "limit.wav", "limit.wav_i16"]      # only the last stage's audio
    assert [w.size for w in out["wav_list"]] == MARKED == [w.size for w in out["wav_int16_list"]]
    fig = out["watermark"]
    assert fig["lens_out"].tolist() == MARKED and fig["offsets"].tolist() == [0, 512, 2048, 2560] and fig["key"] == 0xC0FFEE
    assert fig["payload"].tolist() == [1, 2, 3] and fig["nbits"].tolist() == [2, 2, 2] and fig["strength_db"].tolist() == [0.5, 1.0, 2.0]
    assert not any(k in fig for k in ("wav", "wav_list", "wav_i16")) and out["stretch"]["lens_out"].tolist() == NEW


def test_the_mark_alone_is_the_last_stage_and_flac_reads_its_int16(eng):
    lib = eng.fake
    out = eng.synthesize(utterances(), watermark=7, flac=[True, False, True])
    assert lib.names() == ["ev_synthesize", "ev_watermark", "ev_flac", "ev_flac"]
    (wm,) = lib.calls("ev_watermark")
    assert wm["src"] == ("synth.wav", 0) and wm["cfg"]["want_i16"] == 1 and wm["cfg"]["key"] == 7      # FLAC will read it
    assert (wm["payloads"], wm["nbits"], wm["strengths_db"]) == ([0, 0, 0], [0, 0, 0], [1.0, 1.0, 1.0])
    assert lib.calls("ev_synthesize")[0]["flags"] & _ffi.EV_FLAG_WANT_INT16 == 0      # the source makes no int16 of its own
    want = fkw.marked(fk.ramp(N), LENS)
    assert np.array_equal(out["wav"], want) and [w.size for w in out["wav_list"]] == LENS
    assert [(e["src"], e["lens"]) for e in lib.calls("ev_flac")] == [(("watermark.wav_i16", 0), [768]), (("watermark.wav_i16", 2 * 2048), [512])]
    assert out["flac_list"][1] is None and out["flac_list"][2] == b"fLaC" + fk.to_i16(want)[2048:].tobytes()[:8]
    out = eng.synthesize(utterances(), watermark="7:5:3", want_int16=True)
    assert lib.calls("ev_watermark")[-1]["cfg"]["want_i16"] == 1 and lib.calls("ev_watermark")[-1]["payloads"] == [5, 5, 5]
    assert lib.calls("ev_watermark")[-1]["nbits"] == [3, 3, 3] and [w.size for w in out["wav_int16_list"]] == LENS
    out = eng.synthesize(utterances(), watermark=dict(key=9, strength_db=0.5), delivery=8000)
    assert lib.calls("ev_deliver")[-1]["src"] == ("watermark.wav", 0) and lib.calls("ev_deliver")[-1]["lens"] == LENS
    assert lib.calls("ev_watermark")[-1]["cfg"]["want_i16"] == 0 and "wav" not in out and [d.size for d in out["delivered_list"]] == [384, 640, 256]


def test_the_checks_come_before_any_library_call(eng):
    lib = eng.fake
    with pytest.raises(ValueError, match="^watermark needs the vocoder's waveform$"):
        eng.synthesize(utterances(), watermark=7, vocoder=False)
    for bad, text in ((WatermarkConfig(key=1, nbits=[1, 1]), "one entry per segment \\(3\\), got 2"), (WatermarkConfig(key=1, nbits=17), "nbits\\[0\\] = 17"),
                      (WatermarkConfig(key=1, nbits=2, payload=4), "does not fit 2 bits"), (WatermarkConfig(key=1, strength_db=9.0), "outside \\[0, 6\\]"),
                      (1.5, "watermark: None, a key"), ("1:2", "KEY or KEY:PAYLOAD:NBITS"), (-1, "not an integer in")):
        with pytest.raises(ValueError, match=text):
            eng.synthesize(utterances(), watermark=bad)
    with pytest.raises(ValueError, match="one entry per segment \\(2\\), got 3"):
        eng.synthesize_long([dict(utts=utterances()[:2]), (utterances()[2:], None)], watermark=WatermarkConfig(key=1, nbits=[0, 0, 0]))
    assert lib.names() == []


def test_without_watermark_the_transcript_is_the_one_of_the_library_without_it(monkeypatch):
    """watermark=None, the default, issues exactly the calls it issued before: the stand-in WITHOUT ev_watermark (it would raise on any call of
    it) logs the same entries with the same arguments."""
    logs = []
    for lib in (fks.StretchLib(), fkw.WatermarkLib()):
        monkeypatch.setattr(_ffi, "lib", lambda lib=lib: lib)
        from emotivoice_amd.engine import EVEngine
        e = EVEngine()
        e.synthesize(utterances(), denoise=DenoiseConfig(bias=BIAS), stretch=1.25, loudness=-16.0, limiter=-1.0, want_int16=True, flac=True)
        e.synthesize(utterances(), watermark=None, delivery=8000, flac=[True, False, True])
        e.synthesize_long([dict(utts=utterances())], flac=True, watermark=None)
        logs.append([repr(x) for x in lib.log])
        e.close()
    assert logs[0] == logs[1] and not any("watermark" in x for x in logs[1])
    for cls in (fk.FakeLib, fk.DenoiseLib, fk.DeliverLib, fks.StretchLib):
        assert not hasattr(cls(), "ev_watermark") and not hasattr(cls(), "ev_watermark_detect")      # the existing stand-ins keep raising


def test_synthesize_long_marks_per_document_after_the_stretch(eng):
    lib = eng.fake
    u = utterances()
    n = len(lib.log)
    out = eng.synthesize_long([dict(utts=u[:2]), (u[2:], None)], stretch=[2.0, None], watermark=WatermarkConfig(key=3, payload=[1, 0], nbits=[1, 0]),
                              limiter=-1.0)
    assert [e["name"] for e in lib.log[n:] if e["name"] != "ev_memcpy_d2h"] == ["ev_synthesize", "ev_stitch", "ev_stretch", "ev_watermark", "ev_limit"]
    (wm,) = lib.calls("ev_watermark")
    assert wm["src"] == ("stretch.wav", 0) and wm["lens"] == [1024, 512] and wm["payloads"] == [1, 0] and wm["nbits"] == [1, 0]
    assert lib.calls("ev_limit")[0]["src"] == ("watermark.wav", 0) and lib.calls("ev_limit")[0]["lens"] == [1024, 512]
    assert out["doc_lens"].tolist() == [1024, 512] and out["doc_offsets"].tolist() == [0, 1024, 1536] and [d.size for d in out["documents"]] == [1024, 512]
    out = eng.synthesize_long([dict(utts=u)], watermark=5)
    assert lib.calls("ev_watermark")[-1]["src"] == ("stitch.wav", 0) and np.array_equal(out["documents"][0], out["docs"][0])


def test_the_serving_factories_and_the_flag_take_the_mark(eng):
    from emotivoice_amd.inference_tts import build_parser, chain_from_args
    from emotivoice_amd.serving import engine_flac_synth_fn, engine_synth_fn
    lib = eng.fake
    wavs = engine_synth_fn(eng, watermark="11:2:4")(utterances(), 1.0)
    (wm,) = lib.calls("ev_watermark")
    assert wm["cfg"]["key"] == 11 and wm["payloads"] == [2, 2, 2] and wm["nbits"] == [4, 4, 4] and [w.size for w in wavs] == LENS
    got = engine_flac_synth_fn(eng, watermark=11)(utterances(), 1.0, [True, False, False])
    assert lib.calls("ev_flac")[-1]["src"] == ("watermark.wav_i16", 0) and isinstance(got[0], bytes) and got[1].size == 1280
    with pytest.raises(ValueError):
        engine_synth_fn(eng, watermark="x")
    n = len(lib.log)
    engine_synth_fn(eng)(utterances(), 1.0)
    assert [e["name"] for e in lib.log[n:] if e["name"] != "ev_memcpy_d2h"] == ["ev_synthesize"]
    parser = build_parser()
    wc = chain_from_args(parser.parse_args(["-t", "lines.txt", "--watermark", "0x2A:3:8"]))["watermark"]
    assert (wc.key, wc.payload, wc.nbits) == (42, 3, 8) and "watermark" not in chain_from_args(parser.parse_args(["-t", "lines.txt"]))
