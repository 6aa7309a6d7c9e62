"""The delivery stage in the output chain of EVEngine.synthesize / synthesize_long and in the serving shell, on the CPU, against the stand-in
library of tests/fake_evhip.py with a trivial ev_deliver added: it NEGATES and keeps every second sample, so its output cannot be mistaken
for another stage's.  Which entries are called, in which order and with what; where ev_flac reads; what travels through the batcher."""
import ctypes as C

import numpy as np
import pytest

import fake_evhip as fk
from emotivoice_amd import _ffi
from emotivoice_amd.delivery import DeliveryConfig, wav_container

DEV = _ffi.EV_FLAG_DEVICE_INPUTS
TOKENS = (3, 5, 2)
LENS = [t * fk.UP for t in TOKENS]
OFFS = np.concatenate([[0], np.cumsum(LENS)])
N = int(OFFS[-1])


encode, DeliverLib = fk.encode, fk.DeliverLib


def utterances():
    return [dict(ling=np.arange(t) + 1, speaker=b, style=np.zeros(768, np.float32), content=np.zeros(768, np.float32)) for b, t in enumerate(TOKENS)]


def engine(monkeypatch, lib):
    monkeypatch.setattr(_ffi, "lib", lambda: lib)
    from emotivoice_amd.engine import EVEngine
    e = EVEngine()
    e.fake = lib
    return e


@pytest.fixture
def eng(monkeypatch):
    e = engine(monkeypatch, DeliverLib())
    yield e
    e.close()


def limited(x, lens):
    """What the stand-in's measure + limit makes of x (tests/test_engine_chain.py: gains_for, staged)."""
    from emotivoice_amd.limiter import pre_gain
    from emotivoice_amd.loudness import LoudnessConfig
    g = np.array([pre_gain(fk.LOUDNESS(b), LoudnessConfig(target_lufs=-16.0))[0] for b in range(len(lens))], np.float32)
    return x * np.repeat(g * np.float32(3.0), lens)


def test_synthesize_runs_deliver_after_the_limiter_and_flac_after_deliver(eng):
    lib = eng.fake
    out = eng.synthesize(utterances(), loudness=-16.0, limiter=-1.0, flac=True, delivery=DeliveryConfig(8000, "s16", seed=9))
    assert lib.names() == ["ev_synthesize", "ev_loudness", "ev_limit", "ev_deliver_setup", "ev_deliver", "ev_flac", "ev_flac", "ev_flac"]
    (st,) = lib.calls("ev_deliver_setup")
    assert st["cfg"] == dict(sr_in=16000, sr_out=8000, encoding=_ffi.EV_DELIVER_S16, dither=0, seed=9, half_len=0, taps=None)
    (lim,), (dl,) = lib.calls("ev_limit"), lib.calls("ev_deliver")
    assert lim["cfg"]["want_i16"] == 0      # the earlier stages make no int16 for a delivered response
    # the limiter's device fp32 waveform, not a host copy
    assert (dl["B"], dl["flags"], dl["lens"], dl["is_i16"], dl["src"], dl["seeds"]) == (3, DEV, LENS, 0, ("limit.wav", 0), None)
    y = limited(fk.ramp(N), LENS)
    want = [fk.to_i16(-y[a:b:2]) for a, b in zip(OFFS[:-1], OFFS[1:])]
    offs = np.concatenate([[0], np.cumsum([(2 * w.size + 15) // 16 * 16 for w in want])])
    assert out["delivered_rate"] == 8000 and all(g.dtype == np.int16 and np.array_equal(g, w) for g, w in zip(out["delivered_list"], want))
    assert out["delivery"]["clipped"].tolist() == [0, 1, 2] and out["delivery"]["peak"].tolist() == [0.25] * 3 and out["delivery"]["n_samples"].tolist() == [w.size for w in want]
    # ev_flac: one call per utterance, on deliver's int16, at the delivered rate
    for b, e in enumerate(lib.calls("ev_flac")):
        assert (e["B"], e["flags"], e["lens"], e["is_i16"], e["src"]) == (1, DEV, [want[b].size], 1, ("deliver.data", int(offs[b])))
        assert e["cfg"]["sample_rate"] == 8000
    assert out["flac_list"] == [b"fLaC" + w.tobytes()[:8] for w in want]
    # nothing of the 16 kHz waveform was copied to the host
    assert [e["src"][0] for e in lib.calls("ev_memcpy_d2h")] == ["deliver.data", "flac1.bytes", "flac2.bytes", "flac3.bytes"]
    assert "wav" not in out and "wav_list" not in out and "wav_i16" not in out and "loudness" in out and "limiter" in out


@pytest.mark.parametrize("loudness,limiter,src", ((None, None, "synth.wav"), (-16.0, None, "loudness.wav"), (None, -1.0, "limit.wav")))
def test_deliver_reads_the_last_stage(eng, loudness, limiter, src):
    out = eng.synthesize(utterances(), loudness=loudness, limiter=limiter, delivery=DeliveryConfig(24000, "ulaw"))
    (dl,) = eng.fake.calls("ev_deliver")
    assert dl["src"] == (src, 0) and dl["flags"] == DEV
    x = fk.ramp(N)
    y = x if src == "synth.wav" else x * np.float32(2.0) if src == "loudness.wav" else x * np.float32(3.0)
    assert all(np.array_equal(g, encode(-y[a:b:2], 2)) and g.dtype == np.uint8 for g, a, b in zip(out["delivered_list"], OFFS[:-1], OFFS[1:]))
    eng.synthesize(utterances(), loudness=loudness, limiter=limiter, delivery=DeliveryConfig(24000, "ulaw"))
    assert len(eng.fake.calls("ev_deliver_setup")) == 1 and len(eng.fake.calls("ev_deliver")) == 2      # the same config: one setup
    eng.synthesize(utterances(), delivery=8000)
    assert eng.fake.calls("ev_deliver_setup")[-1]["cfg"]["sr_out"] == 8000 and eng.fake.calls("ev_deliver_setup")[-1]["cfg"]["encoding"] == 1


def test_synthesize_long_goes_through_it(eng):
    from emotivoice_amd.longform import StitchConfig
    lib = eng.fake
    u = utterances()
    docs = [dict(utts=u[:2]), (u[2:], None)]
    out = eng.synthesize_long(docs, config=StitchConfig(want_int16=True), limiter=-1.0, flac=True, delivery=DeliveryConfig(48000, "s16", dither=True))
    assert lib.names() == ["ev_synthesize", "ev_stitch", "ev_limit", "ev_deliver_setup", "ev_deliver", "ev_flac", "ev_flac"]
    assert lib.calls("ev_stitch")[0]["cfg"]["want_i16"] == 0 and lib.calls("ev_limit")[0]["cfg"]["want_i16"] == 0
    (dl,) = lib.calls("ev_deliver")
    assert (dl["B"], dl["flags"], dl["lens"], dl["src"]) == (2, DEV, [2048, 512], ("limit.wav", 0))
    assert lib.calls("ev_deliver_setup")[0]["cfg"]["dither"] == 1
    y = -fk.ramp(N) * np.float32(3.0)
    want = [fk.to_i16(-y[0:2048:2]), fk.to_i16(-y[2048:2560:2])]
    assert out["documents"] is out["delivered_list"] and all(np.array_equal(g, w) for g, w in zip(out["documents"], want))
    assert out["delivered_rate"] == 48000 and out["sample_rate"] == 16000
    assert out["sentence_times"] == [[(0.0, 768 / 16000.0), (768 / 16000.0, 2048 / 16000.0)], [(0.0, 512 / 16000.0)]]      # seconds: they hold at any rate
    assert [e["cfg"]["sample_rate"] for e in lib.calls("ev_flac")] == [48000, 48000] and [e["src"] for e in lib.calls("ev_flac")] == [("deliver.data", 0), ("deliver.data", 2048)]
    assert out["flac_list"] == [b"fLaC" + w.tobytes()[:8] for w in want]
    assert "docs" not in out and "docs_i16" not in out


def test_flac_with_a_law_encoding_raises_before_any_call(eng):
    from emotivoice_amd.serving import engine_flac_synth_fn
    u = utterances()
    for enc in ("ulaw", "alaw", "f32"):
        with pytest.raises(ValueError, match="s16"):
            eng.synthesize(u, flac=True, delivery=DeliveryConfig(8000, enc))
        with pytest.raises(ValueError, match="s16"):
            eng.synthesize_long([dict(utts=u)], flac=True, delivery=DeliveryConfig(8000, enc))
        with pytest.raises(ValueError, match="s16"):
            engine_flac_synth_fn(eng, delivery=DeliveryConfig(8000, enc))
    for bad in ("8000", 8000.0, True, DeliveryConfig(16001), DeliveryConfig(8000, "f32", dither=True)):
        with pytest.raises(ValueError):
            eng.synthesize(u, delivery=bad)
    with pytest.raises(ValueError, match="vocoder"):
        eng.synthesize(u, delivery=8000, vocoder=False)
    assert eng.fake.log == []


def _strip(log):
    """A transcript as text: the entries and their arguments (a measure-only ev_loudness carries a NaN target, which equals itself only as text)."""
    return [repr(e) for e in log]


@pytest.mark.parametrize("kw", (dict(), dict(want_int16=True, flac=[True, False, True]), dict(loudness=-16.0, limiter=-1.0, flac=True), dict(limiter=-1.0, want_int16=True)))
def test_without_delivery_the_transcript_is_the_one_of_the_plain_library(monkeypatch, kw):
    """delivery=None, the default, issues exactly the calls it issued before: the stand-in WITHOUT ev_deliver (it would raise on any call of
    it) logs the same entries with the same arguments as the one with it, and the results agree."""
    from emotivoice_amd.longform import StitchConfig
    logs, outs = [], []
    for lib in (fk.FakeLib(), DeliverLib()):
        e = engine(monkeypatch, lib)
        outs.append(e.synthesize(utterances(), delivery=None, **kw))
        long_kw = {k: v for k, v in kw.items() if k != "want_int16"}
        long_kw["flac"] = bool(kw.get("flac"))
        outs.append(e.synthesize_long([dict(utts=utterances())], config=StitchConfig(want_int16=bool(kw.get("want_int16"))), delivery=None, **long_kw))
        logs.append(_strip(lib.log))
        e.close()
    assert logs[0] == logs[1] and not any("deliver" in e for e in logs[1])
    for a, b in ((outs[0], outs[2]), (outs[1], outs[3])):
        assert sorted(a) == sorted(b) and "delivered_list" not in a
        assert np.array_equal(a.get("wav", a.get("wav_i16")), b.get("wav", b.get("wav_i16")))


def _service(batcher):
    from emotivoice_amd.serving import TTSService
    return TTSService(batcher, {"a": 1, "b": 2}, {"v": 0}, g2p=lambda t: "a b a", embed=lambda t: np.zeros(768, np.float32))


def test_serving_delivers_bytes(eng):
    from emotivoice_amd.serving import DynamicBatcher, encode_audio, engine_flac_synth_fn, engine_synth_fn
    dc = DeliveryConfig(8000, "ulaw")
    bat = DynamicBatcher(engine_synth_fn(eng, limiter=-1.0, delivery=dc), max_wait_ms=1.0, delivery=dc)
    try:
        svc = _service(bat)
        assert svc.sample_rate == 8000
        want = encode(-(fk.ramp(3 * fk.UP) * np.float32(3.0))[::2], 2).tobytes()
        got = svc.submit("x", "v").result(timeout=30)
        assert isinstance(got, bytes) and got == want
        assert svc.speech("x", "v", response_format="ulaw", timeout=30) == want
        assert svc.speech("x", "v", response_format="wav", timeout=30) == wav_container(want, 8000, "ulaw")
        for fmt in ("pcm", "alaw"):      # not this service's encoding
            with pytest.raises(ValueError):
                svc.speech("x", "v", response_format=fmt, timeout=30)
        with pytest.raises(ValueError, match="flac_synth_fn"):
            svc.speech("x", "v", response_format="flac", timeout=30)
    finally:
        assert bat.close()
    s16 = DeliveryConfig(24000)
    bat = DynamicBatcher(engine_synth_fn(eng, delivery=s16), max_wait_ms=1.0, delivery=24000, flac_synth_fn=engine_flac_synth_fn(eng, delivery=s16))
    try:
        svc = _service(bat)
        pcm = fk.to_i16(-fk.ramp(3 * fk.UP)[::2]).tobytes()
        assert svc.sample_rate == 24000 and svc.speech("x", "v", response_format="pcm", timeout=30) == pcm
        assert svc.speech("x", "v", response_format="wav", timeout=30) == wav_container(pcm, 24000, "s16")
        assert svc.speech("x", "v", response_format="flac", timeout=30) == b"fLaC" + pcm[:8]
        assert eng.fake.calls("ev_flac")[-1]["cfg"]["sample_rate"] == 24000
        with pytest.raises(ValueError, match="ulaw"):
            svc.speech("x", "v", response_format="ulaw", timeout=30)
    finally:
        assert bat.close()
    # encode_audio on its own
    assert encode_audio(b"\x01\x02", "alaw", 8000, DeliveryConfig(8000, "alaw")) == b"\x01\x02"
    assert encode_audio(b"\x01\x02", "wav", 8000, DeliveryConfig(8000, "s16")) == wav_container(b"\x01\x02", 8000, "s16")
    with pytest.raises(ValueError, match="not available"):
        encode_audio(b"\x01\x02", "mp3", 8000, DeliveryConfig(8000, "s16"))


def test_serving_without_delivery_is_as_it_was(eng):
    from emotivoice_amd.serving import DynamicBatcher, encode_audio, engine_synth_fn
    bat = DynamicBatcher(engine_synth_fn(eng), max_wait_ms=1.0)
    try:
        svc = _service(bat)
        assert bat.delivery is None and svc.sample_rate == 16000
        got = svc.submit("x", "v").result(timeout=30)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, fk.ramp(3 * fk.UP))
        for fmt in ("ulaw", "alaw"):
            with pytest.raises(ValueError, match="delivery"):
                svc.speech("x", "v", response_format=fmt, timeout=30)
            with pytest.raises(ValueError, match="delivery"):
                bat.submit([1, 2], 0, np.zeros(768), np.zeros(768), response_format=fmt)
            with pytest.raises(ValueError, match="delivery"):
                encode_audio(got, fmt, 16000)
        assert not any("deliver" in n for n in eng.fake.names())
    finally:
        assert bat.close()
    with pytest.raises(ValueError) as ei:      # the message for a format nobody offers, word for word
        encode_audio(np.zeros(4, np.float32), "mp3", 16000)
    assert str(ei.value) == "response_format 'mp3' is not available (wav, pcm, flac); mp3 needs pydub / ffmpeg"
    with pytest.raises(ValueError, match="an encoded stream cannot be re-encoded as 'pcm'"):
        encode_audio(b"fLaC", "pcm", 16000)
