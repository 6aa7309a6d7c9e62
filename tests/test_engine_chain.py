"""The output chain of EVEngine.synthesize / synthesize_long (emotivoice_amd/output_chain.py: synthesis -> [stitch] -> [denoise] -> [loudness |
limit | measure + limit] -> [deliver] -> [flac]) on the CPU, against the stand-in library of tests/fake_evhip.py: which entries are called, in
which order and with what, what is copied to the host, and which stage every returned value comes from.  This file holds the stages the plain
stand-in has -- loudness, limiter and FLAC; tests/test_denoise.py and tests/test_deliver_chain.py hold the first and the last but one, and
tests/test_chain_transcripts.py the cross product of all five.  The expectations are the behaviour of the code before the chain was first
unified; the two tests whose names end in ``new_check`` assert argument checks that were added with it (deselect them with ``-k "not new_check"``)."""
import itertools

import numpy as np
import pytest

import fake_evhip as fk
from emotivoice_amd import _ffi
from emotivoice_amd.limiter import LimiterConfig, pre_gain
from emotivoice_amd.longform import StitchConfig
from emotivoice_amd.loudness import LoudnessConfig

DEV = _ffi.EV_FLAG_DEVICE_INPUTS
TOKENS = (3, 5, 2)
LENS = [t * fk.UP for t in TOKENS]                # 768, 1280, 512 samples
OFFS = [0, 768, 2048, 2560]
N = OFFS[-1]
DOC_LENS, DOC_OFFS = [2048, 512], [0, 2048, 2560]      # documents: utterances 0-1 and utterance 2
MASK = [True, False, True]
TARGET, CEILING = -16.0, -1.0
FIGURES = dict(loudness=np.float64, rel_threshold=np.float64, gain=np.float32, peak=np.float32, flags=np.uint8, nonfinite=np.int64,
               block_offsets=np.int64, block_ms=list, block_state=list)
LIMITED = dict(true_peak_in=np.float32, sample_peak_in=np.float32, true_peak_out=np.float32, sample_peak_out=np.float32, min_gain=np.float32,
               limited=np.int64, nonfinite=np.int64)


def utterances():
    return [dict(ling=np.arange(t) + 1, speaker=b, style=np.zeros(768, np.float32), content=np.zeros(768, np.float32)) for b, t in enumerate(TOKENS)]


@pytest.fixture
def eng(monkeypatch):
    lib = fk.FakeLib()
    monkeypatch.setattr(_ffi, "lib", lambda: lib)
    from emotivoice_amd.engine import EVEngine
    e = EVEngine()
    e.fake = lib
    yield e
    e.close()


def gains_for(B):
    """The host pre-gains of measure + limit for the loudness the stand-in reports."""
    return np.array([pre_gain(fk.LOUDNESS(b), LoudnessConfig(target_lufs=TARGET))[0] for b in range(B)], np.float32)


def staged(x, lens, loudness, limiter):
    """What the stand-in's stages make of the packed fp32 ``x``: (the audio, the buffer it lies in)."""
    if limiter:
        g = gains_for(len(lens)) if loudness else np.ones(len(lens), np.float32)
        return x * np.repeat(g * np.float32(3.0), lens), "limit"
    return x * np.float32(2.0), "loudness"


def check_stages(lib, lens, src, loudness, limiter, want_i16):
    """The ev_loudness / ev_limit entries of the transcript; -> their names in order."""
    names = []
    if loudness:
        names.append("ev_loudness")
        (e,) = lib.calls("ev_loudness")
        assert (e["B"], e["flags"], e["lens"], e["is_i16"], e["src"]) == (len(lens), DEV, lens, 0, (src, 0))
        assert e["cfg"]["sample_rate"] == 16000 and e["cfg"]["want_i16"] == (0 if limiter else int(want_i16))
        assert np.isnan(e["cfg"]["target_lufs"]) if limiter else e["cfg"]["target_lufs"] == TARGET      # with a limiter: measure only
    if limiter:
        names.append("ev_limit")
        (e,) = lib.calls("ev_limit")
        assert (e["B"], e["flags"], e["lens"], e["is_i16"], e["src"]) == (len(lens), DEV, lens, 0, (src, 0))
        assert e["cfg"]["sample_rate"] == 16000 and e["cfg"]["want_i16"] == int(want_i16) and e["cfg"]["ceiling"] == LimiterConfig(ceiling_dbtp=CEILING).ceiling
        assert e["gains"] == (gains_for(len(lens)).tolist() if loudness else None)      # gains are null without a loudness target
    return names


def check_figures(out, B, loudness, limiter):
    assert ("loudness" in out) == bool(loudness) and ("limiter" in out) == bool(limiter)
    if loudness:
        fig = out["loudness"]
        assert list(fig) == list(FIGURES) and all(isinstance(fig[k], t) if t is list else fig[k].dtype == t for k, t in FIGURES.items())
        assert fig["loudness"].tolist() == [fk.LOUDNESS(b) for b in range(B)] and fig["flags"].tolist() == [0] * B
        assert np.array_equal(fig["gain"], gains_for(B) if limiter else np.full(B, 2.0, np.float32))      # with a limiter: the host pre-gain
        assert [m.tolist() for m in fig["block_ms"]] == [[0.25]] * B
    if limiter:
        lim = out["limiter"]
        assert list(lim) == list(LIMITED) and all(lim[k].dtype == t and lim[k].shape == (B,) for k, t in LIMITED.items())
        assert lim["limited"].tolist() == list(range(B)) and lim["true_peak_in"].tolist() == [np.float32(0.9)] * B


def same(list_, flat, offs):
    return len(list_) == len(offs) - 1 and all(np.array_equal(x, flat[a:b]) for x, a, b in zip(list_, offs[:-1], offs[1:]))


@pytest.mark.parametrize("loudness,limiter,want_int16,flac", list(itertools.product((None, TARGET), (None, CEILING), (False, True), (None, True, MASK))))
def test_synthesize_chain(eng, loudness, limiter, want_int16, flac):
    lib = eng.fake
    out = eng.synthesize(utterances(), want_int16=want_int16, flac=flac, loudness=loudness, limiter=limiter)
    stage = loudness is not None or limiter is not None
    want_i16 = want_int16 or flac is not None
    sel = [] if flac is None else [0, 1, 2] if flac is True else [0, 2]
    runs = [] if flac is None else [(0, 3)] if flac is True else [(0, 1), (2, 3)]

    # the transcript
    (syn,) = lib.calls("ev_synthesize")
    assert (syn["B"], syn["tokens"]) == (3, list(TOKENS))
    assert syn["flags"] == (0 if stage else _ffi.EV_FLAG_WANT_INT16 if want_int16 else 0)      # a stage makes the int16 itself
    assert lib.names() == ["ev_synthesize"] + check_stages(lib, LENS, "synth.wav", loudness, limiter, want_i16) + ["ev_flac"] * len(runs)

    # the audio and where it was copied from
    if stage:
        wav, buf = staged(fk.ramp(N), LENS, loudness, limiter)
    else:
        wav, buf = fk.ramp(N), "synth"
    copies = [((buf + ".wav", 0), 4 * N)] + ([((buf + ".wav_i16", 0), 2 * N)] if (want_i16 if stage else want_int16) else [])
    keys = ["mel_lens", "mel_offsets", "cu_seqlens", "wav", "wav_list"]
    assert out["wav"].dtype == np.float32 and np.array_equal(out["wav"], wav) and same(out["wav_list"], wav, OFFS)
    if stage and want_i16:
        keys += ["wav_i16", "wav_int16_list"]
        assert out["wav_i16"].dtype == np.int16 and np.array_equal(out["wav_i16"], fk.to_i16(wav)) and same(out["wav_int16_list"], fk.to_i16(wav), OFFS)
    elif want_int16:
        keys += ["wav_i16"]      # EV_FLAG_WANT_INT16's: no list
        assert out["wav_i16"].dtype == np.int16 and np.array_equal(out["wav_i16"], fk.to_i16(wav))
    check_figures(out, 3, loudness, limiter)
    assert out["mel_lens"].dtype == np.int32 and out["mel_lens"].tolist() == list(TOKENS)
    assert out["mel_offsets"].dtype == np.int64 and out["mel_offsets"].tolist() == [0, 3, 8, 10]
    assert out["cu_seqlens"].dtype == np.int32 and out["cu_seqlens"].tolist() == [0, 3, 8, 10]

    # ev_flac: one call per run of selected utterances, from the fp32 synthesis (wrapping) or from the last stage's int16
    pcm = fk.to_i16(wav) if stage else wav
    for e, (a, b) in zip(lib.calls("ev_flac"), runs):
        assert (e["B"], e["flags"], e["lens"], e["is_i16"]) == (b - a, DEV, LENS[a:b], int(stage)) and type(e["B"]) is int      # ctypes takes no numpy integer
        assert e["src"] == ((buf + ".wav_i16", 2 * OFFS[a]) if stage else ("synth.wav", 4 * OFFS[a]))
        assert e["cfg"] == dict(sample_rate=16000, block_size=4096, max_fixed_order=4, max_partition_order=5, convert=_ffi.EV_FLAC_WRAP)
        copies.append((("flac%d.bytes" % (runs.index((a, b)) + 1), 0), 12 * (b - a)))
    if flac is not None:
        keys.append("flac_list")
        assert out["flac_list"] == [b"fLaC" + pcm[OFFS[b]:OFFS[b + 1]].tobytes()[:8] if b in sel else None for b in range(3)]
    assert [(e["src"], e["nbytes"]) for e in lib.calls("ev_memcpy_d2h")] == copies
    assert sorted(out) == sorted(keys + (["loudness"] if loudness else []) + (["limiter"] if limiter else []))


@pytest.mark.parametrize("loudness,limiter,want_int16,flac", list(itertools.product((None, TARGET), (None, CEILING), (False, True), (None, True))))
def test_synthesize_long_chain(eng, loudness, limiter, want_int16, flac):
    lib = eng.fake
    u = utterances()
    out = eng.synthesize_long([dict(utts=u[:2]), (u[2:], None)], config=StitchConfig(want_int16=want_int16), flac=flac, loudness=loudness, limiter=limiter)
    stage = loudness is not None or limiter is not None
    want_i16 = want_int16 or bool(flac)      # flac=True turns config.want_int16 on

    (syn,) = lib.calls("ev_synthesize")
    assert (syn["B"], syn["flags"], syn["tokens"]) == (3, 0, list(TOKENS))
    (st,) = lib.calls("ev_stitch")
    assert (st["B"], st["flags"], st["src"], st["offsets"], st["lens"], st["seg_doc"]) == (3, DEV, ("synth.wav", 0), OFFS[:-1], LENS, [0, 0, 1])
    assert st["cfg"]["want_i16"] == int(want_i16)
    assert lib.names() == ["ev_synthesize", "ev_stitch"] + check_stages(lib, DOC_LENS, "stitch.wav", loudness, limiter, want_i16) + ["ev_flac"] * bool(flac)

    # one copy of the last stage's documents: int16 with want_int16, else fp32
    wav, buf = staged(-fk.ramp(N), DOC_LENS, loudness, limiter) if stage else (-fk.ramp(N), "stitch")
    keys = ["doc_lens", "doc_offsets", "seg_pos", "seg_start", "seg_end", "seg_peak", "documents", "seg_doc", "sentence_times", "sample_rate"]
    if want_i16:
        keys += ["wav_i16", "docs_i16"]
        copies = [((buf + ".wav_i16", 0), 2 * N)]
        assert out["wav_i16"].dtype == np.int16 and np.array_equal(out["wav_i16"], fk.to_i16(wav)) and same(out["docs_i16"], fk.to_i16(wav), DOC_OFFS)
        assert out["documents"] is out["docs_i16"]
    else:
        keys += ["wav", "docs"]
        copies = [((buf + ".wav", 0), 4 * N)]
        assert out["wav"].dtype == np.float32 and np.array_equal(out["wav"], wav) and same(out["docs"], wav, DOC_OFFS)
        assert out["documents"] is out["docs"]
    check_figures(out, 2, loudness, limiter)
    assert out["doc_lens"].dtype == np.int64 and out["doc_lens"].tolist() == DOC_LENS and out["doc_offsets"].tolist() == DOC_OFFS
    assert out["seg_pos"].dtype == np.int64 and out["seg_pos"].tolist() == [0, 768, 0] and out["seg_end"].tolist() == LENS
    assert out["seg_peak"].dtype == np.float32 and out["seg_doc"].tolist() == [0, 0, 1] and out["sample_rate"] == 16000
    assert out["sentence_times"] == [[(0.0, 768 / 16000.0), (768 / 16000.0, 2048 / 16000.0)], [(0.0, 512 / 16000.0)]]

    # ev_flac: one call for all documents, from the last stage's int16
    if flac:
        keys.append("flac_list")
        (e,) = lib.calls("ev_flac")
        assert (e["B"], e["flags"], e["lens"], e["is_i16"], e["src"]) == (2, DEV, DOC_LENS, 1, (buf + ".wav_i16", 0))
        assert e["cfg"] == dict(sample_rate=16000, block_size=4096, max_fixed_order=4, max_partition_order=5, convert=_ffi.EV_FLAC_WRAP)
        copies.append((("flac1.bytes", 0), 24))
        assert out["flac_list"] == [b"fLaC" + fk.to_i16(wav)[a:b].tobytes()[:8] for a, b in zip(DOC_OFFS[:-1], DOC_OFFS[1:])]
    assert [(e["src"], e["nbytes"]) for e in lib.calls("ev_memcpy_d2h")] == copies
    assert sorted(out) == sorted(keys + (["loudness"] if loudness else []) + (["limiter"] if limiter else []))


def test_prosody_takes_the_prosody_entry(eng):
    from emotivoice_amd.prosody import Prosody
    out = eng.synthesize(utterances(), prosody=Prosody(speed=1.0), loudness=TARGET)
    assert eng.fake.names() == ["ev_synthesize_prosody", "ev_loudness"] and np.array_equal(out["wav"], fk.ramp(N) * np.float32(2.0))


def test_no_vocoder_rejections(eng):
    out = eng.synthesize(utterances(), vocoder=False)
    assert eng.fake.calls("ev_synthesize")[0]["flags"] == _ffi.EV_FLAG_NO_VOCODER and "wav" not in out
    before = len(eng.fake.log)
    for kw in (dict(flac=True), dict(flac=MASK), dict(loudness=TARGET), dict(limiter=CEILING), dict(limiter=True, loudness=TARGET)):
        with pytest.raises(ValueError, match="needs the vocoder's waveform"):
            eng.synthesize(utterances(), vocoder=False, **kw)
    assert len(eng.fake.log) == before      # nothing was called


def test_invalid_stage_arguments_raise_before_any_call_new_check(eng):
    u = utterances()
    bad = (dict(limiter="loud"), dict(limiter=3.0), dict(limiter=LimiterConfig(sample_rate=48000)), dict(loudness="x"), dict(loudness=5.0),
           dict(loudness=float("nan")), dict(loudness=TARGET, limiter=False), dict(loudness=True, limiter=CEILING), dict(flac=[True, False]))
    for kw in bad:
        with pytest.raises(ValueError):
            eng.synthesize(u, **kw)
        if "flac" not in kw:
            with pytest.raises(ValueError):
                eng.synthesize_long([dict(utts=u)], **kw)
    assert eng.fake.log == []


def test_raw_calls_check_the_size_of_lens_new_check(eng):
    x = np.zeros(8, np.float32)
    for call in (eng.features_raw, eng.pitch_raw, eng.resample_raw):
        with pytest.raises(ValueError, match="entries"):
            call(2, x.ctypes.data, False, [4, 2, 2])
        call(2, x.ctypes.data, False, [4, 4])
    assert eng.fake.names() == ["stub"] * 3
    for call in (eng.flac_raw, eng.loudness_raw, eng.limit_raw):      # these had the check before
        with pytest.raises(ValueError, match="entries"):
            call(2, x.ctypes.data, False, [4, 2, 2])
