"""CPU: the numpy restatement of ev_deliver (tests/deliver_oracle.py) against CPython's audioop and its own known answers, the dither's
statistics, the RIFF container of emotivoice_amd.delivery, DeliveryConfig's rejections and the binding's new names."""
import audioop
import ctypes as C
import io
import struct
import wave

import numpy as np
import pytest

import deliver_oracle as do
from emotivoice_amd import _ffi
from emotivoice_amd.delivery import DeliveryConfig, delivery_config, wav_container

CODES = np.arange(-32768, 32768).astype(np.int16)


def test_g711_equals_audioop_on_every_int16_value():
    assert do.ulaw(CODES).tobytes() == audioop.lin2ulaw(CODES.tobytes(), 2)
    assert do.alaw(CODES).tobytes() == audioop.lin2alaw(CODES.tobytes(), 2)


def test_g711_decodes_to_within_the_segments_step():
    """mu-law quantises the biased 14-bit magnitude in steps of 2^(seg + 1), i.e. 2^(seg + 3) on the int16 scale, A-law in steps of 2^(max(seg, 1)
    + 3): the decoded value (audioop places it inside the step) is less than one step from the input; the clipped top of mu-law (|s| > 32635)
    decodes to 32124, within 2^10 + 2 * 33 * 4 of it."""
    for enc, dec, name in ((do.ulaw, audioop.ulaw2lin, "ulaw"), (do.alaw, audioop.alaw2lin, "alaw")):
        b = enc(CODES)
        back = np.frombuffer(dec(b.tobytes(), 2), np.int16).astype(np.int64)
        seg = (((b ^ (0xFF if name == "ulaw" else 0x55)) >> 4) & 7).astype(np.int64)
        step = 1 << ((seg if name == "ulaw" else np.maximum(seg, 1)) + 3)
        err = np.abs(back - CODES.astype(np.int64))
        inside = np.abs(CODES.astype(np.int64)) <= 32635 if name == "ulaw" else np.ones(CODES.size, bool)
        assert (err[inside] < step[inside]).all(), (name, int((err - step)[inside].max()))
        assert (err[~inside] <= 1024 + 264).all()
        assert (np.sign(back) * np.sign(CODES) >= 0).all()      # never the wrong sign


def test_mix_known_answers():
    assert int(do.mix(0, 0)) == 0x00000000 and int(do.mix(1, 5)) == 0x820138b2 and int(do.mix(12345, 2 ** 32 + 7)) == 0xe07a7e79
    d = do.dither(3, 4096)
    assert d.dtype == np.float32 and (np.abs(d) < 1.0).all() and np.array_equal(d.astype(np.float64) * 2.0 ** 24, np.rint(d.astype(np.float64) * 2.0 ** 24))


@pytest.mark.parametrize("seed", (0, 1, 2, 12345, 0xFFFFFFFF))
@pytest.mark.parametrize("lsb", (0.0, 0.25, -0.5, 0.75, -0.125))
def test_dither_statistics(lsb, seed):
    """TPDF makes the first moment exact and the total error variance 1/4 LSB^2: over 65 536 samples the mean of q lies within 6 sigma =
    6 * 0.5 / sqrt(65536) = 0.0117 LSB of the constant, and the error variance within 2 % of 0.25 for the non-integer constants."""
    y = np.full(65536, lsb / 32768.0, np.float32)
    q, clipped = do.to_s16(y, True, seed)
    q = q.astype(np.float64)
    assert not clipped.any() and abs(q.mean() - lsb) <= 6 * 0.5 / np.sqrt(65536), abs(q.mean() - lsb)
    if lsb != int(lsb):
        assert abs(((q - lsb) ** 2).mean() - 0.25) <= 0.02 * 0.25, ((q - lsb) ** 2).mean()


def test_undithered_rule_truncates_toward_zero():
    """The negative control: 0.25 LSB (and -0.75 LSB) give 0 without dither; the clamp, NaN and clipped."""
    y = np.array([0.25, -0.75, 1.5, -1.5, 40000.0, -40000.0, 32767.5, np.nan, np.inf, -np.inf], np.float32) / np.float32(32768.0)
    s, clipped = do.to_s16(y)
    assert s.tolist() == [0, 0, 1, -1, 32767, -32768, 32767, 0, 32767, -32768]
    assert clipped.tolist() == [False, False, False, False, True, True, True, False, True, True]
    assert not do.to_s16(np.full(65536, 0.25 / 32768.0, np.float32))[0].any()
    w = do.convert(y, "f32")
    assert w["clipped"] == 0 and w["peak"] == np.float32(40000.0) / np.float32(32768.0)      # the peak: finite samples only


def _parse(blob):
    assert blob[:4] == b"RIFF" and blob[8:12] == b"WAVE" and struct.unpack("<I", blob[4:8])[0] == len(blob) - 8
    at, chunks = 12, {}
    while at < len(blob):
        name, size = blob[at:at + 4], struct.unpack("<I", blob[at + 4:at + 8])[0]
        chunks[name] = blob[at + 8:at + 8 + size]
        at += 8 + size + (size & 1)
    assert at == len(blob)
    return chunks


@pytest.mark.parametrize("encoding,tag,width", (("s16", 1, 2), ("f32", 3, 4), ("alaw", 6, 1), ("ulaw", 7, 1)))
@pytest.mark.parametrize("n", (0, 7, 8))
def test_wav_container_header(encoding, tag, width, n):
    data = bytes(range(1, 1 + n * width))
    ch = _parse(wav_container(data, 8000, encoding))
    fmt = ch[b"fmt "]
    assert struct.unpack("<HHIIHH", fmt[:16]) == (tag, 1, 8000, 8000 * width, width, 8 * width)
    if tag == 1:
        assert len(fmt) == 16 and b"fact" not in ch
    else:
        assert len(fmt) == 18 and fmt[16:] == b"\0\0" and struct.unpack("<I", ch[b"fact"])[0] == n
    assert ch[b"data"] == data and list(ch) == ([b"fmt ", b"data"] if tag == 1 else [b"fmt ", b"fact", b"data"])


def test_wav_container_pcm16_reads_back_with_wave():
    x = (np.arange(-300, 301) * 100).astype(np.int16)
    with wave.open(io.BytesIO(wav_container(x.tobytes(), 24000, "s16")), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 24000, x.size)
        assert np.array_equal(np.frombuffer(w.readframes(x.size), np.int16), x)
    for bad in (dict(data=b"abc", sample_rate=8000, encoding="s16"), dict(data=b"", sample_rate=8000, encoding="mp3"), dict(data=b"", sample_rate=0, encoding="s16")):
        with pytest.raises(ValueError):
            wav_container(**bad)


def test_delivery_config_validation():
    assert delivery_config(None) is None and delivery_config(24000) == DeliveryConfig(24000, "s16")
    dc = DeliveryConfig(8000, "ulaw", dither=True, seed=0xFFFFFFFF).validate()
    assert delivery_config(dc) is dc and dc.dtype is np.uint8 and dc.sample_bytes == 1 and dc.output_len(16001, 16000) == 8001
    assert DeliveryConfig(44100, "f32").sample_bytes == 4 and DeliveryConfig(44100).output_len(160, 16000) == 441
    bad = (dict(sample_rate=0), dict(sample_rate=8000.0), dict(sample_rate=True), dict(sample_rate=16001), dict(encoding="mp3"), dict(encoding="f32", dither=True),
           dict(dither=1), dict(seed=-1), dict(seed=1 << 32), dict(taps=np.zeros(4, np.float32)), dict(taps=np.zeros((3, 3), np.float32)),
           dict(taps=np.array([0, np.nan, 0], np.float32)), dict(taps=np.zeros(32771, np.float32)))
    for kw in bad:
        with pytest.raises(ValueError):
            DeliveryConfig(**{"sample_rate": 8000, **kw}).validate()
    for x in (True, 8000.0, "8000"):
        with pytest.raises(ValueError):
            delivery_config(x)


def test_binding_has_the_new_names_and_the_abi_stays():
    assert _ffi.EV_ABI_VERSION == 7
    assert (_ffi.EV_DELIVER_F32, _ffi.EV_DELIVER_S16, _ffi.EV_DELIVER_ULAW, _ffi.EV_DELIVER_ALAW, _ffi.EV_DELIVER_TILE) == (0, 1, 2, 3, 1024)
    for name, nargs in (("ev_default_deliver_config", 1), ("ev_deliver_setup", 2), ("ev_deliver", 8)):
        assert len(_ffi.SIGNATURES[name][1]) == nargs, name
    assert [f for f, _ in _ffi.ev_deliver_config._fields_] == ["struct_size", "sr_in", "sr_out", "encoding", "dither", "seed", "half_len", "taps"]
    assert [f for f, _ in _ffi.ev_deliver_result._fields_] == ["struct_size", "batch", "total_bytes", "data", "byte_offsets", "n_samples", "peak", "clipped"]
    lib = _ffi.lib()      # the library exports them, and its default config is the documented one
    c = _ffi.ev_deliver_config()
    lib.ev_default_deliver_config(C.byref(c))
    assert (c.struct_size, c.sr_in, c.sr_out, c.encoding, c.dither, c.seed, c.half_len, c.taps) == (C.sizeof(c), 16000, 16000, 1, 0, 0, 0, None)
    sizes = (C.c_size_t * 4)()
    assert lib.ev_abi_info(sizes) == 7
