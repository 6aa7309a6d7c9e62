"""CPU checks of the FLAC path: the numpy oracle against an independent decoder, the coverage of the signal set, the conversion rule, the
host-only C entries and the serving shell's flac routing.  Nothing here needs a GPU."""
import ctypes as C
from concurrent.futures import Future

import numpy as np
import pytest

import flac_oracle as fo

from emotivoice_amd import _ffi
from emotivoice_amd.text_io import wav_float_to_int16


@pytest.fixture(scope="module")
def encoded():
    """name -> (signal, stream, info): every signal of the set encoded once with the default configuration."""
    out = {}
    for name, x in fo.signal_set().items():
        info = {}
        out[name] = (x, fo.encode(x, info=info), info)
    return out


def test_crc_routines_meet_their_published_check_values():
    assert fo.crc8(b"123456789") == 0xF4
    assert fo.crc16(b"123456789") == 0xFEE8


def test_every_signal_round_trips_through_the_independent_decoder(encoded):
    for name, (x, data, info) in encoded.items():
        di = {}
        y = fo.decode(data, di)
        assert y.dtype == np.int16 and np.array_equal(x, y), name
        assert di["frame_kind"] == info["frame_kind"].tolist() and di["frame_porder"] == info["frame_porder"].tolist(), name
        assert di["sample_rate"] == 16000 and di["block_size"] == 4096 and di["total"] == x.size, name


def test_the_coded_subframe_has_the_bits_the_chooser_counted():
    for name, x in fo.signal_set().items():
        for lo in range(0, x.size, 4096):
            blk = x[lo:lo + 4096]
            for mfo, mpo in ((4, 5), (2, 0), (0, 6)):
                ch = fo.choose(blk, mfo, mpo)
                assert fo.subframe_bits(blk, ch).size == ch["bits"], (name, lo, mfo, mpo)


def test_the_signal_set_reaches_every_subframe_kind_and_partition_order(encoded):
    kinds = {n: set(i["frame_kind"].tolist()) for n, (_, _, i) in encoded.items()}
    porders = {n: set(i["frame_porder"][i["frame_kind"] >= 8].tolist()) for n, (_, _, i) in encoded.items()}
    assert kinds["zeros"] == {0} and kinds["dc"] == {0}
    assert kinds["noise_full"] == {1} and kinds["alternation"] == {1}
    assert kinds["impulse"] == {8} and porders["impulse"] == {5}
    assert kinds["ramp"] == {10} and porders["ramp"] == {0}
    assert kinds["sine440"] == {12}
    assert kinds["noise_small"] == {8}
    assert kinds["voiced"] <= {9, 10} and porders["voiced"] <= {3, 4, 5} and len(porders["voiced"]) >= 2
    assert kinds["sine80_noise"] == {11}
    assert porders["two_levels"] == {1} and porders["four_levels"] == {2}
    assert set().union(*kinds.values()) == {0, 1, 8, 9, 10, 11, 12}
    assert set().union(*porders.values()) >= {0, 1, 2, 3, 4, 5}
    # the alternation drives the order-4 residual to 8 * 65535: 20 bits and a sign, 21 bits after the zigzag; int32 holds it
    assert int(np.abs(fo.residual(encoded["alternation"][0], 4)).max()) == 8 * 65535


def test_edge_lengths_round_trip_and_obey_the_order_and_partition_rules():
    v = fo.voiced(8192)
    for n in (1, 2, 3, 4, 5, 17, 100, 255, 256, 257, 4095, 4096, 4097, 8192):
        info = {}
        data = fo.encode(v[:n], info=info)
        assert np.array_equal(fo.decode(data), v[:n]), n
        last = info["decisions"][-1]
        m = n - (len(info["decisions"]) - 1) * 4096
        assert last["order"] <= m - 1 or last["kind"] < 8, n
        if last["kind"] >= 8:
            assert m % (1 << last["porder"]) == 0 and (m >> last["porder"]) > last["order"], n


def test_other_block_sizes_orders_and_rates_round_trip():
    v = fo.voiced(5000)
    for bs in fo.BLOCK_SIZES:
        assert np.array_equal(fo.decode(fo.encode(v, block_size=bs)), v), bs
    for mfo, mpo in ((0, 5), (4, 0), (0, 0), (4, 6)):
        info = {}
        assert np.array_equal(fo.decode(fo.encode(v, max_fixed_order=mfo, max_partition_order=mpo, info=info)), v), (mfo, mpo)
        fixed = info["frame_kind"] >= 8
        assert (info["frame_kind"][fixed] - 8 <= mfo).all() and (info["frame_porder"] <= mpo).all()
    for sr in fo.SAMPLE_RATE_CODE:
        di = {}
        fo.decode(fo.encode(v[:300], sample_rate=sr), di)
        assert di["sample_rate"] == sr


def test_frame_numbers_beyond_one_byte_round_trip():
    x = fo.voiced(300 * 256 + 7)
    info, di = {}, {}
    data = fo.encode(x, block_size=256, info=info)
    assert len(info["decisions"]) == 301 and np.array_equal(fo.decode(data, di), x)
    # the decoder reads frame numbers of up to six bytes, which the encoder never reaches in a test
    for v, nbytes in ((0x7F, 1), (0x80, 2), (0x7FF, 2), (0x800, 3), (0xFFFF, 3), (0x10000, 4), (0x1FFFFF, 4), (0x200000, 5), (0x3FFFFFF, 5),
                      (0x4000000, 6), (0x7FFFFFFF, 6)):
        enc = fo._utf8_number(v)
        assert len(enc) == nbytes and fo._read_utf8_number(fo._Bits(enc)) == (v, nbytes)


def _bits_to_bytes(bits):
    return np.packbits(np.array(bits, np.uint8)).tobytes()


def test_the_decoder_reads_what_the_encoder_never_writes():
    """A hand-made frame with coding method 1 (5-bit parameters), one Rice partition and one escape partition."""
    x = np.array([5, -3, 7, 100, -100, 0, 2, -2], np.int64)
    b = lambda v, n: fo._bits_of(v & ((1 << n) - 1), n)      # noqa: E731
    bits = [0] + b(8 + 1, 6) + [0] + b(int(x[0]), 16) + b(1, 2) + b(1, 4)      # FIXED 1, method 1, partition order 1
    r = x[1:] - x[:-1]
    u = [int(2 * v if v >= 0 else -2 * v - 1) for v in r]
    bits += b(3, 5)                                                          # partition 0: Rice parameter 3 in 5 bits, residuals 1 .. 3
    for v in u[:3]:
        bits += [0] * (v >> 3) + [1] + b(v, 3)
    bits += b(31, 5) + b(9, 5)                                               # partition 1: escape, 9-bit two's complement
    for v in r[3:]:
        bits += b(int(v), 9)
    hdr = bytes([0xFF, 0xF8, (6 << 4) | 5, 0x08, 0x00, len(x) - 1])
    hdr += bytes([fo.crc8(hdr)])
    body = hdr + _bits_to_bytes(bits)
    frame = body + fo.crc16(body).to_bytes(2, "big")
    data = fo.stream_header(len(x), 16000, 4096, len(frame), len(frame)) + frame
    assert fo.decode(data).tolist() == x.tolist()
    # and it notices damage: a flipped bit fails a CRC, a wrong STREAMINFO count fails the total
    bad = bytearray(data)
    bad[-5] ^= 0x10
    with pytest.raises(ValueError, match="CRC"):
        fo.decode(bytes(bad))
    with pytest.raises(ValueError):
        fo.decode(fo.stream_header(len(x) + 1, 16000, 4096, len(frame), len(frame)) + frame)
    with pytest.raises(ValueError, match="frame sizes"):
        fo.decode(fo.stream_header(len(x), 16000, 4096, len(frame) - 1, len(frame)) + frame)


def test_wrap_conversion_is_wav_float_to_int16():
    x = np.array([0.0, -0.0, 0.5, -0.5, 0.99999, -1.0, 1.0, 1.5, -1.5, 3.7, -3.7, 100.25, -100.25, 1e-6, -1e-6, 32767.9 / 32768, np.nan,
                  1.0 - 2.0 ** -17, -1.0 - 2.0 ** -15], np.float32)
    with np.errstate(invalid="ignore"):
        want = wav_float_to_int16(x)
    assert np.array_equal(fo.to_i16(x, 0), want)
    rng = np.random.default_rng(3)
    y = (rng.standard_normal(4000) * 1.2).astype(np.float32)
    assert np.array_equal(fo.to_i16(y, 0), wav_float_to_int16(y))
    assert np.array_equal(fo.to_i16(y, 1), np.clip(np.trunc(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16))
    assert fo.to_i16(np.array([np.inf, -np.inf, 1e30, -1e30], np.float32), 1).tolist() == [32767, -32768, 32767, -32768]
    assert fo.to_i16(np.array([np.inf, -np.inf], np.float32), 0).tolist() == [-1, 0]      # the low 16 bits of INT32_MAX / INT32_MIN


def test_flac_bound_covers_every_stream(encoded):
    lib = _ffi.lib()
    for name, (x, data, info) in encoded.items():
        bound = lib.ev_flac_bound(x.size, 4096)
        assert bound >= len(data), name
        if set(info["frame_kind"].tolist()) == {1}:      # VERBATIM everywhere: the bound is short of the stream by the unused header bytes only
            assert bound - len(data) <= 7 * len(info["frame_kind"]), name
    noise = fo.signal_set()["noise_full"][:512]      # two full VERBATIM frames of 256: the bound assumes 12 header bytes, these frames have 6
    assert lib.ev_flac_bound(noise.size, 256) == len(fo.encode(noise, block_size=256)) + 2 * 6
    for n, bs in ((0, 4096), (-1, 4096), ((1 << 30) + 1, 4096), (100, 0), (100, 4095), (100, 8192), (100, 128)):
        assert lib.ev_flac_bound(n, bs) == -1, (n, bs)
    assert lib.ev_flac_bound(1 << 30, 256) == 42 + (1 << 22) * (2 * 256 + 15)
    assert lib.ev_flac_bound(4097, 4096) == 42 + (2 * 4096 + 15) + (2 + 15)


def test_default_config_and_python_config_agree():
    from emotivoice_amd.flac import FlacConfig, write_flac
    c = _ffi.ev_flac_config()
    _ffi.lib().ev_default_flac_config(C.byref(c))
    assert (c.struct_size, c.sample_rate, c.block_size, c.max_fixed_order, c.max_partition_order, c.convert) == (C.sizeof(_ffi.ev_flac_config), 16000, 4096, 4, 5, 0)
    d = FlacConfig().validate().to_struct()
    assert bytes(d) == bytes(c)
    for kw in (dict(sample_rate=12345), dict(block_size=4000), dict(max_fixed_order=5), dict(max_partition_order=7), dict(convert="round")):
        with pytest.raises(ValueError, match=list(kw)[0]):
            FlacConfig(**kw).validate()
    with pytest.raises(ValueError):
        write_flac("/nonexistent/x.flac", np.zeros(4, np.int16))


def test_write_flac_writes_a_stream(tmp_path, encoded):
    from emotivoice_amd.flac import write_flac
    p = tmp_path / "a.flac"
    write_flac(str(p), encoded["ramp"][1])
    assert np.array_equal(fo.decode(p.read_bytes()), encoded["ramp"][0])


# ---------------------------------------------------------------------------------------------------------------- serving
def test_encode_audio_passes_flac_bytes_through_and_refuses_an_array():
    from emotivoice_amd.serving import encode_audio
    assert encode_audio(b"fLaC-and-so-on", "flac", 16000) == b"fLaC-and-so-on"
    with pytest.raises(ValueError, match="flac_synth_fn"):
        encode_audio(np.zeros(16, np.float32), "flac", 16000)


def _utt_args(n=3):
    return (np.arange(1, n + 1), 0, np.zeros(768, np.float32), np.zeros(768, np.float32))


def test_batcher_resolves_mixed_batches_and_keeps_synth_fn_for_plain_ones():
    from emotivoice_amd.serving import DynamicBatcher
    calls = []

    def synth(utts, alpha):
        calls.append(("plain", len(utts), alpha))
        return [np.full(4, len(u["ling"]), np.float32) for u in utts]

    def flac_synth(utts, alpha, mask):
        calls.append(("flac", len(utts), alpha, tuple(mask)))
        return [b"fLaC%d" % len(u["ling"]) if m else np.full(4, len(u["ling"]), np.float32) for u, m in zip(utts, mask)]

    b = DynamicBatcher(synth, max_batch=3, max_wait_ms=200.0, flac_synth_fn=flac_synth)
    try:
        futs = [b.submit(*_utt_args(2), response_format="flac"), b.submit(*_utt_args(3)), b.submit(*_utt_args(4), response_format="flac")]
        res = [f.result(timeout=30) for f in futs]
        assert res[0] == b"fLaC2" and res[2] == b"fLaC4" and isinstance(res[1], np.ndarray) and res[1].tolist() == [3.0] * 4
        assert calls == [("flac", 3, 1.0, (True, False, True))]
        futs = [b.submit(*_utt_args(n), response_format=fmt) for n, fmt in ((5, None), (6, "wav"), (7, "pcm"))]
        assert [f.result(timeout=30).tolist() for f in futs] == [[5.0] * 4, [6.0] * 4, [7.0] * 4]
        assert calls[1] == ("plain", 3, 1.0) and len(calls) == 2
    finally:
        assert b.close()
    plain = DynamicBatcher(synth, max_batch=1, max_wait_ms=1.0)
    try:
        with pytest.raises(ValueError, match="flac_synth_fn"):
            plain.submit(*_utt_args(2), response_format="flac")
        assert plain.submit(*_utt_args(2)).result(timeout=30).tolist() == [2.0] * 4
    finally:
        assert plain.close()


def test_engine_flac_synth_fn_hands_alpha_or_prosodies_and_the_mask_to_synthesize():
    from emotivoice_amd.prosody import Prosody
    from emotivoice_amd.serving import engine_flac_synth_fn
    seen = []

    class Engine:
        def synthesize(self, utts, **kw):
            seen.append(kw)
            return dict(wav_list=[np.zeros(2, np.float32)] * len(utts), flac_list=[b"fLaC" if m else None for m in kw["flac"]])

    fn = engine_flac_synth_fn(Engine())
    out = fn([{}, {}], 1.25, [True, False])
    assert out[0] == b"fLaC" and isinstance(out[1], np.ndarray) and seen[0] == dict(alpha=1.25, flac=[True, False])
    fn([{}], [Prosody()], [True])
    assert "prosody" in seen[1] and "alpha" not in seen[1]


def _service(flac):
    from emotivoice_amd.serving import DynamicBatcher, TTSService
    synth = lambda utts, alpha: [np.linspace(-0.5, 0.5, 64, dtype=np.float32) for _ in utts]      # noqa: E731

    def flac_synth(utts, alpha, mask):
        return [fo.encode(wav_float_to_int16(w)) if m else w for w, m in zip(synth(utts, alpha), mask)]

    b = DynamicBatcher(synth, max_batch=2, max_wait_ms=1.0, flac_synth_fn=flac_synth if flac else None)
    svc = TTSService(b, {"a": 1, "b": 2}, {"8051": 0}, g2p=lambda t: "a b a", embed=lambda t: np.zeros(768, np.float32))
    return b, svc


def test_service_speech_returns_the_stream_and_the_endpoint_answers_audio_flac():
    b, svc = _service(True)
    try:
        data = svc.speech("hello", "8051", response_format="flac", timeout=30)
        assert np.array_equal(fo.decode(data), wav_float_to_int16(np.linspace(-0.5, 0.5, 64, dtype=np.float32)))
        assert svc.speech("hello", "8051", response_format="pcm", timeout=30) == wav_float_to_int16(np.linspace(-0.5, 0.5, 64, dtype=np.float32)).tobytes()
        fastapi = pytest.importorskip("fastapi")      # noqa: F841
        pytest.importorskip("httpx")
        from fastapi.testclient import TestClient
        from emotivoice_amd.serving import create_app
        client = TestClient(create_app(svc))
        r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "8051", "response_format": "flac"})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == data
    finally:
        assert b.close()


def test_service_without_flac_synth_fn_answers_400():
    b, svc = _service(False)
    try:
        with pytest.raises(ValueError, match="flac_synth_fn"):
            svc.speech("hello", "8051", response_format="flac", timeout=30)
        pytest.importorskip("fastapi")
        pytest.importorskip("httpx")
        from fastapi.testclient import TestClient
        from emotivoice_amd.serving import create_app
        client = TestClient(create_app(svc))
        r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "8051", "response_format": "flac"})
        assert r.status_code == 400 and "flac_synth_fn" in r.json()["detail"]
    finally:
        assert b.close()
