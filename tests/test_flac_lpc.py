"""CPU: the numpy restatement of ev_flac_lpc (tests/flac_lpc_oracle.py) against its own decoder, against today's streams and against hashlib;
the branches its signal set reaches; FlacConfig's new fields."""
import hashlib

import numpy as np
import pytest

import flac_lpc_oracle as lo
import flac_oracle as fo


@pytest.fixture(scope="module")
def runs():
    """Every signal at every block size and (max_lpc_order, qlp_precision): the stream, its info, the events; and today's stream per block size."""
    sig = lo.signal_set()
    out = dict(signals=sig, streams={}, info={}, events={}, base={})
    for N in lo.BLOCKS:
        for name, x in sig.items():
            out["base"][N, name] = fo.encode(x, block_size=N)
        for L, q in lo.CONFIGS:
            ev = set()
            for name, x in sig.items():
                info = {}
                out["streams"][N, L, q, name] = lo.encode(x, block_size=N, max_lpc_order=L, qlp_precision=q, md5=True, info=info, events=ev)
                out["info"][N, L, q, name] = info
            out["events"][N, L, q] = ev
    return out


def test_streams_decode_to_the_input(runs):
    for (N, L, q, name), data in runs["streams"].items():
        info = {}
        assert np.array_equal(lo.decode(data, info), runs["signals"][name]), (N, L, q, name)
        assert info["md5_checked"] and info["block_size"] == N
        assert info["frame_kind"] == runs["info"][N, L, q, name]["frame_kind"].tolist()


# ---------------------------------------------------------------------------------------------------------------- the decoder on its own
def _bits(v, n):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def _rice(r, k):
    u = 2 * r if r >= 0 else -2 * r - 1
    return [0] * (u >> k) + [1] + _bits(u & ((1 << k) - 1), k)


def _hand_stream(n, type_code, warm, prec, shift, coefs, res, k, method=0):
    """One frame of n samples assembled field by field: subframe type, warm-ups, precision, shift, coefficients, one Rice partition."""
    b = [0] + _bits(type_code, 6) + [0]
    for v in warm:
        b += _bits(v & 0xFFFF, 16)
    b += _bits(prec - 1, 4) + _bits(shift & 31, 5)
    for c in coefs:
        b += _bits(c & ((1 << prec) - 1), prec)
    b += _bits(method, 2) + _bits(0, 4) + _bits(k, 4 if method == 0 else 5)
    for r in res:
        b += _rice(r, k)
    b += [0] * (-len(b) % 8)
    hdr = bytes([0xFF, 0xF8, (6 << 4) | 5, 4 << 1, 0, n - 1])
    hdr += bytes([fo.crc8(hdr)])
    body = hdr + np.packbits(np.array(b, np.uint8)).tobytes()
    c = fo.crc16(body)
    frame = body + bytes([c >> 8, c & 0xFF])
    return fo.stream_header(n, 16000, 256, len(frame), len(frame)) + frame


def _synth(warm, coefs, shift, res, flipped=False, logical=False):
    x = list(warm)
    c = list(reversed(coefs)) if flipped else list(coefs)
    for r in res:
        s = sum(c[j] * x[-1 - j] for j in range(len(c)))
        x.append(r + (((s & 0xFFFFFFFFFFFFFFFF) >> shift) if logical else (s >> shift)))
    return x


def test_decoder_reads_a_hand_assembled_lpc_frame():
    warm, coefs, shift, prec = [100, -50, 30], [5, -7, 2], 2, 5
    res = [3, -2, 0, 7, -9, 1, 4, -4, 2]
    want = _synth(warm, coefs, shift, res)
    # by hand, the first two: 3 + ((5 * 30 - 7 * -50 + 2 * 100) >> 2) = 3 + 175 = 178; -2 + ((5 * 178 - 7 * 30 + 2 * -50) >> 2) = -2 + 145 = 143
    assert want[3:5] == [178, 143]
    assert any(sum(coefs[j] * want[i - 1 - j] for j in range(3)) < 0 for i in range(3, len(want)))      # the arithmetic shift matters
    n = len(want)
    info = {}
    got = lo.decode(_hand_stream(n, 32 + 2, warm, prec, shift, coefs, res, 2), info).tolist()
    assert got == want and info["frame_kind"] == [34]
    assert got == lo.decode(_hand_stream(n, 32 + 2, warm, prec, shift, coefs, res, 3, method=1)).tolist()      # 5-bit Rice parameters
    assert got != _synth(warm, coefs, shift, res, flipped=True)
    assert got != _synth(warm, coefs, shift, res, logical=True)
    # a wrong warm-up count: the type says order 2, three warm-ups were written
    try:
        wrong = lo.decode(_hand_stream(n, 32 + 1, warm, prec, shift, coefs[:2], res, 2)).tolist()
    except ValueError:
        wrong = None
    assert wrong != want
    with pytest.raises(ValueError, match="negative LPC shift"):
        lo.decode(_hand_stream(n, 32 + 2, warm, prec, -1, coefs, res, 2))
    with pytest.raises(ValueError, match="precision code 15"):
        lo.decode(_hand_stream(n, 32 + 2, warm, 16, shift, coefs, res, 2))
    with pytest.raises(ValueError, match="LPC subframe"):
        fo.decode(_hand_stream(n, 32 + 2, warm, prec, shift, coefs, res, 2))      # today's decoder refuses what this one reads
    bad = bytearray(_hand_stream(n, 32 + 2, warm, prec, shift, coefs, res, 2))
    bad[42 + 9] ^= 0x10      # a bit of the first warm-up sample
    with pytest.raises(ValueError, match="CRC-16"):
        lo.decode(bytes(bad))
    bad = bytearray(_hand_stream(n, 32 + 2, warm, prec, shift, coefs, res, 2))
    bad[30] = 1      # a digest that is not the samples'
    with pytest.raises(ValueError, match="MD5"):
        lo.decode(bytes(bad))


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_the_signal_set_reaches_every_branch(runs):
    ev = set().union(*runs["events"].values())
    named = {e for e in ev if isinstance(e, str)}
    assert {e[1] for e in ev if e[0] == "lpc"} == set(range(1, 13))                                       # every LPC order chosen
    assert {"shift_clamped", "shift_negative", "coef_clamped", "r0_zero"} <= named
    assert "shift_negative" in {e for e in runs["events"][4096, 12, 5] if isinstance(e, str)}              # q = 5 on smooth signals
    assert 0 in {e[1] for e in ev if e[0] == "margin"}                                                    # an exact FIXED-vs-LPC tie: FIXED is taken
    assert {e[1] for e in ev if e[0] == "short_block"} >= {1, 2, 3, 10}                                   # last blocks of m <= max_lpc_order samples
    x = runs["signals"]["binary01"][:4096]
    assert lo.analyse(x, 12, 12)[0][0] == 0 and not np.all(x == x[0])                                     # R[0] = 0 on a block that is not constant


def test_levinson_stop():
    """err <= 0 ends the recursion and later orders are no candidates.  No int16 block of the signal set reaches it: a pure alternation of
    +-32767 at m = 4096, the most predictable block tried, leaves err / R[0] near 2e-9 at order 12, seven orders of magnitude above the
    rounding of fp64, so the branch is held to a hand-made autocorrelation."""
    shift, coef, ev = np.full(12, -1, np.int64), np.zeros((12, 12), np.int64), set()
    lo.levinson(np.array([4, 2, 4, 2, 4] + [0] * 8, np.int64), 4, 12, shift, coef, ev)      # k_1 = 1 / 2, k_2 = 1: err = 0 at order 2
    assert "levinson_stop" in ev and shift.tolist() == [11] + [-1] * 11 and coef[0, 0] == 1 << 10
    ev = set()
    _, shift, _ = lo.analyse(fo.signal_set()["alternation"][:4096], 12, 12, ev)
    assert "levinson_stop" not in ev and (shift >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- sizes
def test_never_longer_and_shorter_where_there_is_a_spectrum(runs):
    for (N, L, q, name), data in runs["streams"].items():
        assert len(data) <= len(runs["base"][N, name]), (N, L, q, name)
    for N in lo.BLOCKS:
        for L, q in ((8, 12), (12, 12)):
            for name in ("sine440", "sine80_noise", "alternation", "ar2"):
                assert len(runs["streams"][N, L, q, name]) < len(runs["base"][N, name]), (N, L, q, name)
    ratio = {name: len(runs["streams"][4096, 12, 12, name]) / len(runs["base"][4096, name]) for name in runs["signals"]}
    assert ratio["sine440"] < 0.65 and ratio["alternation"] < 0.1 and ratio["sine80_noise"] < 0.72 and ratio["noise_full"] == 1.0


def test_identity_without_lpc_and_md5(runs):
    for N in lo.BLOCKS:
        for name, x in runs["signals"].items():
            assert lo.encode(x, block_size=N) == runs["base"][N, name], (N, name)
            assert lo.encode(x, block_size=N, md5=True)[:26] == runs["base"][N, name][:26]
            assert lo.encode(x, block_size=N, md5=True)[42:] == runs["base"][N, name][42:]


@pytest.mark.parametrize("nbytes_mod", [0, 2, 54, 56, 62])
def test_md5_field_at_the_padding_edges(nbytes_mod):
    """Sample bytes of 0, 2, 54 (the last length that pads within its round), 56 and 62 mod 64 (16-bit samples: the byte count is even, so 55 and 63
    are reached as 54 and 62, the even lengths on either side of the one-round / two-round edge at 55 | 56)."""
    rng = np.random.default_rng(nbytes_mod)
    for rounds in (0, 1, 3):
        n = (64 * rounds + nbytes_mod) // 2
        if n == 0:
            n = 32
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        data = lo.encode(x, block_size=256, max_lpc_order=4, md5=True)
        assert data[26:42] == hashlib.md5(x.astype("<i2").tobytes()).digest()
        assert np.array_equal(lo.decode(data), x)
        assert lo.encode(x, block_size=256, max_lpc_order=4)[26:42] == bytes(16)


# ---------------------------------------------------------------------------------------------------------------- FlacConfig
def test_flac_config_fields_and_ext():
    import ctypes as C
    from emotivoice_amd import _ffi
    from emotivoice_amd.flac import KIND_LPC, FlacConfig
    assert KIND_LPC == 32 == lo.KIND_LPC
    assert FlacConfig().validate().to_ext() is None and FlacConfig(qlp_precision=9).validate().to_ext() is None
    e = FlacConfig(max_lpc_order=8, md5=True).validate().to_ext()
    assert (e.struct_size, e.max_lpc_order, e.qlp_precision, e.md5, list(e.reserved)) == (C.sizeof(_ffi.ev_flac_ext), 8, 12, 1, [0] * 4)
    assert C.sizeof(_ffi.ev_flac_ext) == 32
    e = FlacConfig(md5=True).to_ext()
    assert (e.max_lpc_order, e.md5) == (0, 1)
    e = FlacConfig(max_lpc_order=12, qlp_precision=15).to_ext()
    assert (e.max_lpc_order, e.qlp_precision, e.md5) == (12, 15, 0)
    for kw in (dict(max_lpc_order=13), dict(max_lpc_order=-1), dict(qlp_precision=4), dict(qlp_precision=16), dict(md5=2), dict(md5="yes")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            FlacConfig(**kw).validate()
    c = FlacConfig(max_lpc_order=8, md5=True).to_struct()      # to_struct is the ev_flac_config it always was
    assert C.sizeof(c) == 24 and (c.sample_rate, c.block_size, c.max_fixed_order, c.max_partition_order, c.convert) == (16000, 4096, 4, 5, 0)


def test_flac_synth_fn_passes_the_service_config():
    """engine_flac_synth_fn(flac_config=): the batch is encoded whole with that config, and utterances outside the mask still come back as waveforms;
    without it the call is today's, with the mask."""
    from emotivoice_amd.flac import FlacConfig
    from emotivoice_amd.serving import engine_flac_synth_fn

    class Eng:
        def synthesize(self, utts, flac=None, **kw):
            self.seen = (flac, kw)
            return dict(flac_list=[b"fLaC%d" % i for i in range(len(utts))], wav_list=[np.full(2, i, np.float32) for i in range(len(utts))])

    eng, fc = Eng(), FlacConfig(max_lpc_order=8, md5=True)
    got = engine_flac_synth_fn(eng, flac_config=fc)([{}, {}, {}], 1.0, [True, False, True])
    assert eng.seen[0] is fc and eng.seen[1] == dict(alpha=1.0)
    assert got[0] == b"fLaC0" and got[2] == b"fLaC2" and np.array_equal(got[1], np.full(2, 1, np.float32))
    engine_flac_synth_fn(eng)([{}, {}], 1.0, [True, False])
    assert eng.seen[0] == [True, False]
    with pytest.raises(ValueError, match="max_lpc_order"):
        engine_flac_synth_fn(eng, flac_config=FlacConfig(max_lpc_order=13))
