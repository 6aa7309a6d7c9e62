"""MI355X: ev_deliver -- the response at the client's rate and encoding on the device (include/evhip.h), against the numpy restatement
(tests/deliver_oracle.py), byte for byte and with no tolerance: the rate pairs with lengths around the 1024-output tile, every int16 code through
mu-law and A-law, the dither, the input forms, the rejections, and synthesize / synthesize_long with delivery= end to end."""
import ctypes as C

import numpy as np
import pytest

import deliver_oracle as do
import flac_oracle as fo
import resample_oracle as ro

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SR = 16000
PAIRS = (8000, 24000, 48000, 44100, 22050, 16000)      # 1/2, 3/2, 3/1, 441/160, 441/320, copy
ENCODINGS = (do.F32, do.S16, do.ULAW, do.ALAW)
BASE_LENS = (1, 2, 3, 255, 1023, 1024, 1025, 4099)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    blob, man = pack_state_dict(synth_state_dict(0, "parity"))
    eng = EVEngine(precision="mx")
    eng.load_blob(blob, man)
    yield dict(eng=eng)
    eng.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _tile_edge_len(sr_out):
    """The shortest input length above 1024 whose OUTPUT length is 1024 k + 1."""
    up, down = ro.ratio(SR, sr_out)
    return next(L for L in range(1025, 20000) if ro.output_len(L, up, down) % 1024 == 1)


def _noise(seed, n):
    """Noise in [-1, 1] with a few samples at +-1.0, so that the conversion clamps."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    x[rng.integers(0, n, max(1, n // 64))] = 1.0
    x[rng.integers(0, n, max(1, n // 64))] = -1.0
    return x


def _run(eng, wavs, dc, seeds=None, sr_in=SR):
    """EVEngine.deliver plus the raw bytes of the result."""
    out = eng.deliver(wavs, dc, sr_in, seeds)
    out["raw"] = eng.d2h(eng.last_deliver.data, (int(eng.last_deliver.total_bytes),), np.uint8)
    return out


def _check(out, want, encoding):
    """Every byte, the layout and the figures of a result against the oracle's per-utterance dicts."""
    n = np.array([w["data"].size for w in want], np.int64)
    offs = do.slots(n, encoding)
    assert np.array_equal(out["n_samples"], n) and np.array_equal(out["byte_offsets"], offs) and (offs % 16 == 0).all()
    assert out["raw"].size == offs[-1]
    for b, w in enumerate(want):
        got = out["delivered_list"][b]
        assert got.dtype == w["data"].dtype and got.tobytes() == w["data"].tobytes(), (encoding, b, n[b])
        assert not out["raw"][offs[b] + w["data"].nbytes:offs[b + 1]].any(), (encoding, b)      # the padding is zero
        assert np.float32(out["peak"][b]).tobytes() == np.float32(w["peak"]).tobytes() and out["clipped"][b] == w["clipped"], (encoding, b, out["peak"][b], w["peak"])


@pytest.mark.parametrize("sr_out", PAIRS)
def test_rate_pair_equals_the_oracle_byte_for_byte(ctx, sr_out):
    from emotivoice_amd.delivery import DeliveryConfig
    eng = ctx["eng"]
    lens = BASE_LENS + (_tile_edge_len(sr_out),)
    wavs = [_noise(100 + i, L) for i, L in enumerate(lens)]
    h, up, down, _ = ro.design(SR, sr_out)
    ys = [ro.resample32(x, h, up, down) for x in wavs]
    assert ro.output_len(lens[-1], up, down) % 1024 == 1
    rs = eng.resample(wavs, SR, sr_out=sr_out)["wav_list"]
    clipped = 0
    for enc in ENCODINGS:
        want = [do.convert(y, enc) for y in ys]
        out = _run(eng, wavs, DeliveryConfig(sr_out, enc))
        _check(out, want, enc)
        clipped += int(out["clipped"].sum())
        if enc == do.F32:      # ev_resample's own bits
            for b, y in enumerate(rs):
                assert out["delivered_list"][b].tobytes() == y.tobytes(), b
    assert clipped > 0      # the inputs reach the clamp


# The forms of the kernel that the rate pairs above do not reach: a long custom filter or a large rate ratio pushes the table, the tile's run of
# inputs, or both out of LDS.  (case, sr_in, sr_out, half of the custom taps or None for the default design, input lengths whose output lengths are
# 1, 2, 1023, 1024, 1025, and where the launcher must put (run, padded, table).)
THROUGH_L1 = ((0, 16000, 8000, 4900, (1, 3, 2046, 2048, 2050), (True, True, False)),
              (1, 24000, 16000, 5000, (1, 3, 1534, 1536, 1537), (True, False, False)),
              (2, 48000, 1000, None, (1, 49, 49104, 49152, 49153), (False, False, True)),
              (3, 50000, 1000, 8200, (1, 51, 51150, 51200, 51201), (False, False, False)))


def _placement(up, down, half, tile=1024, max_run_bytes=49152, max_lds=65536):
    """launch_deliver's choice restated: (run in LDS, run padded, table in LDS)."""
    pad = down >= 2 * up
    run = ((tile - 1) * down + 2 * half) // up + 2
    run_bytes = 4 * (run + run // 32 + 1 if pad else run)
    run_lds = run_bytes <= max_run_bytes
    tab_bytes = 4 * up * (((2 * half) // up + 1) | 1)
    return run_lds, run_lds and pad, (run_bytes if run_lds else 0) + tab_bytes <= max_lds


@pytest.mark.parametrize("case,sr_in,sr_out,half,lens,placement", THROUGH_L1)
def test_forms_that_read_through_l1_equal_the_oracle_byte_for_byte(ctx, case, sr_in, sr_out, half, lens, placement):
    from emotivoice_amd import _ffi
    from emotivoice_amd.delivery import DeliveryConfig
    eng = ctx["eng"]
    up, down = ro.ratio(sr_in, sr_out)
    taps = None if half is None else (0.01 * np.random.default_rng(200 + case).standard_normal(2 * half + 1)).astype(np.float32)
    used_half = ro.design(sr_in, sr_out)[3] if half is None else half
    assert _ffi.EV_DELIVER_TILE == 1024 and _placement(up, down, used_half) == placement      # a new tile or LDS limit must not uncover the case
    assert [ro.output_len(L, up, down) for L in lens] == [1, 2, 1023, 1024, 1025]
    wavs = [_noise(300 + 10 * case + i, L) for i, L in enumerate(lens)]
    s16 = [do.deliver(x, sr_in, sr_out, do.S16, taps=taps) for x in wavs]
    for enc, want in ((do.S16, s16), (do.F32, [do.convert(w["y"], do.F32) for w in s16])):      # the oracle's y once: F32 is its bytes
        _check(_run(eng, wavs, DeliveryConfig(sr_out, enc, taps=taps), sr_in=sr_in), want, enc)


def test_every_int16_code_through_the_copy_path(ctx):
    from emotivoice_amd.delivery import DeliveryConfig
    eng = ctx["eng"]
    codes = np.arange(-32768, 32768).astype(np.int16)
    for x in (codes, codes.astype(np.float32) / np.float32(32768.0)):      # s / 32768 is exact
        assert np.array_equal(_run(eng, [x], DeliveryConfig(SR, "s16"))["delivered_list"][0], codes)
        assert np.array_equal(_run(eng, [x], DeliveryConfig(SR, "ulaw"))["delivered_list"][0], do.ulaw(codes))
        assert np.array_equal(_run(eng, [x], DeliveryConfig(SR, "alaw"))["delivered_list"][0], do.alaw(codes))


@pytest.mark.parametrize("sr_out", (24000, 16000))
def test_dither_equals_the_oracle_and_depends_on_utterance_seed_and_index_alone(ctx, sr_out):
    from emotivoice_amd.delivery import DeliveryConfig
    eng = ctx["eng"]
    wavs = [_noise(7, 3000) * np.float32(0.01), _noise(8, 1025), _noise(9, 5)]
    seeds = np.array([12345, 0, 0xFFFFFFFF], np.uint32)
    for enc in (do.S16, do.ULAW, do.ALAW):
        out = _run(eng, wavs, DeliveryConfig(sr_out, enc, dither=True, seed=77), seeds)
        _check(out, [do.deliver(x, SR, sr_out, enc, True, int(s)) for x, s in zip(wavs, seeds)], enc)
    dc = DeliveryConfig(sr_out, "s16", dither=True, seed=77)
    _check(_run(eng, wavs, dc), [do.deliver(x, SR, sr_out, "s16", True, 77) for x in wavs], "s16")      # no seeds: the config's
    alone = _run(eng, wavs[:1], dc, seeds[:1])["delivered_list"][0]
    first = _run(eng, wavs, dc, seeds)["delivered_list"][0]
    last = _run(eng, [wavs[1], wavs[2], wavs[0]], dc, seeds[[1, 2, 0]])["delivered_list"][2]
    other = _run(eng, wavs[:1], dc, np.array([12346], np.uint32))["delivered_list"][0]
    assert alone.tobytes() == first.tobytes() == last.tobytes() and alone.tobytes() != other.tobytes()
    plain = _run(eng, wavs[:1], DeliveryConfig(sr_out, "s16"))["delivered_list"][0]
    assert plain.tobytes() != alone.tobytes()


def test_dither_mean_and_variance_on_the_device(ctx):
    """A constant of 0.25 LSB over 65 536 samples through the copy path: the mean of q within 6 sigma = 6 * 0.5 / sqrt(65536) = 0.0117 LSB, the
    error variance within 2 % of 1/4 LSB^2; without dither the rule returns 0."""
    from emotivoice_amd.delivery import DeliveryConfig
    eng = ctx["eng"]
    x = np.full(65536, 0.25 / 32768.0, np.float32)
    q = _run(eng, [x], DeliveryConfig(SR, "s16", dither=True, seed=12345))["delivered_list"][0].astype(np.float64)
    print("mean error %.5f LSB, error variance %.5f" % (abs(q.mean() - 0.25), ((q - 0.25) ** 2).mean()))
    assert abs(q.mean() - 0.25) <= 6 * 0.5 / np.sqrt(65536) and abs(((q - 0.25) ** 2).mean() - 0.25) <= 0.02 * 0.25
    assert not _run(eng, [x], DeliveryConfig(SR, "s16"))["delivered_list"][0].any()


def test_int16_and_device_inputs_give_the_same_bytes(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.delivery import DeliveryConfig
    eng = ctx["eng"]
    ints = [np.round(_noise(20 + i, L) * 32767.0).astype(np.int16) for i, L in enumerate((1500, 1, 2049))]
    floats = [x.astype(np.float32) / np.float32(32768.0) for x in ints]
    lens = np.array([x.size for x in ints], np.int64)
    for sr_out, enc in ((8000, "ulaw"), (44100, "s16"), (16000, "alaw"), (24000, "f32")):
        dc = DeliveryConfig(sr_out, enc)
        a = _run(eng, ints, dc)
        b = _run(eng, floats, dc)
        assert a["raw"].tobytes() == b["raw"].tobytes() and np.array_equal(a["clipped"], b["clipped"]) and a["peak"].tobytes() == b["peak"].tobytes()
        for flat, is16 in ((np.concatenate(ints), True), (np.concatenate(floats), False)):
            dev = torch.from_numpy(flat).cuda()
            torch.cuda.synchronize()
            res = eng.deliver_raw(3, dev.data_ptr(), is16, lens, None, _ffi.EV_FLAG_DEVICE_INPUTS)
            assert eng.d2h(res.data, (int(res.total_bytes),), np.uint8).tobytes() == a["raw"].tobytes(), (sr_out, enc, is16)


def test_rejections_come_before_any_launch_and_leave_the_setup_and_the_result(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.delivery import DeliveryConfig
    from emotivoice_amd.engine import EVEngine, EVError
    eng = ctx["eng"]
    lib = eng._lib
    x = _noise(3, 3000)
    dc = DeliveryConfig(8000, "ulaw")
    eng.deliver_setup(dc, SR)
    keep = eng.deliver_raw(2, x.ctypes.data, False, np.array([2000, 1000]))
    want = eng.deliver_to_numpy(keep, dc)
    _check(dict(want, raw=eng.d2h(keep.data, (int(keep.total_bytes),), np.uint8)), [do.deliver(x[:2000], SR, 8000, "ulaw"), do.deliver(x[2000:], SR, 8000, "ulaw")], "ulaw")

    def unchanged():      # reads ``keep``, the result of the last accepted call
        got = eng.deliver_to_numpy(keep, dc)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got["delivered_list"], want["delivered_list"])) and np.array_equal(got["clipped"], want["clipped"])

    def setup(size=None, **kw):
        c = _ffi.ev_deliver_config()
        lib.ev_default_deliver_config(C.byref(c))
        assert (c.struct_size, c.sr_in, c.sr_out, c.encoding, c.dither, c.seed, c.taps) == (C.sizeof(c), 16000, 16000, _ffi.EV_DELIVER_S16, 0, 0, None)
        c.sr_out, c.encoding = 8000, _ffi.EV_DELIVER_ULAW
        for k, v in kw.items():
            setattr(c, k, v)
        if size is not None:
            c.struct_size = size
        return lib.ev_deliver_setup(eng._h, C.byref(c)), lib.ev_last_error(eng._h).decode()

    def run(B=2, wav=x, lens=(2000, 1000), size=None, out=True):
        r = _ffi.ev_deliver_result()
        r.struct_size = C.sizeof(r) if size is None else size
        ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
        rc = lib.ev_deliver(eng._h, B, None if wav is None else _p(wav), 0, None if ln is None else _p(ln), None, 0, C.byref(r) if out else None)
        return rc, lib.ev_last_error(eng._h).decode()

    bad_taps = np.array([0.0, np.nan, 0.0], np.float32)
    for kw, needle in ((dict(size=8), "struct_size"), (dict(encoding=4), "encoding"), (dict(encoding=-1), "encoding"), (dict(dither=2), "dither"),
                       (dict(dither=1, encoding=_ffi.EV_DELIVER_F32), "dither"), (dict(sr_out=16001), "EV_RESAMPLE_MAX_RATIO"), (dict(sr_in=0), "sr_in"),
                       (dict(sr_in=16000 * 1025, sr_out=16000), "EV_RESAMPLE_MAX_RATIO"), (dict(taps=bad_taps.ctypes.data, half_len=1), "taps[1]"),
                       (dict(taps=bad_taps.ctypes.data, half_len=0), "half_len")):
        rc, msg = setup(**kw)
        assert rc < 0 and needle in msg, (kw, msg)
        keep = eng.deliver_raw(2, x.ctypes.data, False, np.array([2000, 1000]))      # the previous setup still works, and gives the same bytes
        unchanged()
    for kw, needle in ((dict(wav=None), "wav"), (dict(lens=None), "lens"), (dict(out=False), "out"), (dict(size=24), "struct_size"),
                       (dict(B=0, lens=()), "B = 0"), (dict(B=65536, lens=[1] * 65536), "B = 65536"), (dict(lens=(2000, 0)), "lens[1]"),
                       (dict(lens=(-5, 1000)), "lens[0]"), (dict(lens=(2000, 2 * 16384 * 256 + 1)), "lens[1]")):
        rc, msg = run(**kw)
        assert rc < 0 and needle in msg, (kw, msg)
        unchanged()
    fresh = EVEngine(precision="mx")
    try:
        with pytest.raises(EVError, match="ev_deliver_setup has not been called"):
            fresh.deliver_raw(1, x.ctypes.data, False, np.array([100]))
    finally:
        fresh.close()
    # its setup is its own: ev_resample_setup does not disturb it, nor the reverse
    rs = eng.resample([x], SR, sr_out=22050)["wav_list"][0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_run(eng, [x[:2000], x[2000:]], dc)["delivered_list"], want["delivered_list"]))
    assert eng.resample([x], SR, sr_out=22050)["wav_list"][0].tobytes() == rs.tobytes()
    with pytest.raises(ValueError, match="entries"):
        eng.deliver_raw(2, x.ctypes.data, False, np.array([3000]))
    with pytest.raises(ValueError, match="seeds"):
        eng.deliver_raw(1, x.ctypes.data, False, np.array([3000]), np.zeros(2, np.uint32))


def test_synthesize_with_delivery(ctx):
    from emotivoice_amd.delivery import DeliveryConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 24], [3, 8])
    plain = eng.synthesize(utts)
    ref = eng.synthesize(utts, loudness=-16, limiter=-1.0)
    out = eng.synthesize(utts, loudness=-16, limiter=-1.0, delivery=DeliveryConfig(8000, "ulaw"))
    assert out["delivered_rate"] == 8000 and "wav" not in out and np.array_equal(out["loudness"]["gain"], ref["loudness"]["gain"])
    for b, x in enumerate(ref["wav_list"]):
        w = do.deliver(x, SR, 8000, "ulaw")
        got = out["delivered_list"][b]
        assert got.dtype == np.uint8 and got.tobytes() == w["data"].tobytes(), b
        assert np.float32(out["delivery"]["peak"][b]).tobytes() == np.float32(w["peak"]).tobytes() and out["delivery"]["clipped"][b] == w["clipped"]
    fl = eng.synthesize(utts, loudness=-16, limiter=-1.0, delivery=DeliveryConfig(24000), flac=True)
    for b, x in enumerate(ref["wav_list"]):
        info = {}
        pcm = fo.decode(fl["flac_list"][b], info)
        assert info["sample_rate"] == 24000 and fl["delivered_list"][b].dtype == np.int16 and np.array_equal(pcm, fl["delivered_list"][b]), b
        assert np.array_equal(fl["delivered_list"][b], do.deliver(x, SR, 24000, "s16")["data"]), b
    bare = eng.synthesize(utts, delivery=44100)      # no earlier stage: the vocoder's waveform
    for b, x in enumerate(plain["wav_list"]):
        assert np.array_equal(bare["delivered_list"][b], do.deliver(x, SR, 44100, "s16")["data"]), b
    with pytest.raises(ValueError, match="s16"):
        eng.synthesize(utts, delivery=DeliveryConfig(8000, "alaw"), flac=True)
    with pytest.raises(ValueError, match="vocoder"):
        eng.synthesize(utts, delivery=8000, vocoder=False)
    again = eng.synthesize(utts)      # without delivery=: the path as it was
    assert set(again) == set(plain) and all(a.tobytes() == p.tobytes() for a, p in zip(again["wav_list"], plain["wav_list"]))


def test_synthesize_long_with_delivery(ctx):
    from emotivoice_amd.delivery import DeliveryConfig
    from emotivoice_amd.longform import StitchConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 24], [3, 3])
    documents = [dict(utts=utts, pauses=["comma"])]
    mk = lambda **kw: StitchConfig(lead_ms=20.0, tail_ms=50.0, **kw)      # noqa: E731
    ref = eng.synthesize_long(documents, config=mk(), limiter=-1.0)
    out = eng.synthesize_long(documents, config=mk(), limiter=-1.0, delivery=DeliveryConfig(48000, "s16", dither=True, seed=5), flac=True)
    w = do.deliver(ref["documents"][0], SR, 48000, "s16", True, 5)
    info = {}
    assert out["delivered_rate"] == 48000 and out["sample_rate"] == SR and out["sentence_times"] == ref["sentence_times"]
    assert out["documents"] is out["delivered_list"] and np.array_equal(out["documents"][0], w["data"])
    assert np.array_equal(fo.decode(out["flac_list"][0], info), w["data"]) and info["sample_rate"] == 48000


def _composed(eng, wavs, dn, rate=24000):
    """What the chain with every stage on must deliver, from the public host-array utilities one after the other: denoise, the loudness
    measurement, the host pre-gain, the limiter, delivery as int16 at ``rate`` and FLAC of that int16."""
    from emotivoice_amd.delivery import DeliveryConfig
    from emotivoice_amd.limiter import pre_gain
    from emotivoice_amd.loudness import LoudnessConfig
    clean = eng.denoise(wavs, dn)["wav_list"]
    measured = eng.loudness(clean)
    gains = np.array([pre_gain(float(l), LoudnessConfig(target_lufs=-16.0))[0] for l in measured["loudness"]], np.float32)
    limited = eng.limit(clean, gains=gains, ceiling_dbtp=-1.0)
    delivered = eng.deliver(limited["wav_list"], DeliveryConfig(rate))["delivered_list"]
    return dict(delivered_list=delivered, flac_list=eng.flac(delivered, sample_rate=rate)["streams"], loudness=measured["loudness"], gain=gains,
                min_gain=limited["min_gain"])


def _check_composed(out, want):
    assert len(out["delivered_list"]) == len(want["delivered_list"]) and len(out["flac_list"]) == len(want["flac_list"])
    for b, (g, w) in enumerate(zip(out["delivered_list"], want["delivered_list"])):
        assert g.dtype == w.dtype == np.int16 and g.tobytes() == w.tobytes(), b
    assert out["flac_list"] == want["flac_list"]
    assert out["loudness"]["loudness"].tobytes() == want["loudness"].tobytes() and out["loudness"]["gain"].tobytes() == want["gain"].tobytes()
    assert out["limiter"]["min_gain"].tobytes() == want["min_gain"].tobytes()


def _explicit_bias():
    """A DenoiseConfig that carries its bias, so that no call in between measures the vocoder's (which would run the vocoder)."""
    from emotivoice_amd.denoise import DenoiseConfig
    return DenoiseConfig(strength=0.1, bias=(0.02 + 0.01 * np.cos(np.arange(513) * 0.05)).astype(np.float32))


def test_synthesize_with_every_stage_equals_the_composition_of_the_utilities(ctx):
    """Bit for bit: the chain reads each stage's device waveform, the utilities the host copy of the same fp32 values."""
    from emotivoice_amd.delivery import DeliveryConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 24], [3, 8])
    dn = _explicit_bias()
    out = eng.synthesize(utts, denoise=dn, loudness=-16, limiter=-1.0, delivery=DeliveryConfig(24000), flac=True)
    _check_composed(out, _composed(eng, eng.synthesize(utts)["wav_list"], dn))


def test_synthesize_long_with_every_stage_equals_the_composition_of_the_utilities(ctx):
    from emotivoice_amd.delivery import DeliveryConfig
    from emotivoice_amd.longform import StitchConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    documents = [dict(utts=synth_inputs(51, [24, 24], [3, 3]), pauses=["comma"])]
    cfg = StitchConfig(lead_ms=20.0, tail_ms=50.0)
    dn = _explicit_bias()
    out = eng.synthesize_long(documents, config=cfg, denoise=dn, loudness=-16, limiter=-1.0, delivery=DeliveryConfig(24000), flac=True)
    _check_composed(out, _composed(eng, eng.synthesize_long(documents, config=cfg)["documents"], dn))
