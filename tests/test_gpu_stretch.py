"""ev_stretch on the device against tests/stretch_oracle.py.  There is no tolerance anywhere: the lag track, sum_dist, edge_frames, the fp32 bits and
the int16 are all the oracle's."""
import ctypes as C

import numpy as np
import pytest

import flac_oracle as fo
import stretch_oracle as so

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SR = 16000
EDGE_LENGTHS = [(1, 1), (1, 2), (2, 1), (255, 300), (257, 129), (511, 1022), (513, 257), (256, 256), (1000, 777)]


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


def _noise(seed, n, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def _speech_like(seed, n):
    """A decaying sum of a few harmonics with a drifting pitch, plus a little noise: the search has something to find."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    f0 = 110.0 + 40.0 * np.sin(2 * np.pi * t / 9000.0)
    ph = 2 * np.pi * np.cumsum(f0) / SR
    x = sum(a * np.sin(h * ph) for h, a in ((1, 0.4), (2, 0.2), (3, 0.1), (5, 0.05)))
    return (x * (0.6 + 0.4 * np.sin(2 * np.pi * t / 3000.0)) + 0.01 * rng.standard_normal(n)).astype(np.float32)


def _same_bits(got, want):
    """fp32 bit for bit; where the oracle has a NaN (0 * Inf of a non-finite input) any NaN will do."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _check(out, wavs, lens_out, int16=False):
    """Every figure and every sample of a stretch_to_numpy(want_track=True) result against the oracle, segment by segment."""
    assert out["lens_out"].tolist() == [int(v) for v in lens_out] and out["offsets"].tolist() == np.concatenate([[0], np.cumsum(lens_out)]).tolist()
    for b, (x, L_out) in enumerate(zip(wavs, lens_out)):
        w = so.stretch(x, int(L_out))
        assert out["frames"][b] == w["frames"] and np.array_equal(out["deltas_list"][b], w["deltas"]), (b, out["deltas_list"][b], w["deltas"])
        assert int(out["sum_dist"][b]) == w["sum_dist"] and out["edge_frames"][b] == w["edge_frames"] and out["nonfinite"][b] == w["nonfinite"], b
        assert _same_bits(out["wav_list"][b], w["wav"]), b
        if int16:
            assert np.array_equal(out["wav_i16_list"][b], w["wav_i16"]), b


def _run(eng, wavs, lens_out, int16=False):
    """ev_stretch on host arrays with explicit output lengths."""
    from emotivoice_amd.packing import pack_segments
    from emotivoice_amd.stretch import StretchConfig
    flat, is16, lens = pack_segments(wavs)
    res = eng.stretch_raw(len(lens), flat.ctypes.data, is16, lens, np.asarray(lens_out, np.int64), StretchConfig(want_int16=int16))
    return eng.stretch_to_numpy(res, want_track=True)


@pytest.mark.parametrize("L_in,L_out", EDGE_LENGTHS)
def test_edge_lengths_equal_the_oracle(ctx, L_in, L_out):
    x = _noise(L_in, L_in)
    _check(_run(ctx["eng"], [x], [L_out], True), [x], [L_out], True)


@pytest.mark.parametrize("speed", [0.5, 0.9, 1.1, 2.0])
def test_20011_samples_at_four_speeds_equal_the_oracle(ctx, speed):
    from emotivoice_amd.stretch import plan_lengths
    x = _speech_like(int(speed * 10), 20011)
    L_out = plan_lengths([20011], [speed])
    out = ctx["eng"].stretch([x], speed=speed, want_track=True)
    assert out["lens_in"].tolist() == [20011] and out["speed"][0] == 20011 / int(L_out[0])
    _check(out, [x], L_out)
    assert np.any(out["deltas_list"][0] != 0)


def test_a_batch_of_eight_equals_the_oracle_and_every_segment_alone(ctx):
    from emotivoice_amd.stretch import StretchConfig
    eng = ctx["eng"]
    lens = [5000, 1, 300, 20011, 777, 2, 4099, 12345]
    wavs = [_speech_like(b, n) if n > 1000 else _noise(b, n) for b, n in enumerate(lens)]
    sc = StretchConfig(speed=[1.25, None, None, 0.8, None, None, 2.0, None], samples=[None, 2, None, None, 1000, None, None, None],
                       seconds=[None, None, 0.01, None, None, None, None, 0.9])
    lens_out = sc.lengths(lens, SR)
    assert lens_out.tolist() == [4000, 2, 160, 25014, 1000, 2, 2050, 14400]
    batch = _run(eng, wavs, lens_out, True)
    _check(batch, wavs, lens_out, True)
    for b in range(8):
        alone = _run(eng, [wavs[b]], [lens_out[b]], True)
        assert alone["wav_list"][0].tobytes() == batch["wav_list"][b].tobytes() and np.array_equal(alone["wav_i16_list"][0], batch["wav_i16_list"][b]), b
        assert np.array_equal(alone["deltas_list"][0], batch["deltas_list"][b]) and alone["sum_dist"][0] == batch["sum_dist"][b], b


def test_int16_input_device_inputs_and_the_int16_output(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.stretch import StretchConfig
    eng = ctx["eng"]
    ints = [np.round(_speech_like(30 + i, n) * 32767.0).astype(np.int16) for i, n in enumerate((6000, 1, 2049))]
    floats = [x.astype(np.float32) / np.float32(32768.0) for x in ints]
    lens, lens_out = np.array([6000, 1, 2049], np.int64), np.array([5000, 1, 3000], np.int64)
    a, b = _run(eng, ints, lens_out, True), _run(eng, floats, lens_out, True)
    _check(a, ints, lens_out, True)
    assert a["wav"].tobytes() == b["wav"].tobytes() and np.array_equal(a["wav_i16"], b["wav_i16"]) and all(np.array_equal(p, q) for p, q in zip(a["deltas_list"], b["deltas_list"]))
    plain = _run(eng, floats, lens_out)      # without want_int16: no int16, the same fp32
    assert "wav_i16" not in plain and not eng.last_stretch.wav_i16 and plain["wav"].tobytes() == a["wav"].tobytes()
    for flat, is16 in ((np.concatenate(ints), True), (np.concatenate(floats), False)):
        dev = torch.from_numpy(flat).cuda()
        torch.cuda.synchronize()
        res = eng.stretch_raw(3, dev.data_ptr(), is16, lens, lens_out, StretchConfig(want_int16=True), _ffi.EV_FLAG_DEVICE_INPUTS)
        got = eng.stretch_to_numpy(res, want_track=True)
        assert got["wav"].tobytes() == a["wav"].tobytes() and np.array_equal(got["wav_i16"], a["wav_i16"]), is16
        assert all(np.array_equal(p, q) for p, q in zip(got["deltas_list"], a["deltas_list"])) and np.array_equal(got["sum_dist"], a["sum_dist"]), is16


def test_70000_samples_span_many_tiles_and_frames(ctx):
    x = _speech_like(70, 70000)
    for L_out in (61000, 83000):
        out = _run(ctx["eng"], [x], [L_out], True)
        assert out["frames"][0] == -(-L_out // 256) > 200
        _check(out, [x], [L_out], True)


def test_full_scale_and_beyond_exercises_the_clamp_of_q(ctx):
    x = _noise(5, 6000, scale=1.5)
    x[::97] = 1.0
    x[50::97] = -1.0
    x[7::501] = 3.0e38      # times 2048: +Inf before the clamp
    assert np.abs(so.quantise(x)).max() == 2047 and np.count_nonzero(np.abs(x) >= 1.0) > 1000
    _check(_run(ctx["eng"], [x], [5000], True), [x], [5000], True)


def test_nonfinite_samples_are_counted_and_decide_as_zero(ctx):
    x = _speech_like(9, 8000)
    x[[0, 5, 700, 3000, 3001, 7999]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    zeroed = np.where(np.isfinite(x), x, np.float32(0))
    for L_out in (8000, 7000):
        out = _run(ctx["eng"], [x, zeroed], [L_out, L_out], True)
        _check(out, [x, zeroed], [L_out, L_out], True)
        assert out["nonfinite"].tolist() == [6, 0] and np.array_equal(out["deltas_list"][0], out["deltas_list"][1]) and out["sum_dist"][0] == out["sum_dist"][1]


def test_periodic_input_comes_out_periodic(ctx):
    base = _noise(80, 80)
    x = np.tile(base, 250)
    for speed in (0.8, 1.25):
        out = ctx["eng"].stretch([x], speed=speed)
        y = out["wav_list"][0]
        m = np.arange(y.size - 2304)
        assert np.array_equal(y[m].view(np.uint32), base[m % 80].view(np.uint32)), speed


def test_identity_at_speed_1_on_the_vocoders_own_waveform(ctx):
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 24], [3, 8])
    plain = eng.synthesize(utts)
    assert all(np.all(np.isfinite(w)) for w in plain["wav_list"])
    out = eng.stretch(plain["wav_list"], speed=1.0, want_track=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out["wav_list"], plain["wav_list"]))
    assert not out["sum_dist"].any() and not out["edge_frames"].any() and not any(d.any() for d in out["deltas_list"])
    chained = eng.synthesize(utts, stretch=1.0)      # the same through the chain, on the device waveform
    assert all(a.tobytes() == b.tobytes() for a, b in zip(chained["wav_list"], plain["wav_list"])) and chained["stretch"]["speed"].tolist() == [1.0, 1.0]
    again = eng.synthesize(utts)      # without stretch=: the path as it was
    assert set(again) == set(plain) and all(a.tobytes() == p.tobytes() for a, p in zip(again["wav_list"], plain["wav_list"]))


def test_rejections_come_before_any_launch_and_leave_the_result(ctx):
    from emotivoice_amd import _ffi
    eng = ctx["eng"]
    lib = eng._lib
    x = _speech_like(3, 3000)
    keep = eng.stretch_raw(2, x.ctypes.data, False, np.array([2000, 1000]), np.array([1800, 1100]))
    want = eng.stretch_to_numpy(keep, want_track=True)
    _check(want, [x[:2000], x[2000:]], [1800, 1100])

    def run(B=2, wav=x, lens=(2000, 1000), lens_out=(1800, 1100), size=None, cfg_size=None, out=True):
        r = _ffi.ev_stretch_result()
        r.struct_size = C.sizeof(r) if size is None else size
        c = _ffi.ev_stretch_config()
        lib.ev_default_stretch_config(C.byref(c))
        assert (c.struct_size, c.want_int16) == (C.sizeof(c), 0)
        if cfg_size is not None:
            c.struct_size = cfg_size
        ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
        lo = None if lens_out is None else np.ascontiguousarray(lens_out, np.int64)
        rc = lib.ev_stretch(eng._h, B, None if wav is None else _p(wav), 0, None if ln is None else _p(ln), None if lo is None else _p(lo), C.byref(c), 0,
                            C.byref(r) if out else None)
        return rc, lib.ev_last_error(eng._h).decode()

    for kw, needle in ((dict(wav=None), "wav is NULL"), (dict(lens=None), "lens is NULL"), (dict(lens_out=None), "lens_out is NULL"), (dict(out=False), "out is NULL"),
                       (dict(size=24), "out->struct_size"), (dict(cfg_size=4), "cfg->struct_size"), (dict(B=0, lens=(), lens_out=()), "B = 0"),
                       (dict(B=65536, lens=[1] * 65536, lens_out=[1] * 65536), "B = 65536"), (dict(lens=(2000, 0)), "lens[1] = 0 < 1"),
                       (dict(lens_out=(0, 1100)), "lens_out[0] = 0 < 1"), (dict(lens_out=(1800, -4)), "lens_out[1] = -4 < 1"),
                       (dict(lens=(2000, (1 << 30) + 1)), "lens[1] = 1073741825 > EV_STRETCH_MAX_SAMPLES"),
                       (dict(lens_out=((1 << 30) + 1, 1100)), "lens_out[0] = 1073741825 > EV_STRETCH_MAX_SAMPLES"),
                       (dict(lens_out=(999, 1100)), "segment 0: 2000 -> 999 samples lies outside the ratios [0.5, 2]"),
                       (dict(lens_out=(4001, 1100)), "segment 0: 2000 -> 4001 samples lies outside the ratios [0.5, 2]")):
        rc, msg = run(**kw)
        assert rc < 0 and needle in msg and msg.startswith("ev_stretch: "), (kw, msg)
        got = eng.stretch_to_numpy(keep, want_track=True)      # the result of the last accepted call is still there
        assert got["wav"].tobytes() == want["wav"].tobytes() and all(np.array_equal(a, b) for a, b in zip(got["deltas_list"], want["deltas_list"]))
        assert np.array_equal(got["sum_dist"], want["sum_dist"]) and np.array_equal(got["lens_out"], want["lens_out"])
    assert run()[0] == 0
    with pytest.raises(ValueError, match="entries"):
        eng.stretch_raw(2, x.ctypes.data, False, np.array([3000]), np.array([1800, 1100]))
    with pytest.raises(ValueError, match="lens_out must have B = 2 entries"):
        eng.stretch_raw(2, x.ctypes.data, False, np.array([2000, 1000]), np.array([3000]))
    with pytest.raises(ValueError, match="segment 0: 3000 -> 1000"):
        eng.stretch([x], speed=3.0)


def test_synthesize_with_every_stage_equals_the_composition_of_the_utilities(ctx):
    """Bit for bit: the chain reads each stage's device waveform, the utilities the host copy of the same fp32 values."""
    from emotivoice_amd.limiter import pre_gain
    from emotivoice_amd.loudness import LoudnessConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 24], [3, 8])
    out = eng.synthesize(utts, denoise=0.01, stretch=[1.25, 0.8], loudness=-16, limiter=-1.0, delivery=8000, flac=True)
    clean = eng.denoise(eng.synthesize(utts)["wav_list"], 0.01)["wav_list"]
    st = eng.stretch(clean, speed=[1.25, 0.8])
    measured = eng.loudness(st["wav_list"])
    gains = np.array([pre_gain(float(l), LoudnessConfig(target_lufs=-16.0))[0] for l in measured["loudness"]], np.float32)
    limited = eng.limit(st["wav_list"], gains=gains, ceiling_dbtp=-1.0)
    delivered = eng.deliver(limited["wav_list"], 8000)["delivered_list"]
    streams = eng.flac(delivered, sample_rate=8000)["streams"]
    assert out["stretch"]["lens_in"].tolist() == [w.size for w in clean] and np.array_equal(out["stretch"]["lens_out"], st["lens_out"])
    assert np.array_equal(out["stretch"]["sum_dist"], st["sum_dist"]) and np.array_equal(out["stretch"]["edge_frames"], st["edge_frames"])
    assert out["stretch"]["speed"].tolist() == st["speed"].tolist() and np.array_equal(out["mel_lens"] * 256, [w.size for w in clean])
    for b, (g, w) in enumerate(zip(out["delivered_list"], delivered)):
        assert g.dtype == w.dtype == np.int16 and g.tobytes() == w.tobytes(), b
        assert np.array_equal(fo.decode(out["flac_list"][b], {}), w), b
    assert out["flac_list"] == streams and out["delivered_rate"] == 8000
    assert out["loudness"]["loudness"].tobytes() == measured["loudness"].tobytes() and out["loudness"]["gain"].tobytes() == gains.tobytes()
    assert out["limiter"]["min_gain"].tobytes() == limited["min_gain"].tobytes()


def test_synthesize_fit_hits_the_slot_exactly(ctx, capsys):
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 24], [3, 8])
    natural = [w.size for w in eng.synthesize(utts)["wav_list"]]
    seconds = [round(natural[0] / SR * 1.07, 3), round(natural[1] / SR * 0.93, 3)]
    out = eng.synthesize_fit(utts, seconds, want_int16=True)
    assert [len(w) for w in out["wav_list"]] == [round(s * SR) for s in seconds] == out["fit"]["target_samples"].tolist()
    assert [len(w) for w in out["wav_int16_list"]] == [round(s * SR) for s in seconds]
    assert out["fit"]["natural_samples"].tolist() == natural and np.array_equal(out["fit"]["model_samples"], out["mel_lens"].astype(np.int64) * 256)
    assert np.array_equal(out["fit"]["residual_speed"], out["stretch"]["speed"]) and all(np.all(np.isfinite(w)) for w in out["wav_list"])
    with capsys.disabled():
        print("\nsynthesize_fit: natural %s, model %s, target %s samples; |residual_speed - 1| = %s" % (
            natural, out["fit"]["model_samples"].tolist(), out["fit"]["target_samples"].tolist(), np.abs(out["fit"]["residual_speed"] - 1).tolist()))
