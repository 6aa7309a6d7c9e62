"""MI355X: ev_limit -- the 4x true-peak meter, the look-ahead limiter and the limited waveform on the device (include/evhip.h), against the numpy
restatement (tests/limit_oracle.py), bit for bit: segments around the tile and the look-ahead with full-scale clicks at their ends and on a tile's
edge, the two kernels through their test entry points, another rate, bitwise invariance, non-finite samples, rejections and lifetime, and
synthesize / synthesize_long with limiter= end to end."""
import ctypes as C

import numpy as np
import pytest

import flac_oracle as fo
import limit_oracle as mo
import loudness_oracle as lo

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = 4096      # EV_LIMIT_TILE
CEILING = mo.DEFAULT_CEILING
PEAKS = ("true_peak_in", "sample_peak_in", "true_peak_out", "sample_peak_out", "min_gain")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.limiter import interpolator
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    assert _ffi.EV_LIMIT_TILE == T
    blob, man = pack_state_dict(synth_state_dict(0, "parity"))
    eng = EVEngine(precision="mx")
    eng.load_blob(blob, man)
    yield dict(eng=eng, h=interpolator(), base=mo.voiced_half(8 * T))
    eng.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.asarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.asarray(a).dtype)


def _segments(base, lengths):
    """Pieces of the voiced signal (peak 0.5) with full-scale clicks at sample 0, at the last sample and on both sides of the first tile edge."""
    segs, at = [], 0
    for n in lengths:
        x = base[at:at + n].copy()
        at += n
        x[0] = 1.0
        x[-1] = -1.0
        if n > T:
            x[T - 1], x[T] = -1.0, 1.0
        segs.append(x)
    return segs


def _check(out, segs, gains, h, **kw):
    """Every figure and every output bit of the device result against the oracle's, segment by segment."""
    want = []
    for b, x in enumerate(segs):
        w = mo.limit(x, 1.0 if gains is None else gains[b], h=h, **kw)
        want.append(w)
        for k in PEAKS:
            assert _bits(out[k][b:b + 1]) == _bits(np.array([w[k]], np.float32)), (k, b, out[k][b], w[k])
        assert out["limited"][b] == w["limited"] and out["nonfinite"][b] == w["nonfinite"], (b, out["limited"][b], w["limited"])
        got = out["wav_list"][b]
        fin = ~np.isnan(w["wav"])
        assert np.array_equal(np.isnan(got), ~fin) and np.array_equal(_bits(got)[fin], _bits(w["wav"])[fin]), b
        if "wav_i16_list" in out:
            assert np.array_equal(out["wav_i16_list"][b], w["wav_i16"]), b
    return want


@pytest.mark.parametrize("L,Hd", [(0, 0), (1, 0), (80, 800), (80, T + 3)])
def test_limit_equals_the_oracle_bit_for_bit(ctx, L, Hd):
    """Lengths 1, 2, L, L + Hd + 1 and the tile with its neighbours, each once with gain 1 (only the clicks are limited) and once with gain 2.5;
    (80, T + 3) makes a hold span a whole tile.  r comes from the meter's kernel and s from the limiter's kernel through their test entry
    points; ev_limit's output must be what those two give."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.limiter import LimiterConfig
    eng, h = ctx["eng"], ctx["h"]
    lengths = sorted({n for n in (1, 2, L, L + Hd + 1, T - 1, T, T + 1, 3 * T + 5) if n >= 1})
    segs = _segments(ctx["base"], lengths) * 2
    gains = np.array([1.0] * len(lengths) + [2.5] * len(lengths), np.float32)
    cfg = LimiterConfig(lookahead_ms=L / 16.0, hold_ms=Hd / 16.0, want_int16=True)
    assert cfg.samples() == (L, Hd)
    lens = np.array([x.size for x in segs], np.int64)
    flat = np.concatenate(segs)
    out = eng.limit_to_numpy(eng.limit_raw(len(segs), flat.ctypes.data, False, lens, gains, cfg))
    want = _check(out, segs, gains, h, L=L, Hd=Hd)
    assert sum(w["limited"] for w in want) > 0 and any(w["min_gain"] < 0.5 for w in want)
    # the two kernels on caller-provided buffers
    lib = _ffi.lib()
    B, total = len(segs), int(lens.sum())
    x_d = torch.from_numpy(flat).cuda()
    r_d, y_d, s_d = (torch.zeros(total, dtype=torch.float32, device="cuda") for _ in range(3))
    i_d = torch.zeros(total, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    sp, tp, mn = (np.zeros(B, np.float32) for _ in range(3))
    nf, lim = np.zeros(B, np.int64), np.zeros(B, np.int64)
    assert lib.ev_op_limit_peak(x_d.data_ptr(), 0, B, _p(lens), _p(gains), float(CEILING), r_d.data_ptr(), _p(sp), _p(tp), _p(nf), None) == 0
    assert lib.ev_op_limit_apply(x_d.data_ptr(), 0, B, _p(lens), _p(gains), r_d.data_ptr(), L, Hd, y_d.data_ptr(), i_d.data_ptr(), s_d.data_ptr(), _p(mn),
                                 _p(lim), None) == 0
    r, s, y = r_d.cpu().numpy(), s_d.cpu().numpy(), y_d.cpu().numpy()
    assert np.array_equal(_bits(r), _bits(np.concatenate([w["r"] for w in want])))
    assert np.array_equal(_bits(s), _bits(np.concatenate([w["s"] for w in want])))
    assert np.array_equal(_bits(y), _bits(out["wav"])) and np.array_equal(i_d.cpu().numpy(), out["wav_i16"])
    assert np.array_equal(_bits(sp), _bits(out["sample_peak_in"])) and np.array_equal(_bits(tp), _bits(out["true_peak_in"]))
    assert np.array_equal(_bits(mn), _bits(out["min_gain"])) and np.array_equal(lim, out["limited"]) and not nf.any()
    # measure only: the same meter over y, no r written
    assert lib.ev_op_limit_peak(y_d.data_ptr(), 0, B, _p(lens), None, float(CEILING), None, _p(sp), _p(tp), _p(nf), None) == 0
    assert np.array_equal(_bits(sp), _bits(out["sample_peak_out"])) and np.array_equal(_bits(tp), _bits(out["true_peak_out"]))
    assert (s <= r).all()


def test_another_rate(ctx):
    """48 000 Hz: 5 ms and 50 ms are 240 and 2 400 samples."""
    eng, h = ctx["eng"], ctx["h"]
    segs = _segments(ctx["base"], (T + 1, 2 * T + 7, 300))
    gains = np.array([2.5, 1.0, 6.0], np.float32)
    out = eng.limit(segs, gains, sample_rate=48000, want_int16=True)
    want = _check(out, segs, gains, h, L=240, Hd=2400)
    assert all(w["limited"] > 0 for w in want)


def _same(a, b, i, j=0):
    for k in PEAKS:
        assert _bits(a[k][i:i + 1]) == _bits(b[k][j:j + 1]), (k, i)
    assert a["limited"][i] == b["limited"][j] and a["nonfinite"][i] == b["nonfinite"][j]
    assert np.array_equal(_bits(a["wav_list"][i]), _bits(b["wav_list"][j])), i
    assert np.array_equal(a["wav_i16_list"][i], b["wav_i16_list"][j]), i


def test_invariance(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.limiter import LimiterConfig
    eng = ctx["eng"]
    segs = _segments(ctx["base"], (3, T - 1, 2 * T + 5, T + 1, 777))
    gains = np.array([1.0, 2.5, 2.5, 6.0, 1.0], np.float32)
    cfg = dict(want_int16=True)
    batch = eng.limit(segs, gains, **cfg)
    assert batch["limited"][2] > 0
    # alone and at an odd offset in a batch of 5
    for i, x in enumerate(segs):
        _same(batch, eng.limit([x], gains[i:i + 1], **cfg), i)
    # device input whose segments start unaligned
    lens = np.array([s.size for s in segs], np.int64)
    d32 = torch.from_numpy(np.concatenate([np.full(1, 9.0, np.float32)] + segs)).cuda()
    torch.cuda.synchronize()
    dev = eng.limit_to_numpy(eng.limit_raw(len(segs), d32.data_ptr() + 4, False, lens, gains, LimiterConfig(**cfg), _ffi.EV_FLAG_DEVICE_INPUTS))
    for i in range(len(segs)):
        _same(batch, dev, i, i)
    # int16 input against the fp32 array s / 32768, from host and from device memory
    s16 = [lo.to_i16(x) for x in segs[1:4]]
    sf = [s.astype(np.float32) / np.float32(32768.0) for s in s16]
    a, b = eng.limit(s16, gains[1:4], **cfg), eng.limit(sf, gains[1:4], **cfg)
    d16 = torch.from_numpy(np.concatenate([np.zeros(3, np.int16)] + s16)).cuda()
    torch.cuda.synchronize()
    dev = eng.limit_to_numpy(eng.limit_raw(3, d16.data_ptr() + 6, True, lens[1:4], gains[1:4], LimiterConfig(**cfg), _ffi.EV_FLAG_DEVICE_INPUTS))
    for i in range(3):
        _same(a, b, i, i)
        _same(a, dev, i, i)
    assert a["limited"].sum() > 0


def test_non_finite_samples_and_the_int16_clamp(ctx):
    """NaN and infinite samples are counted, enter the meter as zero, stay non-finite in wav (NaN stays NaN) and give 0 / the clamp in wav_i16.
    With a ceiling of 1 a sample at +1.0 passes with its bits and becomes 32767, where a wrapping cast gives -32768."""
    eng, h = ctx["eng"], ctx["h"]
    x = ctx["base"][:T + 50].copy()
    x[[10, T - 1, T + 7]] = [np.nan, np.inf, -np.inf]
    x[[300, 400]] = [1.0, -1.0]
    click = np.zeros(64, np.float32)      # alone, a full-scale sample reads a true peak of exactly 1: every tap is below 1
    click[[20, 40]] = [1.0, -1.0]
    out = eng.limit([x, click], ceiling_dbtp=0.0, want_int16=True)
    _check(out, [x, click], None, h, ceiling=1.0)
    assert out["nonfinite"].tolist() == [3, 0] and np.isfinite(out["true_peak_in"]).all() and out["sample_peak_in"].tolist() == [1.0, 1.0]
    assert out["true_peak_in"][1] == 1.0 and out["limited"][1] == 0 and np.array_equal(_bits(out["wav_list"][1]), _bits(click))
    assert out["wav_i16_list"][1][[20, 40]].tolist() == [32767, -32768]
    y, i16 = out["wav_list"][0], out["wav_i16_list"][0]
    assert np.isnan(y[10]) and i16[10] == 0 and not np.isfinite(y[[T - 1, T + 7]]).any() and i16[[T - 1, T + 7]].tolist() == [32767, -32768]
    assert np.isfinite(np.delete(y, [10, T - 1, T + 7])).all()
    assert np.abs(i16.astype(np.int32)).max() <= 32768 and (np.sign(i16[[300, 400]]) == [1, -1]).all()      # clamped, never wrapped
    # a pre-gain that overflows fp32 makes u infinite: counted, and the finite rest is still limited
    big = np.array([3e38, 0.5, -0.25, 0.1], np.float32)
    o2 = eng.limit([big], np.array([4.0], np.float32), want_int16=True)
    _check(o2, [big], [4.0], h)
    assert o2["nonfinite"][0] == 1 and o2["wav_i16_list"][0][0] == 32767


def test_rejections_leave_the_previous_result_and_it_survives_other_calls(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.limiter import LimiterConfig
    eng, h = ctx["eng"], ctx["h"]
    lib = _ffi.lib()
    x = _segments(ctx["base"], (5000,))[0]
    g = np.array([2.5, 1.0], np.float32)
    keep = eng.limit_raw(2, x.ctypes.data, False, np.array([3000, 2000]), g, LimiterConfig(want_int16=True))
    want = eng.limit_to_numpy(keep)
    _check(want, [x[:3000], x[3000:]], g, h)

    def unchanged():
        got = eng.limit_to_numpy(keep)
        for i in range(2):
            _same(want, got, i, i)

    def run(B=2, wav=x, lens=(3000, 2000), gains=g, size=None, out=True, **cfg_kw):
        c = LimiterConfig().to_struct()
        for k, val in cfg_kw.items():
            setattr(c, k, val)
        r = _ffi.ev_limit_result()
        r.struct_size = C.sizeof(r) if size is None else size
        ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
        gn = None if gains is None else np.ascontiguousarray(gains, np.float32)
        rc = lib.ev_limit(eng._h, B, None if wav is None else _p(wav), 0, None if ln is None else _p(ln), None if gn is None else _p(gn), C.byref(c), 0,
                          C.byref(r) if out else None)
        return rc, lib.ev_last_error(eng._h).decode()

    inf, nan = float("inf"), float("nan")
    checks = [(dict(wav=None), "wav"), (dict(lens=None), "lens"), (dict(out=False), "out"), (dict(size=24), "struct_size"), (dict(struct_size=20), "struct_size"),
              (dict(B=0, lens=(), gains=None), "B = 0"), (dict(B=65536, lens=[1] * 65536, gains=None), "B = 65536"), (dict(lens=(3000, 0)), "lens[1]"),
              (dict(lens=(-5, 2000)), "lens[0]"), (dict(lens=(3000, (1 << 30) + 1)), "lens[1]"), (dict(sample_rate=11025), "sample_rate"),
              (dict(sample_rate=0), "sample_rate"), (dict(ceiling=0.0), "ceiling"), (dict(ceiling=1.5), "ceiling"), (dict(ceiling=nan), "ceiling"),
              (dict(ceiling=inf), "ceiling"), (dict(lookahead=-1), "lookahead"), (dict(lookahead=1025), "lookahead"), (dict(hold=-1), "hold"),
              (dict(hold=8193), "hold"), (dict(gains=(1.0, -0.5)), "gains[1]"), (dict(gains=(nan, 1.0)), "gains[0]"), (dict(gains=(1.0, inf)), "gains[1]")]
    for kw, needle in checks:
        rc, msg = run(**kw)
        assert rc < 0 and needle in msg, (kw, msg)
        unchanged()
    assert lib.ev_limit(None, 2, _p(x), 0, _p(np.array([3000, 2000], np.int64)), None, None, 0, C.byref(_ffi.ev_limit_result())) < 0
    eng.loudness([x], target_lufs=-20.0)
    eng.flac([lo.to_i16(x)])
    unchanged()
    with pytest.raises(ValueError, match="entries"):
        eng.limit_raw(2, x.ctypes.data, False, np.array([5000]))
    with pytest.raises(ValueError, match="gains"):
        eng.limit_raw(1, x.ctypes.data, False, np.array([5000]), np.ones(2, np.float32))
    r = eng.limit_raw(1, x.ctypes.data, False, np.array([5000]))      # a good call after them: gains and cfg NULL = 16 kHz, -1 dBTP, 80 and 800, fp32 only
    assert r.wav_i16 is None
    _check(eng.limit_to_numpy(r), [x], None, h)


def _check_limited_audio(out_lim, out_loud, wav_list, i16_list, flac_list, plain_list, h):
    """The returned audio is the oracle applied to the plain waveform with the returned pre-gain; its true peak stays within the margin; a
    stream decodes to the returned int16."""
    gains = out_loud["gain"]
    for b, x in enumerate(plain_list):
        w = mo.limit(x, gains[b], h=h)
        if wav_list is not None:
            assert np.array_equal(_bits(wav_list[b]), _bits(w["wav"])), b
        assert np.array_equal(i16_list[b], w["wav_i16"]), b
        assert np.array_equal(fo.decode(flac_list[b]), i16_list[b]), b
        for k in PEAKS:
            assert _bits(out_lim[k][b:b + 1]) == _bits(np.array([w[k]], np.float32)), (k, b)
        assert out_lim["limited"][b] == w["limited"]
        print("segment %d: pre-gain %.3f, true peak in %.4f, out %.6f, limited %d of %d" % (b, gains[b], w["true_peak_in"], w["true_peak_out"], w["limited"], x.size))
        assert float(out_lim["true_peak_out"][b]) <= float(CEILING) * (1.0 + mo.MARGIN), (b, out_lim["true_peak_out"][b])


def test_synthesize_with_limiter(ctx):
    from emotivoice_amd.limiter import pre_gain
    from emotivoice_amd.loudness import LoudnessConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng, h = ctx["eng"], ctx["h"]
    utts = synth_inputs(51, [24, 24], [3, 8])
    plain = eng.synthesize(utts)
    out = eng.synthesize(utts, loudness=-16, limiter=-1.0, want_int16=True, flac=True)
    ld = out["loudness"]
    meas = eng.loudness(plain["wav_list"])
    assert np.array_equal(ld["loudness"].view(np.uint64), meas["loudness"].view(np.uint64))
    for b in range(2):      # the pre-gain: the gain rule without its sample-peak step
        g, f = pre_gain(float(ld["loudness"][b]), LoudnessConfig(target_lufs=-16.0))
        assert ld["gain"][b] == g and ld["flags"][b] == f
    _check_limited_audio(out["limiter"], ld, out["wav_list"], out["wav_int16_list"], out["flac_list"], plain["wav_list"], h)
    assert np.array_equal(out["mel"], plain["mel"]) and np.array_equal(out["durations"], plain["durations"])
    # a target the limiter has to work for (the synthetic checkpoint's audio is louder than -16 LUFS, so nothing was limited above): the same
    # equalities, and the sample peak within one rounding of the ceiling; the true peak's overshoot on this audio is printed, no figure is set for it
    hot = eng.synthesize(utts, loudness=-6.0, limiter=-1.0, want_int16=True)
    assert hot["limiter"]["limited"].sum() > 0 and (hot["limiter"]["true_peak_in"] > CEILING).any()
    for b in range(2):
        w = mo.limit(plain["wav_list"][b], hot["loudness"]["gain"][b], h=h)
        assert np.array_equal(_bits(hot["wav_list"][b]), _bits(w["wav"])) and np.array_equal(hot["wav_int16_list"][b], w["wav_i16"]), b
        assert hot["limiter"]["limited"][b] == w["limited"] and hot["limiter"]["min_gain"][b] == w["min_gain"]
        assert float(hot["limiter"]["sample_peak_out"][b]) <= float(CEILING) * (1.0 + 2.0 ** -22)
        print("target -6 LUFS, segment %d: true peak in %.4f, out / ceiling - 1 = %.3g, limited %d" % (b, w["true_peak_in"], float(w["true_peak_out"]) / float(CEILING) - 1.0, w["limited"]))
    # the limiter alone: gains of one
    alone = eng.synthesize(utts, limiter=True)
    assert "loudness" not in alone and "wav_i16" not in alone
    for b in range(2):
        assert np.array_equal(_bits(alone["wav_list"][b]), _bits(mo.limit(plain["wav_list"][b], 1.0, h=h)["wav"])), b
    # without limiter=: the path as it was
    ref = eng.loudness(plain["wav_list"], target_lufs=-16.0, want_int16=True)
    same = eng.synthesize(utts, loudness=-16, want_int16=True, flac=True, limiter=None)
    assert "limiter" not in same and np.array_equal(_bits(same["wav"]), _bits(ref["wav"])) and np.array_equal(same["wav_i16"], ref["wav_i16"])
    assert np.array_equal(same["loudness"]["gain"], ref["gain"]) and np.array_equal(same["loudness"]["flags"], ref["flags"])
    for b in range(2):
        assert np.array_equal(fo.decode(same["flac_list"][b]), ref["wav_i16_list"][b]), b
    assert set(eng.synthesize(utts, limiter=None)) == set(plain)
    with pytest.raises(ValueError, match="vocoder"):
        eng.synthesize(utts, limiter=-1.0, vocoder=False)


def test_synthesize_long_with_limiter(ctx):
    from emotivoice_amd.longform import StitchConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng, h = ctx["eng"], ctx["h"]
    utts = synth_inputs(51, [24, 24], [3, 3])
    documents = [dict(utts=utts, pauses=["comma"])]
    mk = lambda **kw: StitchConfig(lead_ms=20.0, tail_ms=50.0, **kw)      # noqa: E731
    plain = eng.synthesize_long(documents, config=mk())
    out = eng.synthesize_long(documents, config=mk(), loudness=-16.0, limiter=-1.0, flac=True)
    assert out["documents"][0].dtype == np.int16 and np.array_equal(out["doc_lens"], plain["doc_lens"]) and out["sentence_times"] == plain["sentence_times"]
    _check_limited_audio(out["limiter"], out["loudness"], None, out["documents"], out["flac_list"], plain["documents"], h)
    f32 = eng.synthesize_long(documents, config=mk(), loudness=-16.0, limiter=-1.0)
    w = mo.limit(plain["documents"][0], f32["loudness"]["gain"][0], h=h)
    assert f32["documents"][0].dtype == np.float32 and np.array_equal(_bits(f32["documents"][0]), _bits(w["wav"]))
    same = eng.synthesize_long(documents, config=mk(), limiter=None)
    assert "limiter" not in same and np.array_equal(_bits(same["documents"][0]), _bits(plain["documents"][0]))
