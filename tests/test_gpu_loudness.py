"""MI355X: ev_loudness -- BS.1770 programme loudness, one gain per segment and the scaled waveform on the device (include/evhip.h), against the
float64 restatement (tests/loudness_oracle.py): the measurement at the edges of the block rule and of the tile, the two gates, the gain rule and
the output rules, bitwise invariance, rejections and lifetime, and synthesize / synthesize_long with loudness= end to end."""
import ctypes as C
import math

import numpy as np
import pytest

import flac_oracle as fo
import loudness_oracle as lo

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = 4096      # EV_LOUDNESS_TILE
LENGTHS_16K = (1, 2, 1599, 1600, 1601, 6399, 6400, 6401, 7999, 8000, 8001, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    assert _ffi.EV_LOUDNESS_TILE == T
    blob, man = pack_state_dict(synth_state_dict(0, "parity"))
    eng = EVEngine(precision="mx")
    eng.load_blob(blob, man)
    yield dict(eng=eng, batch16=_cut(lo.voiced(sum(LENGTHS_16K), 16000), LENGTHS_16K))
    eng.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cut(x, lengths):
    offs = np.concatenate([[0], np.cumsum(lengths)])
    return [x[offs[i]:offs[i + 1]].copy() for i in range(len(lengths))]


def _check_measurement(out, segs, sr, counted_only=False, **cfg):
    """The device's figures against the oracle's, segment by segment: block_ms to 1e-10 relative and the loudness to 1e-8 LU (the only difference is
    the order of fp64 sums through a filter of gain about 1 / (1 - r)^2 = 4500; a tile-wise fp64 evaluation on the CPU differs by 6e-13 LU);
    block_offsets, block_state, nonfinite and the peak exactly.  counted_only: block_ms is compared on the blocks above the absolute gate only.
    That is for a signal that ends in digital zeros: there y is the filter's ring-down, 1e-48 of full scale and falling, and what the two
    evaluations hold at that level is each one's own rounding of the signal before it, so their ratio is bounded by nothing (the CPU tile-wise
    evaluation differs by 2e-9 on such blocks too).  Those blocks enter no figure; that the gate drops them is checked through block_state."""
    want = [lo.measure(x, sr, **cfg) for x in segs]
    assert out["block_offsets"].tolist() == np.concatenate([[0], np.cumsum([w["block_ms"].size for w in want])]).tolist()
    worst_ms, worst_lu = 0.0, 0.0
    for b, w in enumerate(want):
        ms = out["block_ms"][b]
        assert ms.shape == w["block_ms"].shape, b
        nz = (w["block_ms"] > 0) & ((w["block_state"] > 0) | (not counted_only))
        assert (ms[w["block_state"] == 0] < 10.0 ** ((-70.0 + 0.691) / 10.0)).all(), b
        assert np.array_equal(ms[w["block_ms"] == 0], w["block_ms"][w["block_ms"] == 0]), b
        if nz.any():
            worst_ms = max(worst_ms, float(np.abs(ms[nz] / w["block_ms"][nz] - 1.0).max()))
        if math.isinf(w["loudness"]):
            assert out["loudness"][b] == w["loudness"] and out["rel_threshold"][b] == w["rel_threshold"], b
        else:
            worst_lu = max(worst_lu, abs(out["loudness"][b] - w["loudness"]), abs(out["rel_threshold"][b] - w["rel_threshold"]))
        assert out["nonfinite"][b] == w["nonfinite"] and out["peak"][b] == w["peak"], (b, out["peak"][b], w["peak"])
        assert np.array_equal(out["block_state"][b], w["block_state"]), b
    print("worst block_ms relative difference %.3g, worst loudness difference %.3g LU" % (worst_ms, worst_lu))
    assert worst_ms < 1e-10 and worst_lu < 1e-8
    return want


def test_measurement_equals_the_oracle_at_the_edges_of_blocks_and_tiles(ctx):
    """16 kHz: one sample, the 100 ms step, the 400 ms block and one more step, and the tile, each with its neighbours; every segment after the
    first starts at an unaligned offset of the packed buffer.  Three samples are not finite."""
    eng = ctx["eng"]
    segs = [s.copy() for s in ctx["batch16"]]
    segs[4][7], segs[-1][T], segs[-1][2 * T + 3] = np.nan, np.inf, -np.inf
    out = eng.loudness(segs)
    want = _check_measurement(out, segs, 16000)
    assert [w["block_ms"].size for w in want] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 1, 1, 1, 2, 4]
    assert out["nonfinite"].tolist() == [0, 0, 0, 0, 1] + [0] * 10 + [2]
    assert "wav" not in out and (out["gain"] == 1.0).all() and (out["flags"] == 0).all()
    assert eng.last_loudness.wav is None and eng.last_loudness.wav_i16 is None      # measure only


@pytest.mark.parametrize("sr,lengths", [(22050, (8819, 8820, 8821, 3 * T + 5)), (8000, (3199, 3200, 3999, 4000, 4001)),
                                        (48000, (19199, 19200, 23999, 24000, 24001))])
def test_measurement_at_other_rates(ctx, sr, lengths):
    """22 050 Hz: the step of 2 205 samples is odd and does not divide the tile.  8 000 Hz: a tile reaches into seven steps.  48 000 Hz: a step
    spans more than a tile.  One and two blocks each."""
    eng = ctx["eng"]
    segs = _cut(lo.voiced(sum(lengths), sr, seed=sr), lengths)
    want = _check_measurement(eng.loudness(segs, sample_rate=sr), segs, sr)
    assert {w["block_ms"].size for w in want} >= {1, 2}


def test_gates(ctx):
    """4 s with a stretch at -45 dB and a stretch of digital zeros: the oracle must drop blocks at both gates with no block within 0.01 LU of a
    threshold; only then is block_state compared exactly.  An all-zero segment measures -inf, keeps gain 1 and its bits, and is flagged."""
    eng = ctx["eng"]
    x = lo.gated_signal(16000)
    w = lo.measure(x, 16000)
    assert w["block_ms"].size == 37 and (w["block_state"] == 0).sum() >= 1 and (w["block_state"] == 1).sum() >= 1 and (w["block_state"] == 2).sum() >= 1
    assert np.abs(w["block_lufs"] + 70.0).min() > 0.01 and np.abs(w["block_lufs"] - w["rel_threshold"]).min() > 0.01
    zeros = np.zeros(7001, np.float32)
    zeros[5] = -0.0
    out = eng.loudness([x, zeros], target_lufs=-23.0, want_int16=True)
    _check_measurement(out, [x, zeros], 16000, counted_only=True, target_lufs=-23.0)
    assert np.array_equal(out["block_state"][0], w["block_state"])
    assert out["loudness"][1] == -np.inf and out["gain"][1] == 1.0 and out["flags"][1] == lo.UNDEFINED and out["peak"][1] == 0.0
    assert np.array_equal(out["wav_list"][1].view(np.uint32), zeros.view(np.uint32)) and not out["wav_i16_list"][1].any()
    assert out["flags"][0] == 0 and np.array_equal(out["wav_list"][0].view(np.uint32), lo.apply_gain(x, out["gain"][0]).view(np.uint32))


def _check_output(out, segs, sr, **cfg):
    """gain within one fp32 ulp of the oracle's (both round doubles that agree to 1e-11), flags equal, wav bit-equal to x * the reported gain,
    the int16 output equal to the clamping rule on that wav."""
    for b, x in enumerate(segs):
        w = lo.measure(x, sr, **cfg)
        g = out["gain"][b]
        assert abs(float(g) - float(w["gain"])) <= float(np.spacing(w["gain"])), (b, g, w["gain"])
        assert out["flags"][b] == w["flags"], (b, out["flags"][b], w["flags"])
        want = lo.apply_gain(x, g)
        assert np.array_equal(out["wav_list"][b].view(np.uint32), want.view(np.uint32)), b
        if "wav_i16_list" in out:
            assert np.array_equal(out["wav_i16_list"][b], lo.to_i16(want)), b


def test_gain_limits_and_output(ctx):
    eng = ctx["eng"]
    plain, quiet, spiky = lo.voiced(16000), lo.voiced(12001, amp=0.0005), lo.spiky(9999)
    # no limit binds: the output measures the target
    out = eng.loudness([plain, quiet], target_lufs=-23.0, max_gain_db=60.0, want_int16=True)
    _check_output(out, [plain, quiet], 16000, target_lufs=-23.0, max_gain_db=60.0)
    assert out["flags"].tolist() == [0, 0] and out["gain"][0] < 1.0 < out["gain"][1]
    again = eng.loudness(out["wav_list"])
    assert np.abs(again["loudness"] - (-23.0)).max() < 1e-4, again["loudness"]
    # a quiet signal with target 0: the boost limit
    out = eng.loudness([quiet, plain], target_lufs=0.0)
    _check_output(out, [quiet, plain], 16000, target_lufs=0.0)
    assert out["flags"][0] == lo.BOOST_LIMITED and out["gain"][0] == np.float32(10.0) and "wav_i16" not in out
    # a spiky signal: the peak limit; int16 input takes the same path
    spiky16 = lo.to_i16(spiky)
    out = eng.loudness([spiky, plain], target_lufs=-16.0, want_int16=True)
    _check_output(out, [spiky, plain], 16000, target_lufs=-16.0)
    assert out["flags"][0] == lo.PEAK_LIMITED and float(np.abs(out["wav_list"][0]).max()) <= lo.measure(spiky)["peak"] * float(out["gain"][0]) * (1 + 1e-6)
    out16 = eng.loudness([spiky16], target_lufs=-16.0, want_int16=True)
    _check_output(out16, [spiky16], 16000, target_lufs=-16.0)
    assert out16["flags"][0] == lo.PEAK_LIMITED


def test_int16_output_clamps_and_never_wraps(ctx):
    """peak_ceiling = 1.  A finite sample cannot leave [-1, 1] here: |x| g <= p fl(1 / p) <= 1 + 2^-24, which rounds to 1.  What reaches past
    int16 is the sample that lands on +1.0 exactly (32768), and the infinite ones.  (a) Samples at exactly +-1.0 and a target far above: the gain
    is 1, the bits pass, +1.0 becomes 32767 where a wrapping cast gives -32768.  (b) A peak of 0.5 scaled by 2 onto +-1.0: the same through the
    product.  Infinite samples clamp, NaN becomes 0."""
    eng = ctx["eng"]
    base = lo.voiced(8000, amp=0.01)
    a = base.copy()
    a[[100, 200]] = [1.0, -1.0]
    p = np.float32(0.5)
    b = base.copy()
    b[[300, 400, 500, 600, 700]] = [p, -p, np.inf, -np.inf, np.nan]
    cfg = dict(target_lufs=0.0, max_gain_db=80.0, peak_ceiling=1.0)
    want_b = lo.apply_gain(b, lo.measure(b, 16000, **cfg)["gain"])
    assert want_b[300] == 1.0 and want_b[400] == -1.0 and lo.measure(b, 16000, **cfg)["gain"] == 2.0      # the oracle's own scaled peak is full scale
    out = eng.loudness([a, b], want_int16=True, **cfg)
    _check_output(out, [a, b], 16000, **cfg)
    assert out["gain"][0] == 1.0 and out["flags"].tolist() == [lo.PEAK_LIMITED, lo.PEAK_LIMITED] and out["nonfinite"].tolist() == [0, 3]
    assert out["wav_i16_list"][0][[100, 200]].tolist() == [32767, -32768]
    assert out["wav_i16_list"][1][[300, 400, 500, 600, 700]].tolist() == [32767, -32768, 32767, -32768, 0]
    assert np.array_equal(out["wav_list"][0].view(np.uint32), a.view(np.uint32))      # gain 1: the source bits


def _same(a, b, i, j=0):
    """Segment i of result a and segment j of result b agree in every bit, doubles included."""
    for k in ("loudness", "rel_threshold"):
        assert a[k][i:i + 1].view(np.uint64) == b[k][j:j + 1].view(np.uint64), (k, i)
    for k in ("gain", "peak"):
        assert a[k][i:i + 1].view(np.uint32) == b[k][j:j + 1].view(np.uint32), (k, i)
    assert a["flags"][i] == b["flags"][j] and a["nonfinite"][i] == b["nonfinite"][j]
    assert np.array_equal(a["block_ms"][i].view(np.uint64), b["block_ms"][j].view(np.uint64)), i
    assert np.array_equal(a["block_state"][i], b["block_state"][j]), i
    assert np.array_equal(a["wav_list"][i].view(np.uint32), b["wav_list"][j].view(np.uint32)), i
    assert np.array_equal(a["wav_i16_list"][i], b["wav_i16_list"][j]), i


def test_invariance(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.loudness import LoudnessConfig
    eng, segs = ctx["eng"], ctx["batch16"]
    cfg = dict(target_lufs=-20.0, want_int16=True)
    batch = eng.loudness(segs, **cfg)
    # every segment alone
    for i, x in enumerate(segs):
        _same(batch, eng.loudness([x], **cfg), i)
    # device input, none of whose segments but a few starts 16-byte aligned
    flat = np.concatenate([np.full(1, 9.0, np.float32)] + segs)
    d32 = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    lens = np.array([s.size for s in segs], np.int64)
    r = eng.loudness_raw(len(segs), d32.data_ptr() + 4, False, lens, LoudnessConfig(**cfg), _ffi.EV_FLAG_DEVICE_INPUTS)
    dev = eng.loudness_to_numpy(r)
    for i in range(len(segs)):
        _same(batch, dev, i, i)
    # int16 input against the fp32 array s / 32768
    s16 = [lo.to_i16(x) for x in segs[8:]]
    sf = [s.astype(np.float32) / np.float32(32768.0) for s in s16]
    a, b = eng.loudness(s16, **cfg), eng.loudness(sf, **cfg)
    for i in range(len(s16)):
        _same(a, b, i, i)
    d16 = torch.from_numpy(np.concatenate([np.zeros(3, np.int16)] + s16)).cuda()
    torch.cuda.synchronize()
    r = eng.loudness_raw(len(s16), d16.data_ptr() + 6, True, np.array([s.size for s in s16], np.int64), LoudnessConfig(**cfg), _ffi.EV_FLAG_DEVICE_INPUTS)
    dev = eng.loudness_to_numpy(r)
    for i in range(len(s16)):
        _same(a, dev, i, i)


def test_rejections_leave_the_previous_result_and_it_survives_other_calls(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.loudness import LoudnessConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    lib = _ffi.lib()
    x = lo.voiced(5000)
    keep = eng.loudness_raw(2, x.ctypes.data, False, np.array([3000, 2000]), LoudnessConfig(target_lufs=-20.0, want_int16=True))
    want = eng.loudness_to_numpy(keep)
    _check_output(want, [x[:3000], x[3000:]], 16000, target_lufs=-20.0)

    def unchanged():
        got = eng.loudness_to_numpy(keep)
        for i in range(2):
            _same(want, got, i, i)

    def run(B=2, wav=x, lens=(3000, 2000), size=None, out=True, **cfg_kw):
        c = LoudnessConfig(target_lufs=-20.0).to_struct()
        for k, val in cfg_kw.items():
            setattr(c, k, val)
        r = _ffi.ev_loudness_result()
        r.struct_size = C.sizeof(r) if size is None else size
        ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
        rc = lib.ev_loudness(eng._h, B, None if wav is None else _p(wav), 0, None if ln is None else _p(ln), C.byref(c), 0, C.byref(r) if out else None)
        return rc, lib.ev_last_error(eng._h).decode()

    inf, nan = float("inf"), float("nan")
    checks = [(dict(wav=None), "wav"), (dict(lens=None), "lens"), (dict(out=False), "out"), (dict(size=24), "struct_size"), (dict(struct_size=20), "struct_size"),
              (dict(B=0, lens=()), "B = 0"), (dict(B=65536, lens=[1] * 65536), "B = 65536"), (dict(lens=(3000, 0)), "lens[1]"), (dict(lens=(-5, 2000)), "lens[0]"),
              (dict(lens=(3000, (1 << 30) + 1)), "lens[1]"), (dict(sample_rate=11025), "sample_rate"), (dict(sample_rate=0), "sample_rate"),
              (dict(target_lufs=0.5), "target_lufs"), (dict(target_lufs=-70.5), "target_lufs"), (dict(target_lufs=-inf), "target_lufs"),
              (dict(max_gain_db=-0.5), "max_gain_db"), (dict(max_gain_db=inf), "max_gain_db"), (dict(max_gain_db=nan), "max_gain_db"),
              (dict(peak_ceiling=0.0), "peak_ceiling"), (dict(peak_ceiling=1.5), "peak_ceiling"), (dict(peak_ceiling=nan), "peak_ceiling")]
    for kw, needle in checks:
        rc, msg = run(**kw)
        assert rc < 0 and needle in msg, (kw, msg)
        unchanged()
    assert lib.ev_loudness(None, 2, _p(x), 0, _p(np.array([3000, 2000], np.int64)), None, 0, C.byref(_ffi.ev_loudness_result())) < 0
    syn = eng.synthesize(synth_inputs(9, [20]))
    eng.flac([lo.to_i16(x)])
    unchanged()
    assert np.isfinite(syn["wav"]).all()
    with pytest.raises(ValueError, match="entries"):
        eng.loudness_raw(2, x.ctypes.data, False, np.array([5000]))
    r = eng.loudness_raw(1, x.ctypes.data, False, np.array([5000]))      # a good call after them: cfg NULL = 16 kHz, measure only
    assert r.wav is None and abs(eng.loudness_to_numpy(r)["loudness"][0] - lo.measure(x)["loudness"]) < 1e-8


def test_synthesize_with_loudness(ctx):
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 11], [3, 8])
    plain = eng.synthesize(utts)
    same = eng.synthesize(utts, loudness=None)
    assert np.array_equal(plain["wav"].view(np.uint32), same["wav"].view(np.uint32)) and "loudness" not in same and set(plain) == set(same)
    ref = eng.loudness(plain["wav_list"], target_lufs=-20.0, want_int16=True)
    out = eng.synthesize(utts, loudness=-20, want_int16=True, flac=True)
    for k in ("loudness", "rel_threshold"):
        assert np.array_equal(out["loudness"][k].view(np.uint64), ref[k].view(np.uint64)), k
    assert np.array_equal(out["loudness"]["gain"].view(np.uint32), ref["gain"].view(np.uint32)) and np.array_equal(out["loudness"]["flags"], ref["flags"])
    assert np.array_equal(out["wav"].view(np.uint32), ref["wav"].view(np.uint32)) and np.array_equal(out["wav_i16"], ref["wav_i16"])
    for b in range(2):
        assert np.array_equal(out["wav_list"][b].view(np.uint32), ref["wav_list"][b].view(np.uint32)), b
        assert np.array_equal(out["wav_int16_list"][b], ref["wav_i16_list"][b]), b
        assert np.array_equal(fo.decode(out["flac_list"][b]), out["wav_int16_list"][b]), b
        assert np.array_equal(out["loudness"]["block_ms"][b].view(np.uint64), ref["block_ms"][b].view(np.uint64)), b
    assert np.array_equal(out["mel"], plain["mel"]) and np.array_equal(out["durations"], plain["durations"])
    with pytest.raises(ValueError, match="vocoder"):
        eng.synthesize(utts, loudness=-20, vocoder=False)


def test_synthesize_long_with_loudness(ctx):
    from emotivoice_amd.longform import StitchConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 11, 17, 9], [3, 3, 8, 8])
    documents = [dict(utts=utts[:2], pauses=["comma"]), (utts[2:], [-4.0])]
    mk = lambda **kw: StitchConfig(lead_ms=20.0, tail_ms=50.0, **kw)      # noqa: E731
    plain = eng.synthesize_long(documents, config=mk())
    out = eng.synthesize_long(documents, config=mk(), loudness=-20.0)
    ld = out["loudness"]
    assert ld["gain"].shape == (2,) and "loudness" not in plain and np.array_equal(out["doc_lens"], plain["doc_lens"])
    assert out["sentence_times"] == plain["sentence_times"] and np.array_equal(out["seg_pos"], plain["seg_pos"])
    again = eng.loudness(out["documents"])
    for d in range(2):      # one gain per document: the balance between its sentences is the stitched one
        assert np.array_equal(out["documents"][d].view(np.uint32), lo.apply_gain(plain["documents"][d], ld["gain"][d]).view(np.uint32)), d
        assert ld["flags"][d] != 0 or abs(again["loudness"][d] - (-20.0)) < 1e-4, (d, ld["flags"][d], again["loudness"][d])
        w = lo.measure(plain["documents"][d], 16000, target_lufs=-20.0)
        assert abs(ld["loudness"][d] - w["loudness"]) < 1e-8 and ld["flags"][d] == w["flags"], d
    enc = eng.synthesize_long(documents, config=mk(), loudness=-20.0, flac=True)
    for d in range(2):
        assert enc["documents"][d].dtype == np.int16 and np.array_equal(enc["documents"][d], lo.to_i16(out["documents"][d])), d
        assert np.array_equal(fo.decode(enc["flac_list"][d]), enc["documents"][d]), d
