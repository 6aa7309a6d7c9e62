"""MI355X: ev_watermark and ev_watermark_detect (include/evhip.h) against tests/watermark_oracle.py.

Embed.  E = max |y - y64| / max |y64| per segment against the float64 oracle.  The bar is tests/test_gpu_denoise.py's whole-call bar -- 4 x the
largest error the reference's own float32 STFT round trip shows over the fixtures in tests/golden/denoise -- times the largest gain a: at
strength 0 the arithmetic IS ev_denoise's at strength 0 (bit for bit, tested below), and a gain g <= a scales a cell and with it the cell's
forward error, the 2^-22 of its hi / lo split and what the inverse GEMM adds per unit of spectrum by at most a; 1 / a < 1 scales them down.

Detect.  q is held to the interval the oracle gives every cell when each magnitude is off by up to FWD_BAR = 4 x 2^-22 of its frame's largest
(what ev_features and ev_denoise hold this GEMM to) and each of the five fp32 operations of D1 - D3 by half an ulp.  A cell whose X interval is
wider than a point and contains 0 is OPEN; the device's sums may differ from the oracle's by the open count and no more, and every decision must
be the oracle's.  On the CPU side the fixtures must have at most 2 % open cells and no oracle decision within the open count of its threshold."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import denoise_oracle as do
import watermark_oracle as wo
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FWD_BAR = 4 * 2.0 ** -22      # tests/test_gpu_denoise.py
KEY, SR = 0x5EED1234, 16000


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


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
    errs = [float(np.load(p)["ref_err"]) for p in glob.glob(os.path.join(GOLDEN_DIR, "denoise", "dn_[a-h]_*.npz"))]
    assert len(errs) == 8
    bar = 4 * max(errs)
    assert 1e-6 < bar < 1e-5
    speech, rich = wo.speech_like(3, 4 * SR), wo.harmonic_rich(3, 4 * SR)
    marked = dict(speech_like=wo.embed64(speech, KEY).astype(np.float32), harmonic_rich=wo.embed64(rich, KEY, 8, 0xA5).astype(np.float32))
    yield dict(eng=eng, bar=bar, speech=speech, rich=rich, marked=marked, plain=dict(speech_like=speech, harmonic_rich=rich))
    eng.close()


def _cfg(**kw):
    from emotivoice_amd.watermark import WatermarkConfig
    return WatermarkConfig(**dict(dict(key=KEY), **kw))


@pytest.mark.parametrize("L,i16", ((513, False), (2048, False), (2304, True), (16384, False), (32768, False)))
def test_embed_against_the_float64_oracle(ctx, L, i16):
    """513 samples are three frames; 2048 / 2304 samples end on and one frame past a time tile's edge; 16 384 are 65 frames, the 64-frame block
    edge; 32 768 are 129 frames, where the pattern's period wraps.  A second, short segment rides along so that rows of a neighbour lie next
    to the edges.  2 dB, an 8-bit payload."""
    eng = ctx["eng"]
    w, other = ctx["speech"][:L], ctx["rich"][5000:5700]
    if i16:
        w, other = (np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16) for x in (w, other))
    out = eng.watermark([w, other], _cfg(payload=0x5A, nbits=8, strength_db=2.0, want_int16=True))
    a = float(wo.gains_f32(2.0)[0])
    assert out["lens_out"].tolist() == [L // 256 * 256, 512]
    for y, x in zip(out["wav_list"], (w, other)):
        e = do.peak_error(y, wo.embed64(x, KEY, 8, 0x5A, 2.0))
        print("L", x.size, "int16" if i16 else "fp32", "E %.3e bar %.3e" % (e, ctx["bar"] * a))
        assert e <= ctx["bar"] * a
    assert np.array_equal(out["wav_i16"], do.to_i16(out["wav"]))


def test_embed_negative_control_the_bar_sees_one_inverted_band(ctx):
    y = ctx["eng"].watermark([ctx["speech"][:16384]], _cfg())["wav_list"][0]
    a = float(wo.gains_f32(1.0)[0])
    assert do.peak_error(y, wo.embed64(ctx["speech"][:16384], KEY)) <= ctx["bar"] * a
    assert do.peak_error(y, wo.embed64(ctx["speech"][:16384], KEY, invert_band=17)) > ctx["bar"] * a
    assert do.peak_error(y, wo.embed64(ctx["speech"][:16384], KEY, tile_shift=1)) > ctx["bar"] * a


def test_a_batch_of_three_equals_every_segment_alone_and_device_inputs(ctx):
    from emotivoice_amd import _ffi
    eng = ctx["eng"]
    wavs = [ctx["speech"][:20011], ctx["rich"][:513], ctx["speech"][30000:46640]]
    cfg = _cfg(payload=[0x3, 0, 0xBEEF], nbits=[2, 0, 16], strength_db=[0.5, 1.0, 2.0])
    batch = [w.copy() for w in eng.watermark(wavs, cfg)["wav_list"]]
    for b, w in enumerate(wavs):
        alone = eng.watermark([w], _cfg(payload=cfg.payload[b], nbits=cfg.nbits[b], strength_db=cfg.strength_db[b]))["wav_list"][0]
        assert np.array_equal(_bits(alone), _bits(batch[b])), b
    flat = torch.from_numpy(np.concatenate(wavs)).cuda()
    torch.cuda.synchronize()
    res = eng.watermark_raw(3, flat.data_ptr(), False, np.array([w.size for w in wavs], np.int64), cfg, _ffi.EV_FLAG_DEVICE_INPUTS)
    for b, y in enumerate(eng.watermark_to_numpy(res)["wav_list"]):
        assert np.array_equal(_bits(y), _bits(batch[b])), b
    assert not np.array_equal(_bits(batch[0]), _bits(eng.watermark([wavs[0]], _cfg(payload=0x1, nbits=2, strength_db=0.5))["wav_list"][0]))


def test_strength_zero_is_ev_denoise_at_strength_zero_bit_for_bit(ctx):
    from emotivoice_amd.denoise import DenoiseConfig
    eng = ctx["eng"]
    wavs = [ctx["speech"][:20011], ctx["rich"][:513], ctx["rich"][:16640]]
    marked = eng.watermark(wavs, _cfg(strength_db=0.0, payload=0x2A, nbits=8, want_int16=True))
    clean = eng.denoise(wavs, DenoiseConfig(strength=0.0, bias=np.ones(513, np.float32), want_int16=True))
    assert marked["lens_out"].tolist() == clean["lens_out"].tolist() and np.array_equal(_bits(marked["wav"]), _bits(clean["wav"]))
    assert np.array_equal(marked["wav_i16"], clean["wav_i16"])


@pytest.mark.parametrize("kind", ("nan", "inf"))
def test_embed_gives_zero_cells_for_a_non_finite_sample(ctx, kind):
    """include/evhip.h, Embed step 3: mag == 0 (and a NaN) gives a zero cell.  One NaN (or +inf, whose lo plane is inf - inf) in segment 0: the four
    frames that hold it contribute nothing, the output is finite and is the oracle's with those frames zeroed; segment 1 keeps its bits."""
    eng = ctx["eng"]
    i0 = 2400
    clean, other = ctx["speech"][:4869].copy(), ctx["rich"][5000:5700]
    bad = clean.copy()
    bad[i0] = np.float32(np.nan if kind == "nan" else np.inf)
    clean[i0] = 0.0
    re, im = do.stft64(clean, wo.N_FFT, wo.HOP)
    g = wo.gain_map(re.shape[0], wo.pattern(KEY, 8, 0x5A)[0], 2.0)
    dead = np.arange((i0 - wo.N_FFT // 2) // wo.HOP + 1, (i0 + wo.N_FFT // 2) // wo.HOP + 1)
    assert dead.tolist() == [8, 9, 10, 11]
    g[dead] = 0.0
    want = do.istft64(g * re, g * im, wo.N_FFT, wo.HOP)
    cfg = _cfg(payload=0x5A, nbits=8, strength_db=2.0, want_int16=True)
    out = eng.watermark([bad, other], cfg)
    y = out["wav_list"][0]
    e, a = do.peak_error(y, want), float(wo.gains_f32(2.0)[0])
    print(kind, "E %.3e bar %.3e non-finite outputs %d" % (e, ctx["bar"] * a, int((~np.isfinite(out["wav"])).sum())))
    assert np.all(np.isfinite(out["wav"])) and e <= ctx["bar"] * a and np.array_equal(out["wav_i16"], do.to_i16(out["wav"]))
    alone = eng.watermark([other], cfg)["wav_list"][0]
    assert np.array_equal(_bits(alone), _bits(out["wav_list"][1]))


def _oracle_side(wav, key, nbits, marked=True):
    """The oracle's decisions, its intervals and the CPU-side conditions on a fixture.  An unmarked fixture has one decision, absent: the offset
    and the bits of an absent mark are the argmax of noise and mean nothing, so nothing is asked of them."""
    q, lo, hi = wo.band_q(wav, FWD_BAR)
    folded = wo.fold(q, lo, hi)
    d = wo.correlate(folded, key, nbits)
    p = d["offset"] % wo.TILE
    cells = int(folded["A"][p].sum())
    open_all = int(folded["O"][p].sum())
    assert open_all <= 0.02 * cells, (open_all, cells)                                   # at most 2 % open cells
    k = d["open"]
    # present / absent cannot flip: C moves by at most k, and so does n, which moves the threshold 6.25 sqrt(n) by at most 6.25 k / (2 sqrt(n))
    assert abs(d["C"] - wo.THRESHOLD * np.sqrt(d["n"])) > k * (1 + wo.THRESHOLD / (2 * np.sqrt(max(d["n"], 1))))
    op = folded["O"].sum(axis=(1, 2))[np.arange(wo.OFFSETS) % wo.TILE]                  # the open cells of every offset's phase
    d["open_at"] = op
    if not marked:
        return q, lo, hi, d, open_all
    for b in range(nbits):
        assert abs(int(d["bit_C"][b])) > int(d["bit_open"][b]), b                          # no bit can flip
    # no other offset can overtake: its z with every open cell of its phase in its favour stays below the reported one with every open cell against it
    z_all = np.where(d["C_all"] + op > 0, (d["C_all"] + op) / np.sqrt(np.maximum(d["n_all"] - op, 1)), 0.0)
    z_all[d["offset"]] = -np.inf
    assert (d["C"] - open_all) / np.sqrt(d["n"] + open_all) > z_all.max(), (d["z"], z_all.max())
    return q, lo, hi, d, open_all


@pytest.mark.parametrize("name,nbits", (("speech_like", 0), ("harmonic_rich", 8)))
@pytest.mark.parametrize("state", ("marked", "plain"))
def test_detect_against_the_oracle(ctx, name, nbits, state):
    eng = ctx["eng"]
    wav = ctx[state][name]
    q, lo, hi, d, open_all = _oracle_side(wav, KEY, nbits, state == "marked")
    got = eng.watermark_detect([wav, ctx["speech"][:700]], KEY, nbits, want_q=True)      # a short neighbour: three frames, no interior tile
    qd = got["q_list"][0]
    assert qd.shape == q.shape == (wav.size // 256 + 1, 48)
    outside = int(((qd < lo) | (qd > hi)).sum())
    print(name, state, "q: %d of %d cells differ from the float64 q, %d outside the interval; open %d; z %.2f offset %d" %
          (int((qd != q).sum()), q.size, outside, open_all, d["z"], d["offset"]))
    assert outside == 0
    rep = got["report"][0]
    print(name, state, "device C %d n %d offset %d | oracle C %d n %d offset %d" % (got["C"][0], got["n"][0], got["offset"][0], d["C"], d["n"], d["offset"]))
    assert rep["present"] == d["present"] == (state == "marked")
    s = rep["offset"]      # an absent mark: the sums at whatever offset the device reports against the oracle's at that offset
    assert abs(int(got["C"][0]) - int(d["C_all"][s])) <= d["open_at"][s] and abs(int(got["n"][0]) - int(d["n_all"][s])) <= d["open_at"][s]
    if state == "marked":
        assert s == d["offset"] and abs(int(got["C"][0]) - d["C"]) <= d["open"] and abs(int(got["n"][0]) - d["n"]) <= d["open"]
        assert rep["bits"] == d["bits"] and rep["payload"] == d["payload"] == (0xA5 if nbits else 0)
        for b in range(nbits):
            assert abs(int(got["bit_C"][0][b]) - int(d["bit_C"][b])) <= int(d["bit_open"][b]), b
    assert np.all(got["bit_C"][0][nbits:] == 0) and np.all(got["bit_n"][0][nbits:] == 0)
    assert (got["C"][1], got["n"][1], got["offset"][1]) == (0, 0, 0) and not got["report"][1]["present"]
    # the integers follow from the device's own q exactly: the correlation kernel against the oracle's integer half
    own = wo.correlate(wo.fold(qd), KEY, nbits)
    assert (own["C"], own["n"], own["offset"]) == (got["C"][0], got["n"][0], got["offset"][0])
    assert np.array_equal(own["bit_C"], got["bit_C"][0]) and np.array_equal(own["bit_n"], got["bit_n"][0])


@pytest.mark.parametrize("L", (513, 2048, 2304, 16640, 33000))
def test_correlation_is_exact_on_the_device_s_own_q_at_every_edge(ctx, L):
    """Fewer than three tiles (no interior tile: C = n = 0), exactly eight frames, a partial last tile, more than 64 frames, a wrapped period;
    int16 input and a wrong key; in a batch and alone."""
    eng = ctx["eng"]
    w = np.clip(np.round(ctx["marked"]["speech_like"][:L] * 32768.0), -32768, 32767).astype(np.int16)
    got = eng.watermark_detect([w, w[:600]], KEY ^ 5, 16, want_q=True)
    for b in range(2):
        own = wo.correlate(wo.fold(got["q_list"][b]), KEY ^ 5, 16)
        assert (own["C"], own["n"], own["offset"]) == (got["C"][b], got["n"][b], got["offset"][b]), b
        assert np.array_equal(own["bit_C"], got["bit_C"][b]) and np.array_equal(own["bit_n"], got["bit_n"][b]), b
    alone = eng.watermark_detect([w], KEY ^ 5, 16, want_q=True)
    assert np.array_equal(alone["q_list"][0], got["q_list"][0]) and alone["C"][0] == got["C"][0] and alone["offset"][0] == got["offset"][0]


def test_device_embed_then_device_detect_and_the_front_cut(ctx):
    eng = ctx["eng"]
    y = eng.watermark([ctx["speech"], ctx["rich"]], _cfg())["wav_list"]
    got = eng.watermark_detect([y[0], y[1], y[0][1000:], ctx["speech"]], KEY)["report"]
    print([(round(r["z"], 2), r["offset"]) for r in got])
    assert [r["present"] for r in got] == [True, True, True, False] and [r["offset"] for r in got[:3]] == [0, 0, 124]
    assert all(r["z"] >= 1.25 * wo.THRESHOLD for r in got[:3])
    assert not any(r["present"] for r in eng.watermark_detect(list(y), KEY ^ 0x1111)["report"])


def test_rejections_come_before_any_launch_and_leave_the_result(ctx):
    from emotivoice_amd import _ffi
    eng = ctx["eng"]
    lib = eng._lib
    x = ctx["speech"][:3000].copy()
    keep = eng.watermark_raw(2, x.ctypes.data, False, np.array([2000, 1000]), _cfg())
    want = eng.watermark_to_numpy(keep)["wav"].copy()
    keep_d = eng.watermark_detect_raw(2, x.ctypes.data, False, np.array([2000, 1000]), KEY)
    want_q = np.concatenate(eng.watermark_detect_to_numpy(keep_d, want_q=True)["q_list"])

    def embed(B=2, wav=x, lens=(2000, 1000), size=None, cfg_size=None, out=True, payloads=None, nbits=None, db=None):
        r = _ffi.ev_watermark_result()
        r.struct_size = C.sizeof(r) if size is None else size
        c = _ffi.ev_watermark_config()
        lib.ev_default_watermark_config(C.byref(c))
        assert (c.struct_size, c.key, c.want_i16, c.nbits, c.payload, c.strength_db) == (C.sizeof(c), 0, 0, 0, 0, 1.0)
        if cfg_size is not None:
            c.struct_size = cfg_size
        ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
        arrs = [None if v is None else np.ascontiguousarray(v, t) for v, t in ((payloads, np.uint32), (nbits, np.int32), (db, np.float32))]
        rc = lib.ev_watermark(eng._h, B, None if wav is None else _p(wav), 0, None if ln is None else _p(ln), C.byref(c),
                              *[None if a is None else _p(a) for a in arrs], 0, C.byref(r) if out else None)
        return rc, lib.ev_last_error(eng._h).decode()

    def detect(B=2, wav=x, lens=(2000, 1000), size=None, out=True, nbits=0):
        r = _ffi.ev_watermark_detect_result()
        r.struct_size = C.sizeof(r) if size is None else size
        ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
        rc = lib.ev_watermark_detect(eng._h, B, None if wav is None else _p(wav), 0, None if ln is None else _p(ln), C.c_uint32(KEY), nbits, 0,
                                     C.byref(r) if out else None)
        return rc, lib.ev_last_error(eng._h).decode()

    shared = ((dict(wav=None), "wav is NULL"), (dict(lens=None), "lens is NULL"), (dict(out=False), "out is NULL"), (dict(size=8), "out->struct_size"),
              (dict(B=0, lens=()), "B = 0"), (dict(B=65536, lens=[513] * 65536), "B = 65536"), (dict(lens=(2000, 512)), "lens[1] = 512 < n_fft / 2 + 1"),
              (dict(B=1, lens=(16384 * 256,)), "frames > EV_ALIGN_MAX_FRAMES"))
    for kw, needle in shared + ((dict(cfg_size=4), "cfg->struct_size"), (dict(nbits=(0, 17)), "nbits[1] = 17"), (dict(nbits=(-1, 0)), "nbits[0] = -1"),
                                (dict(nbits=(2, 0), payloads=(4, 0)), "payloads[0] = 4 does not fit 2 bits"), (dict(db=(1.0, 6.5)), "strengths_db[1]"),
                                (dict(db=(-0.1, 1.0)), "strengths_db[0]"), (dict(db=(float("nan"), 1.0)), "strengths_db[0]")):
        rc, msg = embed(**kw)
        assert rc < 0 and needle in msg and msg.startswith("ev_watermark: "), (kw, msg)
        assert eng.watermark_to_numpy(keep)["wav"].tobytes() == want.tobytes()      # the result of the last accepted call is still there
    for kw, needle in shared + ((dict(nbits=17), "nbits = 17"), (dict(nbits=-1), "nbits = -1")):
        rc, msg = detect(**kw)
        assert rc < 0 and needle in msg and msg.startswith("ev_watermark_detect: "), (kw, msg)
        assert np.array_equal(np.concatenate(eng.watermark_detect_to_numpy(keep_d, want_q=True)["q_list"]), want_q)
    assert embed()[0] == 0 and detect()[0] == 0
    with pytest.raises(ValueError, match="entries"):
        eng.watermark_raw(2, x.ctypes.data, False, np.array([3000]), _cfg())
    with pytest.raises(ValueError, match="one entry per segment"):
        eng.watermark([x, x], _cfg(nbits=[0, 0, 0]))


def test_synthesize_with_every_stage_equals_the_composition_of_the_utilities(ctx):
    """Bit for bit: the chain reads each stage's device waveform, the utilities the host copy of the same fp32 values.  Without watermark= the
    path is the one it was."""
    from emotivoice_amd.delivery import DeliveryConfig
    from emotivoice_amd.limiter import pre_gain
    from emotivoice_amd.loudness import LoudnessConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 24], [3, 8])
    wc = _cfg(payload=[0x11, 0x2], nbits=[8, 2], strength_db=[1.0, 2.0])
    out = eng.synthesize(utts, stretch=[1.25, 0.8], watermark=wc, loudness=-16, limiter=-1.0, delivery=DeliveryConfig(8000, "ulaw"))
    plain = eng.synthesize(utts)
    st = eng.stretch(plain["wav_list"], speed=[1.25, 0.8])
    marked = eng.watermark(st["wav_list"], wc)
    measured = eng.loudness(marked["wav_list"])
    gains = np.array([pre_gain(float(l), LoudnessConfig(target_lufs=-16.0))[0] for l in measured["loudness"]], np.float32)
    limited = eng.limit(marked["wav_list"], gains=gains, ceiling_dbtp=-1.0)
    delivered = eng.deliver(limited["wav_list"], DeliveryConfig(8000, "ulaw"))["delivered_list"]
    assert np.array_equal(out["watermark"]["lens_out"], marked["lens_out"]) and out["watermark"]["lens_out"].tolist() == [w.size // 256 * 256 for w in st["wav_list"]]
    assert out["watermark"]["payload"].tolist() == [0x11, 0x2] and out["watermark"]["key"] == KEY
    for b, (g, w) in enumerate(zip(out["delivered_list"], delivered)):
        assert g.dtype == w.dtype == np.uint8 and g.tobytes() == w.tobytes(), b
    assert out["loudness"]["loudness"].tobytes() == measured["loudness"].tobytes() and out["limiter"]["min_gain"].tobytes() == limited["min_gain"].tobytes()
    only = eng.synthesize(utts, watermark=KEY)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(only["wav_list"], eng.watermark(plain["wav_list"], KEY)["wav_list"]))
    again = eng.synthesize(utts)
    assert set(again) == set(plain) and all(a.tobytes() == p.tobytes() for a, p in zip(again["wav_list"], plain["wav_list"]))


def test_the_delivered_8_khz_bytes_still_carry_the_mark(ctx):
    """The waveform stages of the chain on the two fixtures, as the device runs them (the test above holds synthesize to this composition):
    ev_watermark -> ev_loudness -> ev_limit -> ev_deliver to 8 kHz mu-law; the bytes decoded on the host as a telephone endpoint would, then
    watermark_detect(sample_rate=8000), which brings them back to 16 kHz with ev_resample."""
    from emotivoice_amd.delivery import DeliveryConfig
    from emotivoice_amd.limiter import pre_gain
    from emotivoice_amd.loudness import LoudnessConfig
    eng = ctx["eng"]
    wavs = [ctx["speech"], ctx["rich"]]
    heard = {}
    for tag, src in (("marked", eng.watermark(wavs, _cfg())["wav_list"]), ("plain", wavs)):
        measured = eng.loudness(src)
        gains = np.array([pre_gain(float(l), LoudnessConfig(target_lufs=-16.0))[0] for l in measured["loudness"]], np.float32)
        limited = eng.limit(src, gains=gains, ceiling_dbtp=-1.0)
        law = eng.deliver(limited["wav_list"], DeliveryConfig(8000, "ulaw"))["delivered_list"]
        assert all(b.dtype == np.uint8 and b.size == 2 * SR for b in law)
        heard[tag] = eng.watermark_detect([wo.ulaw_decode(b) for b in law], KEY, sample_rate=8000)["report"]
    print({k: [(round(r["z"], 2), r["offset"]) for r in v] for k, v in heard.items()})
    assert all(r["present"] and r["offset"] == 0 for r in heard["marked"]) and not any(r["present"] for r in heard["plain"])
