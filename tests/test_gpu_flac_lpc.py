"""MI355X: ev_flac_lpc -- LPC subframes and the MD5 signature on the device (include/evhip.h).  Every byte and every decision against the numpy
restatement (tests/flac_lpc_oracle.py); the analysis' integers through ev_op_flac_lpc; the digests against hashlib; invariance; the identity
with ev_flac; rejections; synthesize / synthesize_long with a FlacConfig, through the oracle's own decoder."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import flac_lpc_oracle as lo
import flac_oracle as fo

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


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
    sig = lo.signal_set()
    yield dict(eng=eng, names=list(sig), signals=list(sig.values()))
    eng.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _ext(**kw):
    from emotivoice_amd import _ffi
    e = _ffi.ev_flac_ext()
    _ffi.lib().ev_default_flac_ext(C.byref(e))
    for k, v in kw.items():
        setattr(e, k, v)
    return e


@pytest.mark.parametrize("N", lo.BLOCKS)
@pytest.mark.parametrize("L,q", lo.CONFIGS)
def test_streams_and_decisions_equal_the_oracle(ctx, N, L, q):
    """The signal set in one batch: streams, frame_kind and frame_porder byte for byte; every stream decodes to its input and verifies its MD5."""
    eng, signals = ctx["eng"], ctx["signals"]
    out = eng.flac(signals, block_size=N, max_lpc_order=L, qlp_precision=q, md5=True)
    assert len(out["streams"]) == len(signals)
    for b, x in enumerate(signals):
        info = {}
        want = lo.encode(x, block_size=N, max_lpc_order=L, qlp_precision=q, md5=True, info=info)
        got = out["streams"][b]
        if got != want:
            n = min(len(got), len(want))
            first = next((i for i in range(n) if got[i] != want[i]), n)
            raise AssertionError("%s (%d samples): %d bytes, oracle %d, first difference at byte %d; kinds %s / %s" % (
                ctx["names"][b], x.size, len(got), len(want), first, out["frame_kind"][b].tolist(), info["frame_kind"].tolist()))
        assert np.array_equal(out["frame_kind"][b], info["frame_kind"]) and np.array_equal(out["frame_porder"][b], info["frame_porder"]), b
        dinfo = {}
        assert np.array_equal(lo.decode(got, dinfo), x) and dinfo["md5_checked"], b
        assert len(got) <= eng._lib.ev_flac_bound(x.size, N), b
    kinds = np.concatenate(out["frame_kind"])
    assert (kinds >= 32).any() and kinds.max() <= 32 + L - 1
    assert out["total_bytes"] == sum(len(s) for s in out["streams"]) == out["stream_offsets"][-1] == out["frame_offsets"][-1]


@pytest.mark.parametrize("N,L,q", [(256, 12, 12), (4096, 12, 5), (4096, 8, 15)])
def test_analysis_integers_equal_the_oracle(ctx, N, L, q):
    """ev_op_flac_lpc: R[0 .. 12], the shifts and the quantised coefficients of every frame, exactly."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.flac import FlacConfig
    lib = _ffi.lib()
    signals = ctx["signals"]
    lens = np.array([s.size for s in signals], np.int64)
    nf = int(sum(-(-s.size // N) for s in signals))
    d_pcm = torch.from_numpy(np.concatenate(signals)).cuda()
    torch.cuda.synchronize()
    R, shift, coef = np.full((nf, 13), -7, np.int64), np.full((nf, 12), -7, np.int32), np.full((nf, 12, 12), -7, np.int32)
    cfg = FlacConfig(block_size=N).to_struct()
    assert lib.ev_op_flac_lpc(d_pcm.data_ptr(), 1, len(signals), _p(lens), C.byref(cfg), L, q, _p(R), _p(shift), _p(coef), None) == 0
    f = 0
    for b, x in enumerate(signals):
        for lo_ in range(0, x.size, N):
            wR, wS, wC = lo.analyse(x[lo_:lo_ + N], L, q)
            assert np.array_equal(R[f], wR), (ctx["names"][b], lo_, R[f].tolist(), wR.tolist())
            assert np.array_equal(shift[f], wS), (ctx["names"][b], lo_, shift[f].tolist(), wS.tolist())
            assert np.array_equal(coef[f], wC), (ctx["names"][b], lo_)
            f += 1
    assert f == nf
    assert lib.ev_op_flac_lpc(d_pcm.data_ptr(), 1, len(signals), _p(lens), C.byref(cfg), 13, q, _p(R), _p(shift), _p(coef), None) == -2
    assert lib.ev_op_flac_lpc(d_pcm.data_ptr(), 1, len(signals), _p(lens), C.byref(cfg), L, 4, _p(R), _p(shift), _p(coef), None) == -2


def test_md5_equals_hashlib(ctx):
    """Segments of very different lengths in one call, the padding edges (sample bytes of 0, 2, 54, 56, 62 mod 64) and more than one chunk of 64
    rounds; int16, and fp32 under both conversions."""
    eng = ctx["eng"]
    rng = np.random.default_rng(3)
    lens = [1, 27, 28, 31, 32, 33, 59, 60, 63, 64, 2047, 2048, 2049, 4096 + 27, 4096 + 28, 40001]
    segs = [rng.integers(-32768, 32768, n).astype(np.int16) for n in lens]
    for cfg in (dict(max_lpc_order=0), dict(max_lpc_order=8)):
        out = eng.flac(segs, md5=True, **cfg)
        for b, x in enumerate(segs):
            assert out["streams"][b][26:42] == hashlib.md5(x.astype("<i2").tobytes()).digest(), (cfg, lens[b])
    plain = eng.flac(segs)
    assert all(plain["streams"][b][:26] + out0[26:42] + plain["streams"][b][42:] == out0 for b, out0 in enumerate(eng.flac(segs, md5=True)["streams"]))
    y = [(rng.standard_normal(n) * 0.9).astype(np.float32) for n in (5000, 77, 1)]
    y[0][[5, 50, 500]] = [np.nan, np.inf, -np.inf]
    for convert, rule in (("wrap", 0), ("clamp", 1)):
        out = eng.flac(y, md5=True, max_lpc_order=4, convert=convert)
        for b, v in enumerate(y):
            assert out["streams"][b][26:42] == hashlib.md5(fo.to_i16(v, rule).astype("<i2").tobytes()).digest(), (convert, b)


def test_invariance_and_identity(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.flac import FlacConfig
    eng = ctx["eng"]
    lib = _ffi.lib()
    sig = dict(zip(ctx["names"], ctx["signals"]))
    x, a, b = sig["sines5"][:6001].copy(), sig["ar8"][:777].copy(), sig["voiced"][5000:9100].copy()
    kw = dict(max_lpc_order=12, md5=True)
    alone = eng.flac([x], **kw)["streams"][0]
    assert alone == lo.encode(x, max_lpc_order=12, md5=True)
    assert eng.flac([x, a, b], **kw)["streams"][0] == alone and eng.flac([a, b, x], **kw)["streams"][2] == alone
    xf = x.astype(np.float32) / np.float32(32768.0)
    assert np.array_equal(fo.to_i16(xf, 0), x)
    assert eng.flac([xf], **kw)["streams"][0] == alone and eng.flac([xf], convert="clamp", **kw)["streams"][0] == alone
    d16 = torch.from_numpy(np.concatenate([np.full(3, 77, np.int16), x])).cuda()
    d32 = torch.from_numpy(np.concatenate([np.full(1, 9.0, np.float32), xf])).cuda()
    torch.cuda.synchronize()
    fc = FlacConfig(**kw)
    r = eng.flac_raw(1, d16.data_ptr() + 2 * 3, True, np.array([x.size]), fc, _ffi.EV_FLAG_DEVICE_INPUTS)
    assert eng.flac_to_numpy(r)["streams"][0] == alone
    r = eng.flac_raw(1, d32.data_ptr() + 4, False, np.array([x.size]), fc, _ffi.EV_FLAG_DEVICE_INPUTS)
    assert eng.flac_to_numpy(r)["streams"][0] == alone
    # identity: ext NULL and the all-off ext are ev_flac
    segs = [x, a, b, sig["noise_full"], sig["zeros"][:33]]
    today = eng.flac(segs)["streams"]
    flat, lens = np.concatenate(segs), np.array([s.size for s in segs], np.int64)
    for ext in (None, _ext(max_lpc_order=0, md5=0), _ext(max_lpc_order=0, md5=0, qlp_precision=7)):
        res = _ffi.ev_flac_result()
        res.struct_size = C.sizeof(res)
        assert lib.ev_flac_lpc(eng._h, len(segs), _p(flat), 1, _p(lens), None, None if ext is None else C.byref(ext), 0, C.byref(res)) == 0
        assert eng.flac_to_numpy(res)["streams"] == today


def test_rejections_leave_the_previous_result(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.flac import FlacConfig
    eng = ctx["eng"]
    lib = _ffi.lib()
    x = ctx["signals"][ctx["names"].index("ar4")][:4096].copy()
    lens = np.array([3000, 1096], np.int64)
    keep = eng.flac_raw(2, x.ctypes.data, True, lens, FlacConfig(max_lpc_order=8, md5=True))
    want = eng.flac_to_numpy(keep)
    assert want["streams"] == [lo.encode(x[:3000], max_lpc_order=8, md5=True), lo.encode(x[3000:], max_lpc_order=8, md5=True)]
    bad_reserved = _ext()
    bad_reserved.reserved[2] = 1
    checks = [(_ext(max_lpc_order=13), "max_lpc_order"), (_ext(max_lpc_order=-1), "max_lpc_order"), (_ext(qlp_precision=4), "qlp_precision"),
              (_ext(qlp_precision=16), "qlp_precision"), (_ext(md5=2), "md5"), (bad_reserved, "reserved[2]"), (_ext(struct_size=28), "struct_size")]
    for ext, needle in checks:
        res = _ffi.ev_flac_result()
        res.struct_size = C.sizeof(res)
        rc = lib.ev_flac_lpc(eng._h, 2, _p(x), 1, _p(lens), None, C.byref(ext), 0, C.byref(res))
        msg = lib.ev_last_error(eng._h).decode()
        assert rc < 0 and needle in msg and "ev_flac_lpc" in msg, (needle, msg)
        assert eng.flac_to_numpy(keep)["streams"] == want["streams"], needle
    res = _ffi.ev_flac_result()
    res.struct_size = C.sizeof(res)
    assert lib.ev_flac_lpc(eng._h, 2, _p(x), 1, _p(np.array([3000, 0], np.int64)), None, C.byref(_ext()), 0, C.byref(res)) < 0
    assert "lens[1]" in lib.ev_last_error(eng._h).decode()
    assert eng.flac_to_numpy(keep)["streams"] == want["streams"]


def test_synthesize_and_synthesize_long_with_a_flac_config(ctx):
    from emotivoice_amd.flac import FlacConfig
    from emotivoice_amd.longform import StitchConfig
    from emotivoice_amd.synthetic import synth_inputs
    from emotivoice_amd.text_io import wav_float_to_int16
    eng = ctx["eng"]
    fc = FlacConfig(max_lpc_order=8, md5=True, sample_rate=48000)      # the sample rate is the engine's, whatever the config says
    utts = synth_inputs(51, [24, 11, 17, 9, 20], [3, 3, 3, 8, 8])
    out = eng.synthesize(utts, flac=fc)
    for b in range(5):
        info = {}
        pcm = lo.decode(out["flac_list"][b], info)
        assert np.array_equal(pcm, wav_float_to_int16(out["wav_list"][b])) and info["sample_rate"] == 16000 and info["md5_checked"], b
        assert out["flac_list"][b] == lo.encode(pcm, max_lpc_order=8, md5=True), b
    staged = eng.synthesize(utts, flac=fc, loudness=-23.0, limiter=True)
    for b in range(5):
        info = {}
        assert np.array_equal(lo.decode(staged["flac_list"][b], info), staged["wav_int16_list"][b]) and info["md5_checked"], b
    assert "limiter" in staged and any(staged["flac_list"][b] != out["flac_list"][b] for b in range(5))
    documents = [dict(utts=utts[:3], pauses=["comma", -4.0]), (utts[3:], ["sentence"])]
    long = eng.synthesize_long(documents, config=StitchConfig(lead_ms=20.0, tail_ms=50.0), flac=fc)
    today = eng.synthesize_long(documents, config=StitchConfig(lead_ms=20.0, tail_ms=50.0), flac=True)
    for d in range(2):
        info = {}
        assert np.array_equal(lo.decode(long["flac_list"][d], info), long["documents"][d]) and info["md5_checked"], d
        assert long["documents"][d].dtype == np.int16 and np.array_equal(long["documents"][d], today["documents"][d]), d
        assert fo.decode(today["flac_list"][d]).tobytes() == long["documents"][d].tobytes() and today["flac_list"][d][26:42] == bytes(16), d
        assert len(long["flac_list"][d]) <= len(today["flac_list"][d]), d
