"""MI355X: ev_flac -- packed PCM -> FLAC streams on the device (include/evhip.h).  Every byte and every decision against the numpy oracle
(tests/flac_oracle.py) at the edges of the order limit, the partition rule, the last-block fields and the frame-number coding; invariance;
rejections and lifetime; synthesize(..., flac=True) and synthesize_long(..., flac=True) end to end through the oracle's independent decoder."""
import ctypes as C

import numpy as np
import pytest

import flac_oracle as fo

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EDGE_LENGTHS = (1, 2, 3, 4, 5, 17, 100, 255, 256, 257, 4095, 4096, 4097, 8192)


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
    yield dict(eng=eng, voiced=fo.voiced(16384))
    eng.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _check(out, signals, **cfg):
    """The device's streams and decisions against the oracle's, segment by segment."""
    assert len(out["streams"]) == len(signals)
    for b, x in enumerate(signals):
        info = {}
        want = fo.encode(x, info=info, **cfg)
        got = out["streams"][b]
        if got != want:
            n = min(len(got), len(want))
            first = next((i for i in range(n) if got[i] != want[i]), n)
            raise AssertionError("segment %d (%d samples): %d bytes, oracle %d, first difference at byte %d; kinds %s / %s" % (
                b, x.size, len(got), len(want), first, out["frame_kind"][b].tolist(), info["frame_kind"].tolist()))
        assert np.array_equal(out["frame_kind"][b], info["frame_kind"]) and np.array_equal(out["frame_porder"][b], info["frame_porder"]), b
    assert out["total_bytes"] == sum(len(s) for s in out["streams"]) == out["stream_offsets"][-1] == out["frame_offsets"][-1]


def test_streams_and_decisions_equal_the_oracle(ctx):
    """One batch: the signal set (every subframe kind, partition orders 0 .. 5) and cuts of the voiced signal at the edges of o < n, of the
    partition rule, of the 8- and 16-bit last-block fields and of a last block of one sample."""
    eng, v = ctx["eng"], ctx["voiced"]
    signals = list(fo.signal_set().values()) + [v[3000:3000 + n].copy() for n in EDGE_LENGTHS]
    out = eng.flac(signals)
    _check(out, signals)
    kinds = set(np.concatenate(out["frame_kind"]).tolist())
    assert kinds == {0, 1, 8, 9, 10, 11, 12}
    assert set(np.concatenate(out["frame_porder"]).tolist()) >= {0, 1, 2, 3, 4, 5}
    for b, x in enumerate(signals):
        assert np.array_equal(fo.decode(out["streams"][b]), x), b
        assert len(out["streams"][b]) <= eng._lib.ev_flac_bound(x.size, 4096), b
    assert np.array_equal(out["stream_frames"], [-(-x.size // 4096) for x in signals])


@pytest.mark.parametrize("frames,extra,mfo,mpo", [(300, 7, 4, 5), (2049, 0, 2, 2)])
def test_frame_numbers_beyond_one_byte(ctx, frames, extra, mfo, mpo):
    """Block size 256: 301 frames need two-byte frame numbers, 2049 frames three-byte ones."""
    eng = ctx["eng"]
    x = np.resize(ctx["voiced"], frames * 256 + extra)
    cfg = dict(block_size=256, max_fixed_order=mfo, max_partition_order=mpo)
    out = eng.flac([x], **cfg)
    _check(out, [x], **cfg)
    assert out["stream_frames"].tolist() == [frames + (1 if extra else 0)]


@pytest.mark.parametrize("cfg", [dict(block_size=256), dict(block_size=512, sample_rate=22050), dict(block_size=1024, max_partition_order=6),
                                 dict(block_size=2048, sample_rate=48000), dict(block_size=4096, max_partition_order=6),
                                 dict(max_fixed_order=0), dict(max_partition_order=0), dict(max_fixed_order=0, max_partition_order=0)])
def test_block_sizes_and_order_limits(ctx, cfg):
    eng = ctx["eng"]
    x = ctx["voiced"][:9001]
    out = eng.flac([x, x[:4096 - 64]], **cfg)
    _check(out, [x, x[:4096 - 64]], **cfg)
    fixed = np.concatenate(out["frame_kind"]) >= 8
    assert (np.concatenate(out["frame_kind"])[fixed] - 8 <= cfg.get("max_fixed_order", 4)).all()
    assert (np.concatenate(out["frame_porder"]) <= cfg.get("max_partition_order", 5)).all()


def test_invariance(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.flac import FlacConfig
    eng, v = ctx["eng"], ctx["voiced"]
    rng = np.random.default_rng(5)
    x = v[100:100 + 6001].copy()
    alone = eng.flac([x])["streams"][0]
    assert alone == fo.encode(x)
    # in the middle of a batch
    batch = eng.flac([v[:777].copy(), x, v[5000:9100].copy()])
    assert batch["streams"][1] == alone
    # the fp32 that converts to it, from the host
    xf = (x.astype(np.float32) / np.float32(32768.0))
    assert np.array_equal(fo.to_i16(xf, 0), x)
    assert eng.flac([xf])["streams"][0] == alone and eng.flac([xf], convert="clamp")["streams"][0] == alone
    # device input: int16 at an odd element offset, fp32 segments none of which starts 16-byte aligned
    d16 = torch.from_numpy(np.concatenate([np.full(3, 77, np.int16), x])).cuda()
    segs = [xf[:1001], xf[1001:1004], xf[1004:]]
    flat = np.concatenate([np.full(1, 9.0, np.float32)] + segs)
    d32 = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    assert d32.data_ptr() % 16 == 0 and all((4 * (1 + o)) % 16 for o in (0, 1001, 1004))
    r = eng.flac_raw(1, d16.data_ptr() + 2 * 3, True, np.array([x.size]), None, _ffi.EV_FLAG_DEVICE_INPUTS)
    assert eng.flac_to_numpy(r)["streams"][0] == alone
    r = eng.flac_raw(3, d32.data_ptr() + 4, False, np.array([s.size for s in segs]), FlacConfig(), _ffi.EV_FLAG_DEVICE_INPUTS)
    dev = eng.flac_to_numpy(r)
    host = eng.flac(segs)
    assert dev["streams"] == host["streams"] and dev["streams"] == [fo.encode(fo.to_i16(s, 0)) for s in segs]
    # wrap against clamp on a signal that leaves [-1, 1), with NaN, infinities and +-0 in it
    y = (rng.standard_normal(5000) * 0.9).astype(np.float32)
    y[[5, 50, 500, 501]] = [np.nan, np.inf, -np.inf, -0.0]
    assert (np.abs(y[np.isfinite(y)]) > 1.0).sum() > 100
    wrap, clamp = eng.flac([y], convert="wrap"), eng.flac([y], convert="clamp")
    assert wrap["streams"][0] == fo.encode(fo.to_i16(y, 0)) and clamp["streams"][0] == fo.encode(fo.to_i16(y, 1))
    assert wrap["streams"][0] != clamp["streams"][0]
    assert np.array_equal(fo.decode(wrap["streams"][0]), fo.to_i16(y, 0)) and np.array_equal(fo.decode(clamp["streams"][0]), fo.to_i16(y, 1))


def test_rejections_leave_the_previous_result_and_it_survives_a_synthesis(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.flac import FlacConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    lib = _ffi.lib()
    x = ctx["voiced"][:5000].copy()
    keep = eng.flac_raw(2, x.ctypes.data, True, np.array([3000, 2000]))
    want = eng.flac_to_numpy(keep)
    assert want["streams"] == [fo.encode(x[:3000]), fo.encode(x[3000:])]

    def run(B=2, pcm=x, lens=(3000, 2000), size=None, out=True, **cfg_kw):
        c = FlacConfig().to_struct()
        for k, val in cfg_kw.items():
            setattr(c, k, val)
        r = _ffi.ev_flac_result()
        r.struct_size = C.sizeof(r) if size is None else size
        ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
        rc = lib.ev_flac(eng._h, B, None if pcm is None else _p(pcm), 1, None if ln is None else _p(ln), C.byref(c), 0, C.byref(r) if out else None)
        return rc, lib.ev_last_error(eng._h).decode()

    checks = [(dict(pcm=None), "pcm"), (dict(lens=None), "lens"), (dict(out=False), "out"), (dict(size=24), "struct_size"), (dict(struct_size=20), "struct_size"),
              (dict(B=0, lens=()), "B = 0"), (dict(B=65536, lens=[1] * 65536), "B = 65536"), (dict(lens=(3000, 0)), "lens[1]"), (dict(lens=(-5, 2000)), "lens[0]"),
              (dict(lens=(3000, (1 << 30) + 1)), "lens[1]"), (dict(sample_rate=11025), "sample_rate"), (dict(sample_rate=0), "sample_rate"),
              (dict(block_size=192), "block_size"), (dict(block_size=8192), "block_size"), (dict(max_fixed_order=5), "max_fixed_order"),
              (dict(max_fixed_order=-1), "max_fixed_order"), (dict(max_partition_order=7), "max_partition_order"), (dict(max_partition_order=-1), "max_partition_order"),
              (dict(convert=2), "convert"), (dict(convert=-1), "convert")]
    for kw, needle in checks:
        rc, msg = run(**kw)
        assert rc < 0 and needle in msg, (kw, msg)
        assert eng.flac_to_numpy(keep)["streams"] == want["streams"], kw      # the previous result, untouched
    assert lib.ev_flac(None, 2, _p(x), 1, _p(np.array([3000, 2000], np.int64)), None, 0, C.byref(_ffi.ev_flac_result())) < 0
    syn = eng.synthesize(synth_inputs(9, [20]))
    eng.features([x.astype(np.float32) / 32768.0])
    after = eng.flac_to_numpy(keep)
    assert after["streams"] == want["streams"] and np.isfinite(syn["wav"]).all()
    assert all(np.array_equal(a, b) for a, b in zip(after["frame_kind"], want["frame_kind"]))
    with pytest.raises(ValueError, match="entries"):
        eng.flac_raw(2, x.ctypes.data, True, np.array([5000]))
    assert eng.flac_to_numpy(eng.flac_raw(1, x.ctypes.data, True, np.array([5000])))["streams"] == [fo.encode(x)]      # a good call after them


def test_synthesize_and_synthesize_long_with_flac(ctx):
    from emotivoice_amd.longform import StitchConfig
    from emotivoice_amd.synthetic import synth_inputs
    from emotivoice_amd.text_io import wav_float_to_int16
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 11, 17, 9, 20], [3, 3, 3, 8, 8])
    plain = eng.synthesize(utts)
    assert "flac_list" not in plain
    out = eng.synthesize(utts, flac=True)
    assert np.array_equal(out["wav"].view(np.uint32), plain["wav"].view(np.uint32))
    for b in range(5):
        info = {}
        pcm = fo.decode(out["flac_list"][b], info)
        assert np.array_equal(pcm, wav_float_to_int16(out["wav_list"][b])) and info["sample_rate"] == 16000, b
        assert out["flac_list"][b] == fo.encode(fo.to_i16(out["wav_list"][b], 0)), b
    mask = [False, True, True, False, True]
    part = eng.synthesize(utts, flac=mask)
    assert [f is not None for f in part["flac_list"]] == mask
    assert all(part["flac_list"][b] == out["flac_list"][b] for b in range(5) if mask[b])
    with pytest.raises(ValueError, match="vocoder"):
        eng.synthesize(utts, flac=True, vocoder=False)
    documents = [dict(utts=utts[:3], pauses=["comma", -4.0]), (utts[3:], ["sentence"])]
    cfg = StitchConfig(lead_ms=20.0, tail_ms=50.0)
    ref = eng.synthesize_long(documents, config=StitchConfig(lead_ms=20.0, tail_ms=50.0, want_int16=True))
    long = eng.synthesize_long(documents, config=cfg, flac=True)
    assert len(long["flac_list"]) == 2 and "flac_list" not in ref
    for d in range(2):
        assert long["documents"][d].dtype == np.int16 and np.array_equal(long["documents"][d], ref["documents"][d]), d
        assert np.array_equal(fo.decode(long["flac_list"][d]), ref["documents"][d]), d


def test_encode_op_writes_its_frames_and_nothing_else(ctx):
    """ev_op_flac_encode on a guard-banded slot buffer: every slot starts with the oracle's frame, and no byte beyond a frame's size rounded up to
    four -- in its slot, in front of the first slot or behind the last one -- is written.  Full, short, one-sample and VERBATIM frames."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.flac import FlacConfig
    lib = _ffi.lib()
    v = ctx["voiced"]
    sig = fo.signal_set()
    GUARD, FILL = 64, 0xA5
    for N, segs in ((4096, [v[:4097].copy(), sig["noise_full"][:4096], sig["zeros"][:33]]), (256, [v[:513].copy(), sig["alternation"][:255], v[:3].copy()])):
        stride = 2 * N + 24
        lens = np.array([s.size for s in segs], np.int64)
        nf = int(sum(-(-s.size // N) for s in segs))
        d_pcm = torch.from_numpy(np.concatenate(segs)).cuda()
        d_slots = torch.full((GUARD + nf * stride + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sizes, kind, porder = np.zeros(nf, np.int32), np.zeros(nf, np.uint8), np.zeros(nf, np.uint8)
        cfg = FlacConfig(block_size=N).to_struct()
        rc = lib.ev_op_flac_encode(d_pcm.data_ptr(), 1, len(segs), _p(lens), C.byref(cfg), d_slots.data_ptr() + GUARD, _p(sizes), _p(kind), _p(porder), None)
        assert rc == 0
        got = d_slots.cpu().numpy()
        assert (got[:GUARD] == FILL).all() and (got[-GUARD:] == FILL).all()
        f = 0
        for x in segs:
            info = {}
            stream = fo.encode(x, block_size=N, info=info)
            pos = 42
            for i, sz in enumerate(info["frame_sizes"].tolist()):
                slot = got[GUARD + f * stride:GUARD + (f + 1) * stride]
                assert sizes[f] == sz and kind[f] == info["frame_kind"][i] and porder[f] == info["frame_porder"][i], (N, f)
                assert slot[:sz].tobytes() == stream[pos:pos + sz], (N, f)
                assert (slot[(sz + 3) // 4 * 4:] == FILL).all(), (N, f)
                pos += sz
                f += 1
        assert f == nf and 1 in kind and 0 in kind
        assert lib.ev_op_flac_encode(d_pcm.data_ptr(), 1, len(segs), _p(lens), C.byref(cfg), d_slots.data_ptr() + GUARD + 1, _p(sizes), _p(kind), _p(porder), None) == -2
        bad = FlacConfig(block_size=N).to_struct()
        bad.block_size = 300
        assert lib.ev_op_flac_encode(d_pcm.data_ptr(), 1, len(segs), _p(lens), C.byref(bad), d_slots.data_ptr() + GUARD, _p(sizes), _p(kind), _p(porder), None) == -2
