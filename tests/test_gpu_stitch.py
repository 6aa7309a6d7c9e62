"""MI355X: ev_stitch -- the sentences of one batch -> finished documents on the device (include/evhip.h).  The scan and the mix kernels at their
edges against the numpy oracle (tests/stitch_oracle.py) on guard-banded buffers, bit invariance, rejections, lifetime, and synthesize_long end
to end.  The bit-exact comparisons use the ramp table the device holds (ev_get_stage("stitch_ramp"))."""
import ctypes as C

import numpy as np
import pytest

import stitch_oracle as so

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 256


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
    yield dict(eng=eng, tabs={})
    eng.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _table(ctx, F):
    """The F ramp values the device holds after an ev_stitch call with fade = F."""
    if F not in ctx["tabs"]:
        eng = ctx["eng"]
        eng.stitch([np.ones(3, np.float32)], [0], [None], trim_frac=0.0, fade=F, keep=0)
        n = eng._lib.ev_get_stage(eng._h, b"stitch_ramp", None, 0)
        assert n == 4 * F, eng._lib.ev_last_error(eng._h)
        tab = np.zeros(F, np.float32)
        assert eng._lib.ev_get_stage(eng._h, b"stitch_ramp", _p(tab), tab.nbytes) == n
        want = so.ramp_table(F)
        if F:
            assert (np.abs(tab.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want)).all()
        ctx["tabs"][F] = tab
    return ctx["tabs"][F]


def _scan_op(segs, frac, abs_thr):
    """ev_op_stitch_scan on segments laid out with unequal gaps between them (filled with a value above every threshold)."""
    from emotivoice_amd import _ffi
    S = len(segs)
    parts, offs, o = [], [], 0
    for s, x in enumerate(segs):
        gap = np.full(3 + 5 * (s % 4), 9.0, np.float32)
        parts += [gap, np.asarray(x, np.float32)]
        offs.append(o + gap.size)
        o += gap.size + len(x)
    parts.append(np.full(7, 9.0, np.float32))
    d_wav = torch.from_numpy(np.concatenate(parts)).cuda()
    torch.cuda.synchronize()
    offs, lens = np.array(offs, np.int64), np.array([len(x) for x in segs], np.int64)
    peak, first, last = np.full(S, -3.0, np.float32), np.full(S, -5, np.int64), np.full(S, -5, np.int64)
    rc = _ffi.lib().ev_op_stitch_scan(d_wav.data_ptr(), S, _p(offs), _p(lens), frac, abs_thr, _p(peak), _p(first), _p(last), None)
    assert rc == 0
    return peak, first, last


def _mix_op(cuts, seg_doc, pos, fl, fr, doc_lens, tab, want_i16=True):
    """ev_op_stitch_mix between guard bands of NaN (fp32) and of 12345 (int16): the documents, and nothing written outside them."""
    from emotivoice_amd import _ffi
    S, D, total = len(cuts), len(doc_lens), int(np.sum(doc_lens))
    n = np.array([len(c) for c in cuts], np.int64)
    src = (np.concatenate([[0], np.cumsum(n)[:-1]]) + 5).astype(np.int64)
    flat = np.concatenate([np.full(5, np.nan, np.float32)] + [np.asarray(c, np.float32) for c in cuts] + [np.full(5, np.nan, np.float32)])
    d_wav = torch.from_numpy(flat).cuda()
    d_out = torch.full((total + 2 * GUARD,), float("nan"), device="cuda")
    d_i16 = torch.full((total + 2 * GUARD,), 12345, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    sd = np.ascontiguousarray(seg_doc, np.int32)
    tab = np.ascontiguousarray(tab, np.float32)
    rc = _ffi.lib().ev_op_stitch_mix(d_wav.data_ptr(), S, _p(src), _p(n), _p(sd), _p(np.ascontiguousarray(pos, np.int64)), _p(np.ascontiguousarray(fl, np.int32)),
                                     _p(np.ascontiguousarray(fr, np.int32)), _p(tab) if tab.size else None, tab.size, D, _p(np.ascontiguousarray(doc_lens, np.int64)),
                                     d_out.data_ptr() + 4 * GUARD, d_i16.data_ptr() + 2 * GUARD if want_i16 else None, None)
    assert rc == 0
    out, i16 = d_out.cpu().numpy(), d_i16.cpu().numpy()
    assert np.isnan(out[:GUARD]).all() and np.isnan(out[GUARD + total:]).all() and not np.isnan(out[GUARD:GUARD + total]).any()
    assert (i16[:GUARD] == 12345).all() and (i16[GUARD + total:] == 12345).all()
    if not want_i16:
        assert (i16 == 12345).all()
    offs = np.concatenate([[0], np.cumsum(doc_lens)]).astype(np.int64) + GUARD
    return [out[offs[d]:offs[d + 1]] for d in range(D)], [i16[offs[d]:offs[d + 1]] for d in range(D)]


def _check_mix(ctx, name, lens, seg_doc, pause, F, lead=0, tail=0, amp=0.7, seed=0, want_i16=True):
    rng = np.random.default_rng(seed)
    tab = _table(ctx, F)
    cuts = [(amp * rng.standard_normal(L)).astype(np.float32) for L in lens]
    pos, fl, fr, doc_lens = so.plan(lens, seg_doc, pause, F, lead, tail)
    want, cover = so.mix(cuts, seg_doc, pos, fl, fr, doc_lens, tab)
    got, got16 = _mix_op(cuts, seg_doc, pos, fl, fr, doc_lens, tab, want_i16)
    for d in range(len(doc_lens)):
        assert np.array_equal(_bits(got[d]), _bits(want[d])), (name, d)
        if want_i16:
            assert np.array_equal(got16[d], so.to_i16(want[d])), (name, d)
    return want, cover, pos, doc_lens


def test_op_scan_at_its_edges():
    """Lengths around the 1024- and 4096-sample chunks; a hit at index 0, at the last index, on both sides of a chunk border from the front and
    from the back; the first hit in the third chunk (the early exit) and the last hit three chunks from the end; all zeros; trim_abs above the
    peak; samples exactly at the threshold (no hit) and equal maxima of either sign."""
    rng = np.random.default_rng(5)
    segs = [(0.5 * rng.standard_normal(L)).astype(np.float32) for L in (1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 9000)]

    def quiet(L, hits, level=0.9):
        x = (1e-4 * rng.uniform(-1, 1, L)).astype(np.float32)
        for i in hits:
            x[i] = level if i % 2 == 0 else -level
        return x
    segs += [quiet(4097, [0]), quiet(4097, [4096]), quiet(4097, [0, 4096]), quiet(4097, [1023, 3072]), quiet(4097, [1024, 3073]), quiet(4097, [1024, 3072]),
             quiet(9000, [2048 + 77, 9000 - 2048 - 77]), quiet(9000, [3000]), np.zeros(1300, np.float32), np.zeros(1, np.float32)]
    ties = np.full(2500, 0.25, np.float32)          # peak 1.0, frac 0.25: 0.25 is the threshold itself, the next float above it is a hit
    ties[[700, 1900]] = [1.0, -1.0]
    ties[[300, 2200]] = np.nextafter(np.float32(0.25), np.float32(1.0))
    ties[1100] = -0.25
    segs.append(ties)
    for frac, abs_thr in ((0.25, 0.0), (0.005, 0.0), (0.0, 0.05), (0.25, 0.3), (0.0, 5.0), (0.0, 0.0)):
        peak, first, last = _scan_op(segs, frac, abs_thr)
        for s, x in enumerate(segs):
            w_peak, w_first, w_last = so.scan(x, frac, abs_thr)
            assert (peak[s].view(np.uint32), first[s], last[s]) == (np.float32(w_peak).view(np.uint32), w_first, w_last), (frac, abs_thr, s, len(x))
    peak, first, last = _scan_op(segs, 0.25, 0.0)
    assert (first[9], last[9]) == (0, 0) and (first[10], last[10]) == (4096, 4096) and (first[12], last[12]) == (1023, 3072) and (first[13], last[13]) == (1024, 3073)
    assert (first[15], last[15]) == (2125, 6875) and (first[17], last[17]) == (-1, -1) and (first[19], last[19]) == (300, 2200) and peak[19] == 1.0
    assert (_scan_op(segs, 0.0, 5.0)[1] == -1).all()          # trim_abs above every peak
    from emotivoice_amd import _ffi
    d = torch.zeros(64, device="cuda")
    one, z = np.array([8], np.int64), np.zeros(1, np.int64)
    pk, f, l = np.zeros(1, np.float32), np.zeros(1, np.int64), np.zeros(1, np.int64)
    lib = _ffi.lib()
    for lens, offs, frac, abs_thr, S in ((z, z, 0.1, 0.0, 1), (one, z - 1, 0.1, 0.0, 1), (one, z, 1.0, 0.0, 1), (one, z, float("nan"), 0.0, 1), (one, z, 0.1, -1.0, 1),
                                         (one, z, 0.1, 0.0, 0)):
        assert lib.ev_op_stitch_scan(d.data_ptr(), S, _p(offs), _p(lens), frac, abs_thr, _p(pk), _p(f), _p(l), None) == -2


def test_op_mix_at_its_edges(ctx):
    """Bit-equal to the oracle between NaN guard bands, fp32 and int16."""
    # every fade length with room for it, a cross-fade of exactly F, a pause and a shorter overlap
    for F in (0, 1, 64, 4096):
        L = 2 * F + 300
        want, cover, pos, doc_lens = _check_mix(ctx, "F%d" % F, [L, L + 17, L + 5, 2 * F + 1], [0, 0, 0, 0], [-F, 40, -(F // 2 + 1), 0], F, lead=3, tail=2, seed=F)
        assert cover[0].max() == (2 if F else 1)
    # n_s < 2 F, down to 1 and 2 samples, with overlaps asked for everywhere
    _check_mix(ctx, "short", [50, 3, 100, 1, 2, 127, 128], [0] * 7, [-64, -64, -10, -64, -1, -64, 0], 64, seed=11)
    # empty segments first, in the middle and last in a document; a document of empty segments only (length lead + tail)
    want, cover, pos, doc_lens = _check_mix(ctx, "empty", [0, 300, 0, 200, 0, 0, 0, 10], [0, 0, 0, 0, 0, 1, 1, 2], [-20, -20, 30, -20, 0, 5, 0, 0], 32, lead=4, tail=6, seed=12)
    assert doc_lens.tolist() == [4 + 300 + 30 + 200 + 6, 4 + 5 + 6, 20] and not want[1].any()
    # an overlap that straddles a 1024-sample tile border, in the second document so that its offset is no multiple of the tile
    want, cover, pos, doc_lens = _check_mix(ctx, "straddle", [37, 1050, 500, 2100], [0, 1, 1, 1], [0, -64, -64, 0], 64, seed=13)
    assert pos[2] == 1050 - 64 and (cover[1][986:1050] == 2).all() and 986 < 1024 < 1050
    # one segment; 40 documents of one 1-sample segment each; lead and tail beyond a tile; values that clamp in int16
    _check_mix(ctx, "one", [777], [0], [0], 64, seed=14)
    want, *_ = _check_mix(ctx, "forty", [1] * 40, list(range(40)), [0] * 40, 64, seed=15)
    assert all(w.size == 1 for w in want)
    want, *_ = _check_mix(ctx, "lead_tail", [600, 900], [0, 0], [1500, 0], 16, lead=1500, tail=1100, seed=16)
    assert want[0].size == 1500 + 600 + 1500 + 900 + 1100 and not want[0][:1500].any() and not want[0][-1100:].any()
    want, *_ = _check_mix(ctx, "clamp", [3000, 2500], [0, 0], [-64, 0], 64, amp=1.3, seed=17)
    i16 = so.to_i16(want[0])
    assert (i16 == 32767).sum() > 20 and (i16 == -32768).sum() > 20 and np.abs(want[0]).max() > 2.0
    _check_mix(ctx, "no_i16", [1500, 700], [0, 0], [-64, 0], 64, seed=18, want_i16=False)
    # what the kernel would mishandle is refused
    from emotivoice_amd import _ffi
    lib = _ffi.lib()
    d = torch.zeros(4096, device="cuda")
    tab = _table(ctx, 64)

    def mix(n, pos, fl, fr, doc_len, F=64, sd=(0, 0, 0)):
        a = lambda v, t: np.ascontiguousarray(v, t)     # noqa: E731
        n_, sd_, pos_, fl_, fr_, dl_ = a(n, np.int64), a(sd[:len(n)], np.int32), a(pos, np.int64), a(fl, np.int32), a(fr, np.int32), a([doc_len], np.int64)
        src = np.zeros(len(n), np.int64)
        return lib.ev_op_stitch_mix(d.data_ptr(), len(n), _p(src), _p(n_), _p(sd_), _p(pos_), _p(fl_), _p(fr_), _p(tab), F, 1, _p(dl_), d.data_ptr() + 8192, None, None)
    assert mix([100, 100], [0, 100], [0, 0], [0, 0], 200) == 0
    for args in (([100, 100], [0, 100], [65, 0], [0, 0], 200), ([100, 100], [0, 100], [0, 0], [0, 101], 200), ([100, 100], [0, 101], [0, 0], [0, 0], 200),
                 ([100, 100], [10, 0], [0, 0], [0, 0], 200), ([100, 100, 100], [0, 50, 99], [0, 0, 0], [0, 0, 0], 300), ([100, -1], [0, 100], [0, 0], [0, 0], 200),
                 ([100, 20], [0, 40], [0, 0], [0, 0], 200)):
        assert mix(*args) == -2, args
    assert mix([100, 100], [0, 100], [0, 0], [0, 0], 200, F=4097) == -2 and mix([100, 100], [0, 100], [0, 0], [0, 0], 200, sd=(0, 2, 2)) == -2


def _doc_inputs(seed, lens):
    rng = np.random.default_rng(seed)
    out = []
    for L in lens:
        w = (0.4 * rng.standard_normal(L)).astype(np.float32)
        lead, tail = int(rng.integers(100, 400)), int(rng.integers(100, 400))
        w[:lead] *= 1e-5
        w[L - tail:] *= 1e-5
        out.append(w)
    return out


CFG = dict(trim_frac=0.005, keep=24, fade=80, lead=160, tail=320, want_int16=True)


def test_stitch_equals_the_oracle_and_is_bit_invariant(ctx):
    """A document alone, first / middle / last of a batch, from host and from device memory, twice: the same bits, and the oracle's."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.longform import StitchConfig
    eng = ctx["eng"]
    A, pa = _doc_inputs(21, [5000, 1800, 2600]), ["comma", -3.0, None]
    B, pb = _doc_inputs(22, [900]), [None]
    Cc, pc = _doc_inputs(23, [1200, 40, 3100, 2000]), [-5.0, -5.0, 12.0, None]
    Cc[1][:] = 0.0                                                       # a silent sentence: an empty segment between two cross-fades
    alone = eng.stitch(A, [0, 0, 0], pa, **CFG)
    tab = _table(ctx, 80)
    from emotivoice_amd.longform import plan_document
    want = so.stitch(A, [0, 0, 0], plan_document([0, 0, 0], pa)[1], tab, trim_frac=0.005, keep=24, lead=160, tail=320)
    assert np.array_equal(_bits(alone["docs"][0]), _bits(want["docs"][0])) and np.array_equal(alone["docs_i16"][0], so.to_i16(want["docs"][0]))
    assert np.array_equal(alone["seg_pos"], want["pos"]) and np.array_equal(alone["seg_start"], want["start"]) and np.array_equal(alone["seg_end"], want["end"])
    assert np.array_equal(_bits(alone["seg_peak"]), _bits(want["peak"])) and alone["doc_lens"].tolist() == want["doc_lens"].tolist()
    assert (want["start"] > 50).all() and (want["end"] < [5000, 1800, 2600]).all() and want["cover"][0].max() == 2
    again = eng.stitch(A, [0, 0, 0], pa, **CFG)
    assert np.array_equal(_bits(again["wav"]), _bits(alone["wav"]))
    for order, at in (((A, pa), (B, pb), (Cc, pc)), 0), (((B, pb), (A, pa), (Cc, pc)), 1), (((Cc, pc), (B, pb), (A, pa)), 2):
        wavs = [w for doc, _ in order for w in doc]
        docs = [d for d, (doc, _) in enumerate(order) for _ in doc]
        pauses = [p for _, ps in order for p in ps]
        batch = eng.stitch(wavs, docs, pauses, **CFG)
        assert np.array_equal(_bits(batch["docs"][at]), _bits(alone["docs"][0])) and np.array_equal(batch["docs_i16"][at], alone["docs_i16"][0]), at
        seg = np.nonzero(np.array(docs) == at)[0]
        assert np.array_equal(batch["seg_pos"][seg], alone["seg_pos"]) and np.array_equal(batch["seg_start"][seg], alone["seg_start"])
        w_all = so.stitch(wavs, docs, plan_document(docs, pauses)[1], tab, trim_frac=0.005, keep=24, lead=160, tail=320)
        for d in range(3):
            assert np.array_equal(_bits(batch["docs"][d]), _bits(w_all["docs"][d])), (at, d)
        ci = docs.index(0 if at == 2 else 2)                      # the first segment of Cc, whose silent second sentence is empty
        assert batch["seg_end"][ci + 1] == batch["seg_start"][ci + 1] == 0
    # device input: the same waveform at an offset inside a larger device buffer
    flat = np.concatenate([np.full(11, 3.0, np.float32)] + A)
    d = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    lens = np.array([w.size for w in A], np.int64)
    offs = 11 + np.concatenate([[0], np.cumsum(lens)[:-1]])
    sd, pause_after = plan_document([0, 0, 0], pa)
    res = eng.stitch_raw(3, d.data_ptr(), offs, lens, sd, pause_after, StitchConfig(**CFG), _ffi.EV_FLAG_DEVICE_INPUTS)
    dev = eng.stitch_to_numpy(res)
    assert np.array_equal(_bits(dev["wav"]), _bits(alone["wav"])) and np.array_equal(dev["wav_i16"], alone["wav_i16"])
    # no trim at all: no scan, the whole segments, peak 0; the library's default config is plain concatenation
    plain = eng.stitch_to_numpy(eng.stitch_raw(3, flat.ctypes.data, offs, lens, sd, np.zeros(3, np.int32), None))
    assert np.array_equal(_bits(plain["wav"]), _bits(np.concatenate(A))) and not plain["seg_peak"].any() and "wav_i16" not in plain
    assert plain["seg_start"].tolist() == [0, 0, 0] and plain["seg_end"].tolist() == lens.tolist()


def test_rejections_then_a_valid_call(ctx):
    """Every rejection by its message; the previous result stays valid and the next good call gives the same bits."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.longform import StitchConfig
    eng = ctx["eng"]
    lib = _ffi.lib()
    A = _doc_inputs(31, [1500, 1400])
    flat = np.concatenate(A)
    good = dict(S=2, seg_offsets=[0, 1500], seg_lens=[1500, 1400], seg_doc=[0, 0], pause_after=[-40, 0])

    def run(cfg_kw=None, size=None, **kw):
        a = dict(good, **kw)
        c = StitchConfig(**CFG).to_struct()
        for k, v in (cfg_kw or {}).items():
            setattr(c, k, v)
        r = _ffi.ev_stitch_result()
        r.struct_size = C.sizeof(r) if size is None else size
        so_, sl, sd, pa = (np.ascontiguousarray(a[k], t) for k, t in (("seg_offsets", np.int64), ("seg_lens", np.int64), ("seg_doc", np.int32), ("pause_after", np.int32)))
        rc = lib.ev_stitch(eng._h, a["S"], _p(flat), _p(so_), _p(sl), _p(sd), _p(pa), C.byref(c), 0, C.byref(r))
        return rc, lib.ev_last_error(eng._h).decode(), r
    rc, msg, keep = run()
    assert rc == 0, msg
    want = eng.stitch_to_numpy(keep)
    nan, inf = float("nan"), float("inf")
    big = 1 << 30
    checks = [(dict(size=40), "struct_size"), (dict(cfg_kw=dict(struct_size=16)), "struct_size"), (dict(S=0), "S 0"), (dict(S=65536), "S 65536"),
              (dict(seg_lens=[1500, 0]), "seg_lens[1]"), (dict(seg_offsets=[-1, 1500]), "seg_offsets[0]"), (dict(seg_doc=[1, 1]), "seg_doc[0]"),
              (dict(seg_doc=[0, 2]), "seg_doc[1]"), (dict(seg_doc=[0, -1]), "seg_doc[1]"), (dict(cfg_kw=dict(fade=-1)), "fade"),
              (dict(cfg_kw=dict(fade=4097)), "fade"), (dict(cfg_kw=dict(keep=-1)), "keep"), (dict(cfg_kw=dict(lead=-1)), "lead"), (dict(cfg_kw=dict(tail=-1)), "tail"),
              (dict(pause_after=[-4097, 0]), "pause_after[0]"), (dict(pause_after=[(1 << 24) + 1, 0]), "pause_after[0]"), (dict(cfg_kw=dict(trim_frac=nan)), "trim_frac"),
              (dict(cfg_kw=dict(trim_frac=-0.1)), "trim_frac"), (dict(cfg_kw=dict(trim_frac=1.0)), "trim_frac"), (dict(cfg_kw=dict(trim_abs=inf)), "trim_abs"),
              (dict(cfg_kw=dict(trim_abs=-1.0)), "trim_abs"), (dict(seg_lens=[big, 1400]), "document 0"),
              (dict(cfg_kw=dict(lead=big - 2000)), "document 0"), (dict(S=65, seg_offsets=[0] * 65, seg_lens=[1500] * 65, seg_doc=[0] * 65, pause_after=[1 << 24] * 65), "document 0")]
    for kw, needle in checks:
        rc, msg, _ = run(**kw)
        assert rc < 0 and needle in msg, (kw, msg)
        still = eng.stitch_to_numpy(keep)                                # the previous result, untouched
        assert np.array_equal(_bits(still["wav"]), _bits(want["wav"])) and np.array_equal(still["seg_pos"], want["seg_pos"]), kw
    rc, msg, r = run()
    after = eng.stitch_to_numpy(r)
    assert rc == 0 and np.array_equal(_bits(after["wav"]), _bits(want["wav"])) and np.array_equal(after["wav_i16"], want["wav_i16"])
    with pytest.raises(ValueError, match="entries each"):
        eng.stitch_raw(2, flat.ctypes.data, [0, 1500], [1500, 1400], [0, 0], [0])


def test_result_survives_the_other_calls(ctx):
    from emotivoice_amd.longform import StitchConfig, plan_document
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    A = _doc_inputs(41, [4000, 3000, 5000])
    flat = np.concatenate(A)
    lens = np.array([w.size for w in A], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    sd, pa = plan_document([0, 0, 1], ["sentence", None, None])
    res = eng.stitch_raw(3, flat.ctypes.data, offs, lens, sd, pa, StitchConfig(**CFG))
    before = eng.stitch_to_numpy(res)
    syn = eng.synthesize(synth_inputs(9, [20]))
    eng.resample([A[0]], 44100, trim=True)
    eng.features([A[2]])
    eng.vocoder([syn["mel_list"][0].T.copy()])
    after = eng.stitch_to_numpy(res)
    assert np.array_equal(_bits(before["wav"]), _bits(after["wav"])) and np.array_equal(before["wav_i16"], after["wav_i16"])
    assert before["wav"].size > 10000 and np.isfinite(syn["wav"]).all() and np.array_equal(before["doc_lens"], after["doc_lens"])
    res2 = eng.stitch_raw(1, flat.ctypes.data, offs[:1], lens[:1], sd[:1], pa[:1], StitchConfig(**CFG))          # a second call replaces the result
    assert eng.stitch_to_numpy(res2)["doc_lens"].tolist() != before["doc_lens"].tolist()


def test_synthesize_long_end_to_end(ctx):
    """Two documents of 3 and 2 short sentences: the documents are the oracle applied to the D2H'd waveforms of ``synthesize`` on the same
    sentences, bit for bit, as fp32 and as int16, and the sentence times are seg_pos in seconds."""
    from emotivoice_amd.longform import StitchConfig, plan_document
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["eng"]
    utts = synth_inputs(51, [24, 11, 17, 9, 20], [3, 3, 3, 8, 8])
    documents = [dict(utts=utts[:3], pauses=["comma", -4.0]), (utts[3:], ["sentence"])]
    cfg = StitchConfig(lead_ms=20.0, tail_ms=50.0)
    out = eng.synthesize_long(documents, config=cfg)
    wavs = [w.copy() for w in eng.synthesize(utts)["wav_list"]]
    tab = _table(ctx, cfg.samples("fade"))
    sd, pa = plan_document([0, 0, 0, 1, 1], ["comma", -4.0, None, "sentence", None])
    want = so.stitch(wavs, sd, pa, tab, trim_frac=np.float32(0.005), keep=cfg.samples("keep"), lead=320, tail=800)
    assert len(out["documents"]) == 2 and out["sample_rate"] == 16000
    for d in range(2):
        assert out["documents"][d].dtype == np.float32 and np.array_equal(_bits(out["documents"][d]), _bits(want["docs"][d])), d
    assert np.array_equal(out["seg_pos"], want["pos"]) and np.array_equal(out["seg_start"], want["start"]) and np.array_equal(out["seg_end"], want["end"])
    n = want["end"] - want["start"]
    flat_times = [t for doc in out["sentence_times"] for t in doc]
    assert [len(doc) for doc in out["sentence_times"]] == [3, 2]
    for s, (t0, t1) in enumerate(flat_times):
        assert t0 == want["pos"][s] / 16000.0 and t1 == (want["pos"][s] + n[s]) / 16000.0
    assert want["pos"][0] == 320 and want["pos"][3] == 320 and (n > 0).all() and all(np.isfinite(w).all() for w in want["docs"])
    out16 = eng.synthesize_long(documents, config=StitchConfig(lead_ms=20.0, tail_ms=50.0, want_int16=True))
    for d in range(2):
        assert out16["documents"][d].dtype == np.int16 and np.array_equal(out16["documents"][d], so.to_i16(want["docs"][d])), d
    assert "wav" not in out16                                            # one D2H copy: the int16 documents only
    with pytest.raises(ValueError, match="sample_rate"):
        eng.synthesize_long(documents, config=StitchConfig(sample_rate=22050))
