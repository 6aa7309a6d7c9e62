"""ev_stitch's host side: the library's ramp table and plan against the numpy oracle, the oracle's own properties (a cross-fade of a constant, bit
copies in the interior, the length formula, at most two segments per sample), split_text and StitchConfig's rejections.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import stitch_oracle as so


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cfg(**kw):
    from emotivoice_amd import _ffi
    c = _ffi.ev_stitch_config()
    _ffi.lib().ev_default_stitch_config(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _lib_plan(n, seg_doc, pause_after, **kw):
    from emotivoice_amd import _ffi
    lib = _ffi.lib()
    n, sd, pa = np.ascontiguousarray(n, np.int64), np.ascontiguousarray(seg_doc, np.int32), np.ascontiguousarray(pause_after, np.int32)
    S = n.size
    pos, fl, fr = np.full(S, -7, np.int64), np.full(S, -7, np.int32), np.full(S, -7, np.int32)
    doc_lens = np.full(int(sd.max()) + 1 if S else 1, -7, np.int64)
    c = _cfg(**kw)
    rc = lib.ev_stitch_plan(S, _p(n), _p(sd), _p(pa), C.byref(c), _p(pos), _p(fl), _p(fr), _p(doc_lens))
    return rc, pos, fl, fr, doc_lens, lib.ev_last_error(None).decode()


def _random_plan_inputs(rng, small=False):
    S = int(rng.integers(1, 9))
    F = int(rng.choice([0, 1, 2, 3, 5, 64])) if small else int(rng.integers(0, 200))
    n = rng.integers(0, 8 if small else 400, S)
    n[rng.random(S) < 0.15] = 0
    seg_doc = np.cumsum(np.concatenate([[0], rng.random(S - 1) < 0.3])).astype(np.int32)
    pause = rng.integers(-(2 * F + 3), 40, S).clip(-so.MAX_FADE, None).astype(np.int32)
    return n.astype(np.int64), seg_doc, pause, F, int(rng.integers(0, 5)), int(rng.integers(0, 5))


def test_default_config_is_plain_concatenation():
    from emotivoice_amd import _ffi
    c = _cfg()
    assert (c.struct_size, c.trim_frac, c.trim_abs, c.keep, c.fade, c.lead, c.tail, c.want_i16) == (C.sizeof(_ffi.ev_stitch_config), 0.0, 0.0, 0, 0, 0, 0, 0)
    rc, pos, fl, fr, doc_lens, _ = _lib_plan([5, 3, 4], [0, 0, 1], [0, 0, 0])
    assert rc == 2 and pos.tolist() == [0, 5, 0] and doc_lens.tolist() == [8, 4] and not fl.any() and not fr.any()


def test_library_ramp_equals_the_python_table():
    """ev_stitch_ramp touches no device.  The two cos implementations may differ in the last float64 bit, which can move the rounded float32 by one
    ulp.  Worst case seen: 0 ulp for F = 1, 2, 64 and 4096 (every value equal); the bound stays 1 ulp."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.longform import ramp_table
    lib = _ffi.lib()
    for F in (1, 2, 64, 4096):
        got = np.full(F, -1.0, np.float32)
        assert lib.ev_stitch_ramp(F, _p(got)) == F
        want = so.ramp_table(F)
        assert np.array_equal(want, ramp_table(F))
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
        worst = float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp).max())
        print("F %d worst %.2f ulp, equal %d / %d" % (F, worst, int((got == want).sum()), F))
        assert worst <= 1.0
        assert (got > 0).all() and (got < 1.0 + 1e-7).all() and (np.diff(got) >= 0).all()
        assert np.abs(got.astype(np.float64) + got[::-1].astype(np.float64) - 1.0).max() <= 2.0 ** -23          # tab[i] + tab[F - 1 - i] = 1
    assert lib.ev_stitch_ramp(0, None) == 0
    assert lib.ev_stitch_ramp(-1, None) == -1 and lib.ev_stitch_ramp(4097, _p(np.zeros(4097, np.float32))) == -1


def test_library_plan_equals_the_oracle():
    rng = np.random.default_rng(0)
    for it in range(3000):
        n, seg_doc, pause, F, lead, tail = _random_plan_inputs(rng, small=it % 2 == 0)
        rc, pos, fl, fr, doc_lens, msg = _lib_plan(n, seg_doc, pause, fade=F, lead=lead, tail=tail)
        assert rc == seg_doc[-1] + 1, msg
        w_pos, w_fl, w_fr, w_len = so.plan(n, seg_doc, pause, F, lead, tail)
        assert np.array_equal(pos, w_pos) and np.array_equal(fl, w_fl) and np.array_equal(fr, w_fr) and np.array_equal(doc_lens, w_len), (n, seg_doc, pause, F)


def test_plan_clamps():
    """n in {0, 1, 2, 3}, -pause > F, -pause > n / 2 and an empty neighbour, by hand and against the library."""
    cases = [  # n, pause, F -> pos, fl, fr, doc_len
        ([0, 1, 2, 3], [-9, -9, -9, 0], 4, [0, 0, 1, 2], [0, 0, 1, 1], [0, 0, 1, 1], 5),        # an empty / a 1-sample neighbour: no overlap; 2 | 3 overlap 1
        ([10, 10], [-100, 0], 3, [0, 7], [3, 3], [3, 3], 17),                                     # -pause > F
        ([4, 100], [-50, 0], 64, [0, 2], [2, 2], [2, 50], 102),                                   # -pause > n / 2
        ([6, 0, 6], [-3, -3, 0], 3, [0, 6, 6], [3, 0, 3], [3, 0, 3], 12),                         # an empty middle: both joints are plain
        ([8, 8], [5, 0], 2, [0, 13], [2, 2], [2, 2], 21),                                         # a pause
        ([8, 8], [-2, 0], 0, [0, 8], [0, 0], [0, 0], 16),                                         # F = 0: a negative pause is no overlap and no gap
    ]
    for n, pause, F, pos, fl, fr, doc_len in cases:
        sd = [0] * len(n)
        got = so.plan(n, sd, pause, F)
        assert (got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3].tolist()) == (pos, fl, fr, [doc_len]), (n, pause, F, got)
        rc, l_pos, l_fl, l_fr, l_len, msg = _lib_plan(n, sd, pause, fade=F)
        assert rc == 1 and (l_pos.tolist(), l_fl.tolist(), l_fr.tolist(), l_len.tolist()) == (pos, fl, fr, [doc_len]), msg


def test_plan_rejections_name_the_field():
    from emotivoice_amd import _ffi
    ok = dict(n=[4, 4], seg_doc=[0, 0], pause_after=[0, 0])
    nan = float("nan")
    checks = [(dict(struct_size=8), "struct_size"), (dict(fade=-1), "fade"), (dict(fade=4097), "fade"), (dict(keep=-1), "keep"), (dict(lead=-1), "lead"),
              (dict(tail=-2), "tail"), (dict(trim_frac=1.0), "trim_frac"), (dict(trim_frac=nan), "trim_frac"), (dict(trim_frac=-0.5), "trim_frac"),
              (dict(trim_abs=-1.0), "trim_abs"), (dict(trim_abs=float("inf")), "trim_abs")]
    for kw, needle in checks:
        rc, *_, msg = _lib_plan(**ok, **kw)
        assert rc == -1 and needle in msg, (kw, msg)
    for arrays, needle in ((dict(ok, seg_doc=[1, 1]), "seg_doc[0]"), (dict(ok, seg_doc=[0, 2]), "seg_doc[1]"), (dict(n=[4, 4, 4], seg_doc=[0, 1, 0], pause_after=[0, 0, 0]), "seg_doc[2]"),
                           (dict(ok, pause_after=[-4097, 0]), "pause_after[0]"), (dict(ok, pause_after=[(1 << 24) + 1, 0]), "pause_after[0]"),
                           (dict(ok, n=[4, -1]), "n[1]"), (dict(ok, n=[1 << 30, 1]), "document 0")):
        rc, *_, msg = _lib_plan(**arrays)
        assert rc == -1 and needle in msg, (arrays, msg)
    # the pause after a document's last segment is ignored, whatever it holds
    rc, pos, *_ = _lib_plan([4, 4], [0, 1], [-99999, 1 << 30])
    assert rc == 2 and pos.tolist() == [0, 0]
    lib = _ffi.lib()
    c = _cfg()
    z = np.zeros(1, np.int64)
    assert lib.ev_stitch_plan(0, _p(z), _p(z), _p(z), C.byref(c), _p(z), _p(z), _p(z), _p(z)) == -1 and "S 0" in lib.ev_last_error(None).decode()
    assert lib.ev_stitch_plan(65536, _p(z), _p(z), _p(z), C.byref(c), _p(z), _p(z), _p(z), _p(z)) == -1


def test_a_constant_cut_in_two_and_overlapped_by_F_stays_one():
    for F in (1, 2, 64, 4096):
        tab = so.ramp_table(F)
        a, b = np.ones(2 * F + 37, np.float32), np.ones(2 * F + 11, np.float32)
        r = so.stitch([a, b], [0, 0], [-F, 0], tab)
        doc = r["docs"][0]
        assert r["pos"].tolist() == [0, a.size - F] and doc.size == a.size + b.size - F
        joint = doc[a.size - F:a.size]
        assert (r["cover"][0][a.size - F:a.size] == 2).all() and r["cover"][0].max() == 2
        assert np.abs(joint.astype(np.float64) - 1.0).max() <= 2.0 ** -23, F
        inner = slice(F, doc.size - F)
        assert np.abs(doc[inner].astype(np.float64) - 1.0).max() <= 2.0 ** -23


def test_interior_samples_are_bit_copies_and_the_length_formula_holds():
    rng = np.random.default_rng(3)
    F, lead, tail, keep = 48, 100, 70, 16
    tab = so.ramp_table(F)
    wavs = []
    for L in (900, 700, 1200):
        w = (0.3 * rng.standard_normal(L)).astype(np.float32)
        w[:150] *= 1e-5
        w[-200:] *= 1e-5
        wavs.append(w)
    wavs[1][300] = np.float32(-0.0)
    pause = [160, -30, 0]
    r = so.stitch(wavs, [0, 0, 0], pause, tab, trim_frac=0.005, keep=keep, lead=lead, tail=tail)
    n = r["end"] - r["start"]
    assert (n < [900, 700, 1200]).all() and (n > 300).all()
    assert r["doc_lens"][0] == lead + n.sum() + 160 - 30 + tail == r["docs"][0].size
    doc = r["docs"][0]
    for s, w in enumerate(wavs):
        lo, hi = int(r["pos"][s]) + int(r["fl"][s]), int(r["pos"][s]) + int(n[s]) - int(r["fr"][s])
        src = w[r["start"][s] + r["fl"][s]:r["end"][s] - r["fr"][s]]
        assert np.array_equal(doc[lo:hi].view(np.uint32), src.view(np.uint32)), s
    assert not doc[:lead].any() and not doc[-tail:].any() and not np.signbit(doc[:lead]).any()
    gap = slice(int(r["pos"][0] + n[0]), int(r["pos"][1]))
    assert gap.stop - gap.start == 160 and not doc[gap].any()
    assert (r["fr"][1], r["fl"][2]) == (30, 30) and (r["fl"][0], r["fr"][0], r["fl"][1], r["fr"][2]) == (F, F, F, F)
    # the last sample above the threshold is kept (ev_resample's trim drops it)
    x = np.zeros(50, np.float32)
    x[10], x[30] = 0.5, 0.25
    assert so.cut(x, 0.005, 0.0, 0)[:2] == (10, 31) and so.cut(x, 0.005, 0.0, 4)[:2] == (6, 35) and so.cut(x, 0.0, 0.3, 0)[:2] == (10, 11)
    assert so.cut(np.zeros(9, np.float32), 0.005, 0.0, 3)[:2] == (0, 0) and so.cut(x, 0.0, 0.6, 3)[:2] == (0, 0) and so.cut(x, 0.0, 0.0, 3)[:2] == (0, 50)


def test_at_most_two_segments_cover_any_sample():
    """Over 10 000 random plans: pos[s + 2] >= pos[s] + n[s] inside a document, starts and ends never decrease, every segment inside its document."""
    rng = np.random.default_rng(1)
    for it in range(10000):
        n, seg_doc, pause, F, lead, tail = _random_plan_inputs(rng, small=it % 2 == 0)
        pos, fl, fr, doc_lens = so.plan(n, seg_doc, pause, F, lead, tail)
        end = pos + n
        same1 = seg_doc[1:] == seg_doc[:-1]
        assert (pos[1:][same1] >= pos[:-1][same1]).all() and (end[1:][same1] >= end[:-1][same1]).all()
        same2 = seg_doc[2:] == seg_doc[:-2]
        assert (pos[2:][same2] >= end[:-2][same2]).all(), (n, seg_doc, pause, F)
        assert (pos >= lead).all() and (end + tail <= doc_lens[seg_doc]).all()
        assert (fl <= np.minimum(F, n // 2)).all() and (fr <= np.minimum(F, n // 2)).all()
        if it % 50 == 0:
            cuts = [np.ones(int(v), np.float32) for v in n]
            _, cover = so.mix(cuts, seg_doc, pos, fl, fr, doc_lens, so.ramp_table(F))
            assert max(int(c.max()) if c.size else 0 for c in cover) <= 2


def test_int16_truncates_then_clamps():
    x = np.array([0.0, 0.99999, 1.0, 1.5, -1.0, -1.00004, -1.7, 0.5 / 32768, -0.5 / 32768, 1.5 / 32768, -1.5 / 32768, 32767.9 / 32768], np.float32)
    assert so.to_i16(x).tolist() == [0, 32767, 32767, 32767, -32768, -32768, -32768, 0, 0, 1, -1, 32767]


TEXTS = [
    "今天天气很好。我们去公园散步吧！你觉得怎么样？好的；走吧。",
    "The engine is fast. It runs at 12 000x real time! Does it stitch? Yes; it does.",
    "第一段，有逗号、顿号，还有一个很长很长很长很长很长很长很长很长很长很长很长很长的句子。\n\nSecond paragraph: pi is 3.14, at 12:30 a.m. it was e.g. fine... really?!\n最后一行没有句号",
    "   \n\n  ",
    "Averyveryveryveryveryveryveryveryveryveryveryveryverylongwordwithoutanyspaces and more words that follow it, here.",
    "“引号里的话。”他说。'Quoted.' She said.",
]


def _squash(s):
    return re.sub(r"\s+", "", s)


@pytest.mark.parametrize("max_chars", [8, 20, 80])
def test_split_text(max_chars):
    from emotivoice_amd.longform import PAUSE_CLASSES, pauses_ms, split_text
    for text in TEXTS:
        pieces, joints = split_text(text, max_chars)
        assert len(joints) == max(len(pieces) - 1, 0)
        assert all(p and p == p.strip() and len(p) <= max_chars for p in pieces), pieces
        assert _squash("".join(pieces)) == _squash(text)
        assert set(joints) <= set(PAUSE_CLASSES) <= set(pauses_ms)
    assert split_text(TEXTS[3], max_chars) == ([], [])


def test_split_text_classes():
    from emotivoice_amd.longform import split_text
    pieces, joints = split_text(TEXTS[0], 80)
    assert pieces == ["今天天气很好。", "我们去公园散步吧！", "你觉得怎么样？", "好的；", "走吧。"] and joints == ["sentence"] * 4
    pieces, joints = split_text(TEXTS[1], 80)
    assert pieces == ["The engine is fast.", "It runs at 12 000x real time!", "Does it stitch?", "Yes;", "it does."] and joints == ["sentence"] * 4
    pieces, joints = split_text("One, two, three, four. Next line\nLast", 12)
    assert pieces == ["One, two,", "three, four.", "Next line", "Last"] and joints == ["comma", "sentence", "paragraph"]
    pieces, joints = split_text("pi is 3.14, at 12:30 it was fine... really?!", 80)
    assert pieces == ["pi is 3.14, at 12:30 it was fine...", "really?!"]
    pieces, joints = split_text("abcdefghij klm", 4)
    assert pieces == ["abcd", "efgh", "ij", "klm"] and joints == ["none", "none", "none"]
    pieces, joints = split_text(TEXTS[5], 80)
    assert pieces == ["“引号里的话。”", "他说。", "'Quoted.'", "She said."]
    with pytest.raises(ValueError):
        split_text("a", 0)


def test_stitch_config_rejections_and_units():
    from emotivoice_amd.longform import StitchConfig, flatten_documents, pause_samples, plan_document
    c = StitchConfig().validate()
    assert (c.trim_frac, c.samples("keep"), c.samples("fade"), c.samples("lead"), c.samples("tail")) == (0.005, 160, 80, 0, 0)
    s = StitchConfig(fade=7, keep_ms=1.0, lead_ms=2.5, want_int16=True).to_struct()
    assert (s.struct_size, s.fade, s.keep, s.lead, s.tail, s.want_i16) == (C.sizeof(s), 7, 16, 40, 0, 1) and abs(s.trim_frac - 0.005) < 1e-9
    nan = float("nan")
    for kw, needle in ((dict(trim_frac=1.0), "trim_frac"), (dict(trim_frac=-0.1), "trim_frac"), (dict(trim_frac=nan), "trim_frac"), (dict(trim_abs=-1.0), "trim_abs"),
                       (dict(trim_abs=nan), "trim_abs"), (dict(keep=-1), "keep"), (dict(lead_ms=-1.0), "lead"), (dict(tail=-3), "tail"), (dict(fade=4097), "fade"),
                       (dict(fade_ms=300.0), "fade"), (dict(fade_ms=-1.0), "fade"), (dict(keep_ms=nan), "keep_ms"), (dict(sample_rate=0), "sample_rate")):
        with pytest.raises(ValueError, match=needle):
            StitchConfig(**kw).validate()
    assert pause_samples("sentence") == 4800 and pause_samples(-5) == -80 and pause_samples(None) == 0 and pause_samples("x", table={"x": 1.0}) == 16
    with pytest.raises(ValueError, match="unknown pause class"):
        pause_samples("breath")
    sd, pa = plan_document([0, 0, 0, 1, 1], ["comma", -5.0, "paragraph", 12.5, "sentence"])
    assert sd.dtype == pa.dtype == np.int32 and sd.tolist() == [0, 0, 0, 1, 1] and pa.tolist() == [1920, -80, 0, 200, 0]
    for bad_doc in ([1, 1], [0, 2], [0, 1, 0]):
        with pytest.raises(ValueError, match="seg_doc"):
            plan_document(bad_doc, [None] * len(bad_doc))
    with pytest.raises(ValueError, match=r"pause_after\[0\]"):
        plan_document([0, 0], [-300.0, None])
    with pytest.raises(ValueError, match="pauses for"):
        plan_document([0, 0], [None])
    utts, seg_doc, pauses = flatten_documents([dict(utts=["a", "b", "c"], pauses=["comma", 5]), (["d"], []), dict(utts=["e", "f"])])
    assert utts == list("abcdef") and seg_doc.tolist() == [0, 0, 0, 1, 2, 2] and pauses == ["comma", 5, None, None, "sentence", None]
    with pytest.raises(ValueError, match="document 0"):
        flatten_documents([(["a", "b"], [])])
