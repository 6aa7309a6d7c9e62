"""MI355X: ev_resample -- recordings at any common rate -> the 16 kHz, optionally trimmed and padded, waveform on the device (include/evhip.h).
Accuracy against the float64 oracle within the float32 accumulation bound of the specified sum, the kernels at their edges on guard-banded
buffers, bit invariance, the trim against the numpy restatement of the reference, rejections, lifetime, and a 48 kHz recording through
align_recordings end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import resample_oracle as ro
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 7.0


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import align_oracle as ao
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    blob, man = pack_state_dict(ao.aligner_state_dict(synth_state_dict(0, "parity")))
    engs = {}
    for prec in ("mx", "strict", "fast"):
        engs[prec] = EVEngine(precision=prec, keep_stages=(prec == "mx"))
    engs["mx"].load_blob(blob, man)
    fx = dict(a_l20011=ro.speechlike(31, 20011, 44100), b_l12289_i16=ro.speechlike(32, 12289, 48000, i16=True))
    g = dict(np.load(os.path.join(GOLDEN_DIR, "features", "feat_a_n48_self.npz")))
    yield dict(engs=engs, fx=fx, g=g)
    for e in engs.values():
        e.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _utt(g):
    return dict(ling=g["in_ling"], speaker=int(g["in_speaker"]), style=g["in_style"], content=g["in_content"])


def _stage(eng, name):
    """A flat float32 stage of the resampler through ev_get_stage."""
    n = eng._lib.ev_get_stage(eng._h, name.encode(), None, 0)
    assert n > 0 and n % 4 == 0, eng._lib.ev_last_error(eng._h)
    out = np.zeros(n // 4, np.float32)
    assert eng._lib.ev_get_stage(eng._h, name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes) == n
    return out


def _resample_op(wavs, sr_in, sr_out, taps=None):
    """ev_op_resample on a guarded buffer: one output per utterance; nothing written past the packed outputs and every sample written."""
    from emotivoice_amd import _ffi
    up, down = ro.ratio(sr_in, sr_out)
    is16 = wavs[0].dtype == np.int16
    lens = np.array([len(w) for w in wavs], np.int64)
    ns = [ro.output_len(int(n), up, down) for n in lens]
    TT = sum(ns)
    d_wav = torch.from_numpy(np.concatenate(wavs).astype(np.int16 if is16 else np.float32)).cuda()
    d_y = torch.full((TT + 512,), GUARD, device="cuda")
    torch.cuda.synchronize()
    t = None if taps is None else np.ascontiguousarray(taps, np.float32)
    rc = _ffi.lib().ev_op_resample(d_wav.data_ptr(), 1 if is16 else 0, len(wavs), lens.ctypes.data_as(C.c_void_p), sr_in, sr_out,
                                   None if t is None else t.ctypes.data_as(C.c_void_p), 0 if t is None else (t.size - 1) // 2, d_y.data_ptr(), None)
    assert rc == 0
    y = d_y.cpu().numpy()
    assert (y[TT:] == GUARD).all() and (y[:TT] != GUARD).all()
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    return [y[offs[b]:offs[b + 1]] for b in range(len(wavs))]


def _trim_op(ys, frac, pad):
    from emotivoice_amd import _ffi
    lens = np.array([len(y) for y in ys], np.int64)
    cap = int(lens.sum()) + 2 * pad * len(ys)
    d_y = torch.from_numpy(np.concatenate(ys).astype(np.float32)).cuda()
    d_out = torch.full((cap + 512,), GUARD, device="cuda")
    torch.cuda.synchronize()
    out_lens, start, end = (np.full(len(ys), -5, np.int64) for _ in range(3))
    rc = _ffi.lib().ev_op_trim(d_y.data_ptr(), len(ys), lens.ctypes.data_as(C.c_void_p), frac, pad, d_out.data_ptr(), out_lens.ctypes.data_as(C.c_void_p),
                               start.ctypes.data_as(C.c_void_p), end.ctypes.data_as(C.c_void_p), None)
    assert rc == 0
    out = d_out.cpu().numpy()
    TT = int(out_lens.sum())
    assert (out[TT:] == GUARD).all() and (out[:TT] != GUARD).all()
    offs = np.concatenate([[0], np.cumsum(out_lens)])
    return [out[offs[b]:offs[b + 1]] for b in range(len(ys))], start, end


def _within_bound(name, y, x, h, up, down, bad):
    """|dev - o64| <= (ntaps + 2) 2^-24 max_p sum_j |h_p[j]| max|x| per output sample; lengths equal."""
    o64 = ro.resample64(x, h, up, down)
    assert y.size == o64.size == ro.output_len(len(x), up, down), name
    bound = ro.accumulation_bound(h, up, ro.taps_per_output(h, up), np.abs(ro.as_float(x)).max())
    err = float(np.abs(y.astype(np.float64) - o64).max()) if y.size else 0.0
    same = int((_bits(y) == _bits(ro.resample32(x, h, up, down))).sum())
    print(name, "n %d  E(dev) %.3e  bound %.3e  bit-equal to the float32 oracle %d / %d" % (y.size, err, bound, same, y.size))
    if not err <= bound:
        bad.append((name, err, bound))


def test_accuracy_within_the_accumulation_bound(ctx):
    from emotivoice_amd.resample import phase_table
    eng = ctx["engs"]["mx"]
    bad = []
    for name, sr_in in (("a_l20011", 44100), ("b_l12289_i16", 48000)):
        w = ctx["fx"][name]
        out = eng.resample([w], sr_in)
        h, up, down, half = ro.design(sr_in, 16000)
        assert out["wav_lens"][0] == ro.output_len(len(w), up, down) and out["trim_start"][0] == 0 and out["trim_end"][0] == out["wav_lens"][0]
        _within_bound(name, out["wav_list"][0], w, h, up, down, bad)
        assert np.abs(out["wav_list"][0]).max() > 0.1
        assert np.array_equal(_bits(_stage(eng, "resample_taps")), _bits(phase_table(h, up).reshape(-1)))      # the table in use
    assert not bad, bad


def test_op_resample_at_its_edges(ctx):
    """L = 1 and 2, outputs just below / at / above the kernel's tile, up > down, up = 1, the largest table (read through L1), a run too long for
    LDS (read through L1) with a small and with a large table, and taps whose half is no multiple of up."""
    from emotivoice_amd import _ffi
    TM = _ffi.EV_RESAMPLE_TILE
    rng = np.random.default_rng(7)

    def sig(L):
        return rng.uniform(-1.0, 1.0, L).astype(np.float32)
    odd = (0.2 * rng.standard_normal(11)).astype(np.float32)           # half = 5 with up = 3
    long_taps = (0.01 * rng.standard_normal(2 * 8200 + 1)).astype(np.float32)
    cases = [("up1", 48000, 16000, [1, 2, 3 * TM - 3, 3 * TM, 3 * TM + 1, 3 * (2 * TM) + 1], None),
             ("up2", 8000, 16000, [1, 2, TM // 2 - 1, TM // 2, TM // 2 + 1], None),
             ("up3_down2", 16000, 24000, [1, 2, 170, 171, 172], None),
             ("441_160", 44100, 16000, [1, 2, 701, 703, 706, 1500], None),
             ("441_320", 22050, 16000, [1, 353, 354], None),
             ("largest_table", 11025, 16000, [1, 2, 176, 177, 300], None),
             ("run_through_l1", 48000, 1000, [1, 47, 49, 20000], None),
             ("run_and_table_through_l1", 50000, 1000, [4000, 1], long_taps),
             ("odd_half", 16000, 24000, [1, 2, 171, 400], odd)]
    bad = []
    for name, sr_in, sr_out, Ls, taps in cases:
        up, down = ro.ratio(sr_in, sr_out)
        h = taps if taps is not None else ro.design(sr_in, sr_out)[0]
        wavs = [sig(L) for L in Ls]
        outs = _resample_op(wavs, sr_in, sr_out, taps)
        for w, y in zip(wavs, outs):
            _within_bound("%s/L%d" % (name, len(w)), y, w, h, up, down, bad)
    assert {ro.output_len(L, 1, 3) for L in (3 * TM - 3, 3 * TM, 3 * TM + 1)} == {TM - 1, TM, TM + 1}
    assert {ro.output_len(L, 160, 441) for L in (701, 703, 706)} == {TM - 1, TM, TM + 1}
    assert not bad, bad


def test_equal_rates_copy_and_impulses_reproduce_the_phase_rows(ctx):
    rng = np.random.default_rng(8)
    f = rng.uniform(-1.0, 1.0, 1031).astype(np.float32)
    i16 = rng.integers(-32768, 32767, 777, dtype=np.int16, endpoint=True)
    (yf, yf2), = [_resample_op([f, f[:1]], 22050, 22050)]
    assert np.array_equal(_bits(yf), _bits(f)) and np.array_equal(_bits(yf2), _bits(f[:1]))
    yi, = _resample_op([i16], 16000, 16000)
    assert np.array_equal(_bits(yi), _bits(i16.astype(np.float32) / np.float32(32768.0)))
    for sr_in, sr_out, L in ((44100, 16000, 50), (8000, 16000, 40), (11025, 16000, 30)):
        h, up, down, half = ro.design(sr_in, sr_out)
        for at in (0, L - 1):
            x = np.zeros(L, np.float32)
            x[at] = 1.0
            y, = _resample_op([x], sr_in, sr_out)
            i = np.arange(y.size, dtype=np.int64) * down - at * up
            want = np.where(np.abs(i) <= half, h[np.clip(i + half, 0, 2 * half)], np.float32(0.0)).astype(np.float32)
            assert (want != 0).sum() >= 2 and np.array_equal(y, want), (sr_in, at)


def test_bit_invariance(ctx):
    """Alone vs first, middle and last of a ragged batch of 5; int16 vs the equal floats; host vs device input; mx vs strict vs fast; twice."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.resample import ResampleConfig
    eng = ctx["engs"]["mx"]
    a = ctx["fx"]["a_l20011"][:5003].copy()
    rng = np.random.default_rng(9)
    o1, o2 = rng.uniform(-1, 1, 1).astype(np.float32), rng.uniform(-1, 1, 2777).astype(np.float32)
    kw = dict(trim=True)
    alone = eng.resample([a], 44100, **kw)
    again = eng.resample([a], 44100, **kw)
    batch = eng.resample([a, o1, a, o2, a], 44100, **kw)
    assert alone["wav_lens"][0] > 1600 and len(set(batch["wav_lens"].tolist())) == 3
    for pos in (0, 2, 4):
        assert np.array_equal(_bits(batch["wav_list"][pos]), _bits(alone["wav_list"][0])), pos
        assert batch["trim_start"][pos] == alone["trim_start"][0] and batch["trim_end"][pos] == alone["trim_end"][0]
    assert np.array_equal(_bits(again["wav"]), _bits(alone["wav"]))
    for j, w in ((1, o1), (3, o2)):
        assert np.array_equal(_bits(batch["wav_list"][j]), _bits(eng.resample([w], 44100, **kw)["wav_list"][0])), j
    i16 = ctx["fx"]["b_l12289_i16"][:4001]
    fl = i16.astype(np.float32) / np.float32(32768.0)
    oi, of = eng.resample([i16], 48000, **kw), eng.resample([fl], 48000, **kw)
    assert np.array_equal(_bits(oi["wav"]), _bits(of["wav"])) and oi["trim_start"][0] == of["trim_start"][0] and oi["wav"].size > 1600
    for prec in ("strict", "fast"):
        out = ctx["engs"][prec].resample([a], 44100, **kw)
        assert np.array_equal(_bits(out["wav"]), _bits(alone["wav"])), prec
    eng.resample_setup(ResampleConfig(sr_in=44100, **kw))
    d = torch.from_numpy(np.concatenate([a, o2])).cuda()
    torch.cuda.synchronize()
    dev = eng.resample_to_numpy(eng.resample_raw(2, d.data_ptr(), False, np.array([a.size, o2.size], np.int64), flags=_ffi.EV_FLAG_DEVICE_INPUTS))
    assert np.array_equal(_bits(dev["wav_list"][0]), _bits(alone["wav_list"][0]))
    assert np.array_equal(_bits(dev["wav_list"][1]), _bits(batch["wav_list"][3]))


def _trim_inputs():
    rng = np.random.default_rng(10)
    body = (0.4 * rng.standard_normal(3000)).astype(np.float32)
    quiet = np.concatenate([1e-4 * np.abs(body).max() * rng.uniform(-1, 1, 700), body, 1e-4 * np.abs(body).max() * rng.uniform(-1, 1, 900)]).astype(np.float32)
    loud_first = body.copy()
    loud_first[0] = 0.9
    only_last = np.zeros(1500, np.float32)
    only_last[-1] = 0.5
    return [quiet, loud_first, only_last, np.zeros(1300, np.float32)]


def test_trim_equals_the_numpy_restatement_of_the_reference(ctx):
    """sr_in == sr_out: start / end / output bit-equal to get_mel's trim for a quiet lead-in and tail, a start above the threshold at index 0, a
    last sample that alone is loud (empty cut) and all zeros (2 pad zeros, start = end = 0); the same through ev_op_trim on guarded buffers."""
    eng = ctx["engs"]["mx"]
    ys = _trim_inputs()
    out = eng.resample(ys, 16000, trim=True)
    op, op_start, op_end = _trim_op(ys, 0.005, 800)
    op3, _, _ = _trim_op(ys, 0.25, 3)
    for b, y in enumerate(ys):
        want, start, end = ro.trim(y, 0.005, 800)
        assert (out["trim_start"][b], out["trim_end"][b], out["wav_lens"][b]) == (start, end, want.size) == (op_start[b], op_end[b], op[b].size), b
        assert np.array_equal(_bits(out["wav_list"][b]), _bits(want)) and np.array_equal(_bits(op[b]), _bits(want)), b
        assert np.array_equal(_bits(op3[b]), _bits(ro.trim(y, 0.25, 3)[0])), b
    assert (out["trim_start"][0], out["trim_end"][0]) == (700, 3699) and out["trim_start"][1] == 0
    assert (out["trim_start"][2], out["trim_end"][2], out["wav_lens"][2]) == (1499, 1499, 1600)
    assert (out["trim_start"][3], out["trim_end"][3], out["wav_lens"][3]) == (0, 0, 1600) and not out["wav_list"][3].any()
    from emotivoice_amd import _ffi
    d = torch.zeros(4096, device="cuda")
    one = np.array([100], np.int64)
    o = np.zeros(3, np.int64)
    args = lambda frac, pad, dst, lens=one: (d.data_ptr(), 1, lens.ctypes.data_as(C.c_void_p), frac, pad, dst, o[0:].ctypes.data_as(C.c_void_p),     # noqa: E731
                                             o[1:].ctypes.data_as(C.c_void_p), o[2:].ctypes.data_as(C.c_void_p), None)
    lib = _ffi.lib()
    assert lib.ev_op_trim(*args(0.005, 8, d.data_ptr())) == -2             # in place
    for frac, pad in ((0.0, 8), (1.0, 8), (float("nan"), 8), (0.005, -1)):
        assert lib.ev_op_trim(*args(frac, pad, d.data_ptr() + 8192)) == -2, (frac, pad)
    assert lib.ev_op_trim(*args(0.005, 8, d.data_ptr() + 8192, np.array([0], np.int64))) == -2


def test_resample_then_trim(ctx):
    """The combined path is the numpy trim of the device's own untrimmed output, bit for bit, and cuts where the float64 pipeline cuts (fixtures
    whose float64 |y| stays 1e-5 away from the threshold within 64 samples of either cut -- asserted first)."""
    eng = ctx["engs"]["mx"]
    rng = np.random.default_rng(12)
    wavs, rates = [], (44100, 48000)
    for sr, name in zip(rates, ("a_l20011", "b_l12289_i16")):
        body = ro.as_float(ctx["fx"][name])[:9000]
        wavs.append(np.concatenate([2e-5 * rng.uniform(-1, 1, 3000), body, 2e-5 * rng.uniform(-1, 1, 2000)]).astype(np.float32))
    for sr, w in zip(rates, wavs):
        h, up, down, half = ro.design(sr, 16000)
        y64 = ro.resample64(w, h, up, down)
        s64, e64, thr = ro.trim64(y64)
        margin = ro.cut_margin(y64, thr, s64, e64)
        print(sr, "float64 cut %d .. %d of %d, margin %.2e" % (s64, e64, y64.size, margin))
        assert margin >= 1e-5 and 0 < s64 < e64 < y64.size - 1
        out = eng.resample([w, w[:4000]], sr, trim=True)
        raw = _stage(eng, "resample_raw")
        n0 = ro.output_len(w.size, up, down)
        assert raw.size == n0 + ro.output_len(4000, up, down)
        want, start, end = ro.trim(raw[:n0], 0.005, 800)
        assert np.array_equal(_bits(out["wav_list"][0]), _bits(want)) and (out["trim_start"][0], out["trim_end"][0]) == (start, end)
        assert np.array_equal(_bits(out["wav_list"][1]), _bits(ro.trim(raw[n0:], 0.005, 800)[0]))
        assert (start, end) == (s64, e64)


def test_rejections_then_a_valid_call(ctx):
    """Every rejection by its message, each followed by a good call that gives the bits of an untouched handle; ev_resample before any setup."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.resample import ResampleConfig
    lib = _ffi.lib()
    wav = ctx["fx"]["a_l20011"][:3000].copy()
    want = ctx["engs"]["mx"].resample([wav], 44100, trim=True)
    fresh = EVEngine(precision="mx")
    try:
        def run(lens=(3000,), B=None, size=None):
            r = _ffi.ev_resample_result()
            r.struct_size = C.sizeof(r) if size is None else size
            wl = np.asarray(lens, np.int64)
            rc = lib.ev_resample(fresh._h, len(wl) if B is None else B, wav.ctypes.data_as(C.c_void_p), 0, wl.ctypes.data_as(C.c_void_p), 0, C.byref(r))
            return rc, lib.ev_last_error(fresh._h).decode()

        def setup(cfg_size=None, taps=None, **kw):
            c = _ffi.ev_resample_config()
            lib.ev_default_resample_config(C.byref(c))
            assert (c.struct_size, c.sr_in, c.sr_out, c.taps, c.trim_frac, c.trim_pad) == (C.sizeof(c), 16000, 16000, None, 0.0, 0)
            c.sr_in = 44100
            for k, v in kw.items():
                setattr(c, k, v)
            if taps is not None:
                c.taps = taps.ctypes.data
            if cfg_size is not None:
                c.struct_size = cfg_size
            rc = lib.ev_resample_setup(fresh._h, C.byref(c))
            return rc, lib.ev_last_error(fresh._h).decode()
        rc, msg = run()
        assert rc < 0 and "ev_resample_setup has not been called" in msg
        nan, inf = float("nan"), float("inf")
        t3, tbad = np.ones(3, np.float32), np.array([0.0, inf, 0.0], np.float32)
        many = np.zeros(32771, np.float32)
        checks = [(setup, dict(cfg_size=24), "struct_size"), (setup, dict(sr_in=0), "sr_in"), (setup, dict(sr_out=-5), "sr_out"),
                  (setup, dict(sr_in=16001), "EV_RESAMPLE_MAX_RATIO"), (setup, dict(sr_in=1, sr_out=1025), "EV_RESAMPLE_MAX_RATIO"),
                  (setup, dict(taps=many, half_len=16385), "EV_RESAMPLE_MAX_TAPS"), (setup, dict(taps=t3, half_len=0), "half_len"),
                  (setup, dict(taps=tbad, half_len=1), "taps[1]"), (setup, dict(trim_frac=-0.1), "trim_frac"), (setup, dict(trim_frac=1.0), "trim_frac"),
                  (setup, dict(trim_frac=nan), "trim_frac"), (setup, dict(trim_frac=0.005, trim_pad=-1), "trim_pad"),
                  (run, dict(size=40), "struct_size"), (run, dict(lens=[100, 0]), "wav_lens[1]"), (run, dict(lens=[16384 * 256 * 3]), "EV_ALIGN_MAX_FRAMES"),
                  (run, dict(B=0), "B 0"), (run, dict(B=65536), "B 65536")]
        for fn, kw, needle in checks:
            rc, msg = fn(**kw)
            assert rc < 0 and needle in msg, (kw, msg)
            ok = fresh.resample([wav], 44100, trim=True) if fn is run else None
            if ok is not None:
                assert np.array_equal(_bits(ok["wav"]), _bits(want["wav"])), kw
        # a rejected setup leaves the previous one in place
        fresh.resample([wav], 44100, trim=True)
        assert setup(sr_in=0)[0] < 0
        r = fresh.resample_to_numpy(fresh.resample_raw(1, wav.ctypes.data, False, np.array([3000], np.int64)))
        assert np.array_equal(_bits(r["wav"]), _bits(want["wav"]))
        # 48000 -> 16000 with trim: 16384 * 256 outputs fit without the padding only
        fresh.resample_setup(ResampleConfig(sr_in=48000, trim=True))
        rc, msg = run(lens=[16384 * 256 * 3 - 2])
        assert rc < 0 and "EV_ALIGN_MAX_FRAMES" in msg
    finally:
        fresh.close()


def test_result_survives_the_other_calls(ctx):
    from emotivoice_amd.resample import ResampleConfig
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["engs"]["mx"]
    g = ctx["g"]
    w = ctx["fx"]["a_l20011"]
    eng.resample_setup(ResampleConfig(sr_in=44100, trim=True))
    res = eng.resample_raw(1, w.ctypes.data, False, np.array([w.size], np.int64))
    before = eng.resample_to_numpy(res)
    eng.features([g["wav"]])
    eng.pitch([g["wav"]])
    syn = eng.synthesize(synth_inputs(9, [40]))
    after = eng.resample_to_numpy(res)
    assert np.array_equal(_bits(before["wav"]), _bits(after["wav"])) and np.isfinite(syn["wav"]).all() and before["wav"].size > 5000
    res2 = eng.resample_raw(1, w.ctypes.data, False, np.array([3000], np.int64))           # a second call replaces the result
    second = eng.resample_to_numpy(res2)
    assert second["wav_lens"][0] != before["wav_lens"][0]
    assert np.array_equal(_bits(second["wav"]), _bits(eng.resample([w[:3000]], 44100, trim=True)["wav"]))


def test_a_48_khz_recording_end_to_end(ctx):
    """The fixture's waveform upsampled to 48 kHz by the float64 oracle between 0.3 s of zeros: align_recordings(sample_rate=48000, trim=True)
    aligns the trimmed 16 kHz waveform, reports the offset back to the recording's clock, hands the device waveform to ev_features without a copy,
    and without the new arguments stays on the parent's path."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.alignment import align_recordings
    from emotivoice_amd.resample import ResampleConfig
    eng = ctx["engs"]["mx"]
    g = ctx["g"]
    utt = _utt(g)
    h, up, down, half = ro.design(16000, 48000)
    z = np.zeros(int(0.3 * 48000), np.float32)
    x48 = np.concatenate([z, ro.resample64(g["wav"], h, up, down).astype(np.float32), z])
    out = align_recordings(eng, [utt], [x48], energy_stats=(0.0, 1.0), sample_rate=48000, trim=True)
    n = int(out["resampled_lens"][0])
    assert int(out["durations"].sum()) == n // 256 + 1 == int(out["mel_lens"][0])
    assert abs(n - (g["wav"].size + 1600)) <= 4
    assert abs(out["time_offset_s"][0] - (0.3 - 0.05)) <= 1.0 / 16000 + 1e-12
    # the zero-copy hand-over: the mel from the device pointer is the mel of the D2H copy of the same waveform
    eng.resample_setup(ResampleConfig(sr_in=48000, trim=True))
    rs = eng.resample_raw(1, x48.ctypes.data, False, np.array([x48.size], np.int64))
    host = eng.resample_to_numpy(rs)
    assert host["wav_lens"][0] == n
    dev = eng.features_to_numpy(eng.features_raw(1, rs.wav, False, host["wav_lens"], flags=_ffi.EV_FLAG_DEVICE_INPUTS))
    cpu = eng.features([host["wav_list"][0]])
    assert np.array_equal(_bits(dev["mel_list"][0]), _bits(cpu["mel_list"][0])) and np.array_equal(_bits(dev["energy"]), _bits(cpu["energy"]))
    same = eng.align([utt], cpu["mel_list"], energy=cpu["energy_list"])
    assert np.array_equal(same["durations"], out["durations"]) and np.array_equal(_bits(same["score"]), _bits(out["score"]))
    # without the new arguments: the parent's path
    f = eng.features([g["wav"]])
    want = eng.align([utt], f["mel_list"], energy=f["energy_list"])
    for kw in (dict(), dict(sample_rate=16000), dict(sample_rate=None, trim=False)):
        plain = align_recordings(eng, [utt], [g["wav"]], energy_stats=(0.0, 1.0), **kw)
        assert "resampled_lens" not in plain and "time_offset_s" not in plain
        assert np.array_equal(plain["durations"], want["durations"]) and np.array_equal(_bits(plain["score"]), _bits(want["score"]))
        assert np.array_equal(_bits(plain["energy"]), _bits(want["energy"]))
