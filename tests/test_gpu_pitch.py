"""MI355X: ev_pitch -- wav -> F0 track on the device (include/evhip.h).  Accuracy against the float64 oracle with the oracle's own float32
evaluation as the yardstick, ground truth on signals of known F0, bit invariance (batch position, int16 / float, precision mode, host / device
input), the two kernels at their edges, rejections, lifetime, and wav -> per-token pitch -> prosody transfer end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import align_oracle as ao
import pitch_oracle as po
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLOOR = 2.0 ** -22           # a few float32 roundings: the least any float32 evaluation can be held to
MARGIN = 1e-4                # frames whose decisions are closer than this to flipping in the float64 oracle are not compared
CAP = 0.05                   # at most this share of a fixture's frames
STATS = (225.089, 53.78)     # the reference config's pitch_stats, passed explicitly
AMPS = (1.0, 0.5, 0.33, 0.25)
GUARD = 7.0


def speechlike(seed, L, i16=False):
    """A harmonic source on a random piecewise-linear F0 in 90-380 Hz with a 3000-sample silence, a 3000-sample 0.2 randn stretch and 0.003
    noise overall."""
    rng = np.random.default_rng(seed)
    nk = L // 8000 + 2
    f0 = np.interp(np.arange(L), np.linspace(0, L - 1, nk), rng.uniform(90.0, 380.0, nk))
    x = 0.3 * po.harmonic(f0, AMPS)
    s0, n0 = L // 14, L - 3200
    x[s0:s0 + 3000] = 0.0
    x[n0:n0 + 3000] = 0.2 * rng.standard_normal(3000)
    x += 0.003 * rng.standard_normal(L)
    if i16:
        return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    blob, man = pack_state_dict(ao.aligner_state_dict(synth_state_dict(0, "parity")))
    engs = {}
    for prec in ("mx", "strict", "fast"):
        engs[prec] = EVEngine(precision=prec, keep_stages=(prec == "mx"))
        engs[prec].load_blob(blob, man)
    fx = dict(a_l20011=speechlike(21, 20011), b_l16384_i16=speechlike(22, 16384, i16=True), c_l7000=speechlike(23, 7000))
    # the oracles once, shared and left unchanged
    o64 = {k: po.pitch64(w, stats=STATS) for k, w in fx.items()}
    o32 = {k: po.pitch64(w, dtype=np.float32, sequential=True, stats=STATS) for k, w in fx.items()}
    g = dict(np.load(os.path.join(GOLDEN_DIR, "features", "feat_a_n48_self.npz")))
    yield dict(engs=engs, fx=fx, o64=o64, o32=o32, g=g)
    for e in engs.values():
        e.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _utt(g):
    return dict(ling=g["in_ling"], speaker=int(g["in_speaker"]), style=g["in_style"], content=g["in_content"])


def _yin_op(wavs, cfg=None):
    """ev_op_pitch_yin on guarded buffers: per utterance (f0, aperiodicity, tau)."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.pitch import PitchConfig
    cfg = cfg or PitchConfig()
    is16 = wavs[0].dtype == np.int16
    lens = np.array([len(w) for w in wavs], np.int64)
    Ts = [int(n) // cfg.hop + 1 for n in lens]
    TT = sum(Ts)
    d_wav = torch.from_numpy(np.concatenate(wavs).astype(np.int16 if is16 else np.float32)).cuda()
    d_f0 = torch.full((TT + 64,), GUARD, device="cuda")
    d_ap = torch.full((TT + 64,), GUARD, device="cuda")
    d_tau = torch.full((TT + 64,), 77, device="cuda", dtype=torch.int32)
    torch.cuda.synchronize()
    rc = _ffi.lib().ev_op_pitch_yin(d_wav.data_ptr(), 1 if is16 else 0, len(wavs), lens.ctypes.data_as(C.c_void_p), cfg.sample_rate, cfg.hop, cfg.win,
                                    cfg.f_min, cfg.f_max, cfg.threshold, cfg.silence_rms, d_f0.data_ptr(), d_ap.data_ptr(), d_tau.data_ptr(), None)
    assert rc == 0
    f0, ap, tau = d_f0.cpu().numpy(), d_ap.cpu().numpy(), d_tau.cpu().numpy()
    assert (f0[TT:] == GUARD).all() and (ap[TT:] == GUARD).all() and (tau[TT:] == 77).all()      # nothing written past the packed outputs
    assert (f0[:TT] != GUARD).all() and (ap[:TT] != GUARD).all() and (tau[:TT] != 77).all()      # and every frame written
    outs, o = [], 0
    for T in Ts:
        outs.append((f0[o:o + T], ap[o:o + T], tau[o:o + T]))
        o += T
    return outs


def _fill_op(f0s, mean=0.0, std=1.0):
    from emotivoice_amd import _ffi
    frames = np.array([len(f) for f in f0s], np.int32)
    TT = int(frames.sum())
    d_f0 = torch.from_numpy(np.concatenate(f0s).astype(np.float32)).cuda()
    d_out = torch.full((TT + 64,), GUARD, device="cuda")
    torch.cuda.synchronize()
    rc = _ffi.lib().ev_op_pitch_fill(d_f0.data_ptr(), len(f0s), frames.ctypes.data_as(C.c_void_p), mean, std, d_out.data_ptr(), None)
    assert rc == 0
    out = d_out.cpu().numpy()
    assert (out[TT:] == GUARD).all()
    offs = np.concatenate([[0], np.cumsum(frames)])
    return [out[offs[b]:offs[b + 1]] for b in range(len(f0s))]


def _compare(name, f0, ap, tau, pitch, o64, o32, bad):
    """The accuracy criterion for one utterance; appends what misses to ``bad`` and returns the frames compared."""
    T = o64["f0"].size
    keep = o64["margin"] >= MARGIN
    left_out = int((~keep).sum())
    assert left_out <= CAP * T, (name, left_out, T)
    assert np.array_equal(o32["tau"][keep], o64["tau"][keep]), name          # the yardstick decides as the float64 oracle does
    assert np.array_equal((f0 > 0)[keep], o64["voiced"][keep]), name
    assert np.array_equal(tau[keep], o64["tau"][keep]), name
    assert (f0[tau < 0] == 0).all() and (ap[tau < 0] == 1.0).all() and (f0[tau >= 0] > 0).all()
    kv = keep & o64["voiced"]
    rows = []
    e_ref, e_dev = po.rel_error(o32["f0"][kv], o64["f0"][kv]), po.rel_error(f0[kv], o64["f0"][kv])
    checks = [("f0", e_ref, e_dev),
              ("aperiodicity", po.abs_error(o32["aperiodicity"][keep], o64["aperiodicity"][keep]), po.abs_error(ap[keep], o64["aperiodicity"][keep]))]
    if pitch is not None:
        # the continuous track of an unvoiced frame takes its value from its voiced neighbours: where a frame that is left out decides
        # differently on the device, only the voiced frames (whose track is their own F0) are comparable
        kp = keep if np.array_equal(f0 > 0, o64["voiced"]) and np.array_equal(o32["voiced"], o64["voiced"]) else kv
        checks.append(("pitch", po.abs_error(o32["pitch"][kp], o64["pitch"][kp]), po.abs_error(pitch[kp], o64["pitch"][kp])))
    for what, e_ref, e_dev in checks:
        rows.append("%s E(f32) %.3e E(dev) %.3e" % (what, e_ref, e_dev))
        if not e_dev <= 4 * max(e_ref, FLOOR):
            bad.append((name, what, e_ref, e_dev))
    print(name, "T %d left out %d voiced %d |" % (T, left_out, int(kv.sum())), " | ".join(rows))
    return keep


def test_accuracy_against_the_float64_oracle(ctx):
    """On the frames whose float64 decisions have a margin >= 1e-4 (at least 95 % of a fixture): voicing and lag equal the oracle's, and for f0
    (relative), aperiodicity (absolute) and pitch (absolute, standardised units) E(device) <= 4 max(E(float32 sequential oracle), 2^-22), both
    against float64.  The continuous track equals the oracle's fill of the device's own f0_hz to 1e-6."""
    eng = ctx["engs"]["mx"]
    bad = []
    for name, w in ctx["fx"].items():
        out = eng.pitch([w], pitch_stats=STATS)
        f0, ap, pitch = out["f0_list"][0], out["aperiodicity_list"][0], out["pitch_list"][0]
        (f0_op, ap_op, tau), = _yin_op([w])
        assert np.array_equal(_bits(f0_op), _bits(f0)) and np.array_equal(_bits(ap_op), _bits(ap)), name
        assert out["mel_lens"][0] == len(w) // 256 + 1 == f0.size
        assert 0 < (f0 > 0).sum() < f0.size and (len(w) < 16000 or (f0 > 0).sum() >= 0.3 * f0.size), name      # voiced and unvoiced stretches
        _compare(name, f0, ap, tau, pitch, ctx["o64"][name], ctx["o32"][name], bad)
        cont = eng.pitch([w])["pitch_list"][0]                           # stats (0, 1): the continuous track in Hz
        np.testing.assert_allclose(cont, po.fill(f0), rtol=1e-6, atol=0, err_msg=name)
        assert np.array_equal(_bits(pitch), _bits(po.standardise(cont, *STATS))), name
    assert not bad, bad


def test_ground_truth_on_the_device(ctx):
    """The kernel itself on signals of known F0 (a kernel that agrees with a wrong oracle still fails here): steady tones within 1e-3 on every
    interior frame, the 110 -> 330 Hz glide within 1e-2, a missing fundamental found, noise and silence unvoiced."""
    eng = ctx["engs"]["mx"]
    tones = [80.5, 100.0, 133.3, 220.0, 311.0, 399.0]
    n = 8000
    wavs = [(0.3 * po.harmonic(np.full(n, f), AMPS)).astype(np.float32) for f in tones]
    wavs.append((0.3 * po.harmonic(np.linspace(110.0, 330.0, 16000), AMPS)).astype(np.float32))
    wavs.append((0.3 * po.harmonic(np.full(n, 120.0), (0.0, 1.0, 0.7, 0.5))).astype(np.float32))
    wavs.append((0.3 * np.random.default_rng(5).standard_normal(n)).astype(np.float32))
    wavs.append(np.zeros(5000, np.float32))
    out = eng.pitch(wavs)
    for f, f0 in zip(tones + [120.0], out["f0_list"][:6] + [out["f0_list"][7]]):
        inner = f0[3:-3]
        err = np.abs(inner.astype(np.float64) - f).max() / f
        print(f, "worst relative error %.2e" % err)
        assert (inner > 0).all() and err <= 1e-3, (f, err)
    g = out["f0_list"][6].astype(np.float64)
    truth = 110.0 + 220.0 * np.minimum(np.arange(g.size) * 256, 15999) / 15999
    err = (np.abs(g - truth) / truth)[3:-3].max()
    print("glide worst relative error %.2e" % err)
    assert (g[3:-3] > 0).all() and err <= 1e-2, err
    assert (out["f0_list"][8] == 0).all() and (out["f0_list"][9] == 0).all() and (out["aperiodicity_list"][9] == 1.0).all()
    assert (out["pitch_list"][9] == 0).all()


def test_batch_position_and_int16_invariance(ctx):
    eng = ctx["engs"]["mx"]
    fx = ctx["fx"]
    a = fx["a_l20011"][:7000].copy()          # silence, then a voiced stretch
    rng = np.random.default_rng(3)
    tone = (0.3 * po.harmonic(np.full(20000, 177.0), AMPS)).astype(np.float32)
    others = [tone[:1], tone[:255], tone[:256], tone[:777], (0.2 * rng.standard_normal(3000)).astype(np.float32)]
    batch = [a, others[0], others[1], a, others[2], others[3], others[4], a]
    out = eng.pitch(batch, pitch_stats=STATS)
    assert out["mel_lens"].tolist() == [28, 1, 1, 28, 2, 4, 12, 28]
    alone = eng.pitch([a], pitch_stats=STATS)
    keys = ("pitch_list", "f0_list", "aperiodicity_list")
    for pos in (0, 3, 7):
        for k in keys:
            assert np.array_equal(_bits(out[k][pos]), _bits(alone[k][0])), (pos, k)
    for j, w in zip((1, 2, 4, 5, 6), others):
        one = eng.pitch([w], pitch_stats=STATS)
        for k in keys:
            assert np.array_equal(_bits(out[k][j]), _bits(one[k][0])), (j, k)
    # the 777-sample tone is voiced somewhere, so the tiny utterances are not trivially equal
    assert (out["f0_list"][5] > 0).any()
    i16 = fx["b_l16384_i16"]
    as_float = i16.astype(np.float32) / np.float32(32768.0)
    oi, of = eng.pitch([i16], pitch_stats=STATS), eng.pitch([as_float], pitch_stats=STATS)
    for k in keys:
        assert np.array_equal(_bits(oi[k][0]), _bits(of[k][0])), k


def test_precision_mode_and_device_input_invariance(ctx):
    from emotivoice_amd import _ffi
    wavs = [ctx["fx"]["c_l7000"], ctx["fx"]["a_l20011"]]
    ref = ctx["engs"]["mx"].pitch(wavs, pitch_stats=STATS)
    keys = ("pitch_list", "f0_list", "aperiodicity_list")
    for prec in ("strict", "fast"):
        out = ctx["engs"][prec].pitch(wavs, pitch_stats=STATS)
        for b in range(2):
            for k in keys:
                assert np.array_equal(_bits(out[k][b]), _bits(ref[k][b])), (prec, k)
    eng = ctx["engs"]["mx"]
    flat = torch.from_numpy(np.concatenate(wavs)).cuda()
    torch.cuda.synchronize()
    res = eng.pitch_raw(2, flat.data_ptr(), False, np.array([len(w) for w in wavs], np.int64), STATS[0], STATS[1], None, flags=_ffi.EV_FLAG_DEVICE_INPUTS)
    dev = eng.pitch_to_numpy(res)
    for b in range(2):
        for k in keys:
            assert np.array_equal(_bits(dev[k][b]), _bits(ref[k][b])), k


def test_op_pitch_yin_at_its_edges(ctx):
    """T = 1, an utterance shorter than win, T = one frame more than the kernel's tile, a batch whose last tile is partial, and a second config."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.pitch import PitchConfig
    TF = _ffi.EV_PITCH_TILE_FRAMES
    rng = np.random.default_rng(11)

    def sig(L, f=150.0):
        return (0.3 * po.harmonic(np.full(L, f), AMPS) + 0.003 * rng.standard_normal(L)).astype(np.float32)
    c2 = PitchConfig(hop=128, win=512, f_min=100.0, f_max=500.0).validate()
    cases = [("T1", [sig(100)], None), ("shorter_than_win", [sig(700, 210.0)], None), ("tile_plus_one", [sig(TF * 256 + 3, 97.0)], None),
             ("partial_last_tile", [sig(TF * 256 + 5, 301.0), np.zeros(300, np.float32), sig(11 * 256 + 1, 123.0)], None),
             ("second_config", [sig(5000, 333.0), sig(129, 140.0)], c2)]
    bad = []
    for name, wavs, cfg in cases:
        outs = _yin_op(wavs, cfg)
        for w, (f0, ap, tau) in zip(wavs, outs):
            assert f0.size == len(w) // (cfg.hop if cfg else 256) + 1
            _compare("%s/%d" % (name, len(w)), f0, ap, tau, None, po.pitch64(w, cfg), po.pitch64(w, cfg, dtype=np.float32, sequential=True), bad)
    assert _yin_op(cases[0][1])[0][0].shape == (1,) and _yin_op(cases[2][1])[0][0].shape == (TF + 1,)
    assert (_yin_op(cases[3][1])[1][0] == 0).all()
    assert (_yin_op(cases[4][1], c2)[0][0][5:-5] > 0).all()
    assert not bad, bad
    # what ev_pitch rejects is -2 here
    d = torch.zeros(1024, device="cuda")
    lens = np.array([512], np.int64)
    lib = _ffi.lib()
    for kw in (dict(hop=0), dict(win=4096), dict(f_min=10.0), dict(threshold=0.0)):
        a = dict(sample_rate=16000, hop=256, win=1024, f_min=80.0, f_max=400.0, threshold=0.15, silence_rms=1e-3)
        a.update(kw)
        rc = lib.ev_op_pitch_yin(d.data_ptr(), 0, 1, lens.ctypes.data_as(C.c_void_p), a["sample_rate"], a["hop"], a["win"], a["f_min"], a["f_max"],
                                 a["threshold"], a["silence_rms"], d.data_ptr(), d.data_ptr() + 2048, None, None)
        assert rc == -2, kw


def test_op_pitch_fill_on_hand_made_tracks(ctx):
    rng = np.random.default_rng(4)

    def pattern(T, p):
        return np.where(rng.random(T) < p, rng.uniform(80.0, 400.0, T), 0.0).astype(np.float32)
    mid = np.zeros(40, np.float32); mid[23] = 200.0
    first = np.zeros(70, np.float32); first[0] = 111.0
    last = np.zeros(70, np.float32); last[-1] = 333.0
    alt = np.zeros(131, np.float32); alt[::2] = rng.uniform(80.0, 400.0, 66)
    gap = np.zeros(1025, np.float32); gap[3], gap[1000] = 90.0, 380.0           # one interpolation across many 64-frame chunks
    f0s = [np.zeros(12, np.float32), mid, first, last, alt, np.array([0.0], np.float32), np.array([250.0], np.float32),
           pattern(64, 0.5), pattern(65, 0.5), pattern(1025, 0.2), pattern(1025, 0.02), gap, np.zeros(1025, np.float32)]
    for mean, std in ((0.0, 1.0), STATS):
        outs = _fill_op(f0s, mean, std)
        for f0, got in zip(f0s, outs):
            cont = po.fill(f0)
            want = po.standardise(cont, mean, std)
            scale = np.abs(cont).astype(np.float64) / std + 1e-30
            assert (np.abs(got.astype(np.float64) - want) <= 1e-6 * np.maximum(scale, abs(mean) / std)).all(), (f0.size, mean)
            held = (f0 > 0) | (np.arange(f0.size) < (np.nonzero(f0 > 0)[0].min() if (f0 > 0).any() else 0)) | \
                   (np.arange(f0.size) > (np.nonzero(f0 > 0)[0].max() if (f0 > 0).any() else f0.size))
            assert np.array_equal(_bits(got[held]), _bits(want[held])), f0.size     # voiced frames and the edge holds are copies: exact
    assert np.array_equal(outs[0], po.standardise(np.zeros(12, np.float32), *STATS))
    from emotivoice_amd import _ffi
    d = torch.zeros(64, device="cuda")
    fr = np.array([8], np.int32)
    assert _ffi.lib().ev_op_pitch_fill(d.data_ptr(), 1, fr.ctypes.data_as(C.c_void_p), 0.0, 1.0, d.data_ptr(), None) == -2      # in place
    assert _ffi.lib().ev_op_pitch_fill(d.data_ptr(), 1, fr.ctypes.data_as(C.c_void_p), 0.0, 0.0, d.data_ptr() + 128, None) == -2
    fr0 = np.array([0], np.int32)
    assert _ffi.lib().ev_op_pitch_fill(d.data_ptr(), 1, fr0.ctypes.data_as(C.c_void_p), 0.0, 1.0, d.data_ptr() + 128, None) == -2


def test_rejections_then_a_valid_call(ctx):
    """Every rejection by needle in ev_last_error, each followed by a good call that gives the bits of an untouched handle.  The fresh handle has
    neither weights nor a feature setup."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine
    lib = _ffi.lib()
    wav = ctx["fx"]["a_l20011"][:7000].copy()
    want = ctx["engs"]["mx"].pitch([wav], pitch_stats=STATS)
    fresh = EVEngine(precision="mx")
    try:
        def call(lens=(7000,), mean=STATS[0], std=STATS[1], size=None, cfg_size=None, **kw):
            c = _ffi.ev_pitch_config()
            lib.ev_default_pitch_config(C.byref(c))
            assert (c.struct_size, c.sample_rate, c.hop, c.win) == (C.sizeof(c), 16000, 256, 1024)
            for k, v in kw.items():
                setattr(c, k, v)
            if cfg_size is not None:
                c.struct_size = cfg_size
            r = _ffi.ev_pitch_result()
            r.struct_size = C.sizeof(r) if size is None else size
            wl = np.asarray(lens, np.int64)
            rc = lib.ev_pitch(fresh._h, len(wl), wav.ctypes.data_as(C.c_void_p), 0, wl.ctypes.data_as(C.c_void_p), C.byref(c), mean, std, 0, C.byref(r))
            return rc, lib.ev_last_error(fresh._h).decode()
        nan, inf = float("nan"), float("inf")
        for kw, needle in ((dict(size=40), "struct_size"), (dict(cfg_size=28), "struct_size"), (dict(lens=[100, 0]), "wav_lens[1]"),
                           (dict(lens=[16384 * 256]), "EV_ALIGN_MAX_FRAMES"), (dict(hop=0), "hop"), (dict(hop=1025), "hop"), (dict(win=4096), "win"),
                           (dict(win=2048, hop=2048), "EV_PITCH_MAX_LDS"), (dict(f_min=nan), "f_min"), (dict(f_max=inf), "f_max"), (dict(f_min=0.0), "f_min"),
                           (dict(f_min=400.0), "f_min"), (dict(f_max=4000.5), "f_max"), (dict(f_min=10.0), "tau_max"), (dict(threshold=0.0), "threshold"),
                           (dict(threshold=1.01), "threshold"), (dict(threshold=nan), "threshold"), (dict(silence_rms=-1e-3), "silence_rms"),
                           (dict(silence_rms=inf), "silence_rms"), (dict(mean=nan), "pitch_mean"), (dict(mean=inf), "pitch_mean"),
                           (dict(std=0.0), "pitch_std"), (dict(std=-1.0), "pitch_std"), (dict(std=nan), "pitch_std"), (dict(std=inf), "pitch_std")):
            rc, msg = call(**kw)
            assert rc < 0 and needle in msg, (kw, msg)
            ok = fresh.pitch([wav], pitch_stats=STATS)
            for k in ("pitch_list", "f0_list", "aperiodicity_list"):
                assert np.array_equal(_bits(ok[k][0]), _bits(want[k][0])), (kw, k)
        rc, msg = call()
        assert rc == 0, msg
    finally:
        fresh.close()


def test_result_survives_the_other_calls(ctx):
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["engs"]["mx"]
    g = ctx["g"]
    wl = np.array([g["wav"].size], np.int64)
    res = eng.pitch_raw(1, g["wav"].ctypes.data, False, wl, STATS[0], STATS[1])
    before = eng.pitch_to_numpy(res)
    f = eng.features([g["wav"]])
    eng.align([_utt(g)], f["mel_list"], energy=f["energy_list"])
    syn = eng.synthesize(synth_inputs(9, [40]))
    eng.vocoder([np.ascontiguousarray(f["mel_list"][0])])
    after = eng.pitch_to_numpy(res)
    for k in ("pitch", ):
        assert np.array_equal(_bits(before[k]), _bits(after[k]))
    for k in ("f0_list", "aperiodicity_list"):
        assert np.array_equal(_bits(before[k][0]), _bits(after[k][0]))
    assert np.isfinite(syn["wav"]).all() and before["mel_lens"][0] == f["mel_lens"][0]


def test_wav_to_pitch_transfer_end_to_end(ctx):
    """align_recordings(pitch_stats=...) gives the per-token means of ev_pitch's track over the aligned spans and leaves durations and score
    untouched; transfer_from_recordings then synthesises with exactly those values, and without pitch_stats (or pitch=False) with the predictor's."""
    from emotivoice_amd.alignment import align_recordings, transfer_from_recordings
    eng = ctx["engs"]["mx"]
    g = ctx["g"]
    utt, dst = _utt(g), dict(_utt(g), speaker=33)
    plain = align_recordings(eng, [utt], [g["wav"]], energy_stats=(0.0, 1.0))
    assert plain["pitch"] is None
    out = align_recordings(eng, [utt], [g["wav"]], energy_stats=(0.0, 1.0), pitch_stats=STATS)
    track = eng.pitch([g["wav"]], pitch_stats=STATS)["pitch_list"][0]
    assert track.size == int(out["mel_lens"][0]) and (eng.pitch([g["wav"]])["f0_list"][0] >= 0).all()
    want = ao.average_by_duration(out["durations"], track)
    assert np.array_equal(_bits(out["pitch"]), _bits(want))
    assert np.array_equal(out["durations"], plain["durations"]) and np.array_equal(_bits(out["score"]), _bits(plain["score"]))
    assert np.array_equal(_bits(out["energy"]), _bits(plain["energy"]))
    tr = transfer_from_recordings(eng, [utt], [g["wav"]], [dst], energy_stats=(0.0, 1.0), pitch_stats=STATS, vocoder=False)
    assert np.array_equal(_bits(eng.get_stage("pitch_eff")), _bits(want))
    assert tr["mel_lens"][0] == int(out["durations"].sum()) and np.array_equal(_bits(tr["alignment"]["pitch"]), _bits(want))
    eng.synthesize([dst], vocoder=False)
    predicted = eng.get_stage("pitch_eff").copy()
    assert not np.array_equal(predicted, want)
    for kw in (dict(pitch_stats=STATS, pitch=False), dict()):
        tr = transfer_from_recordings(eng, [utt], [g["wav"]], [dst], energy_stats=(0.0, 1.0), vocoder=False, **kw)
        assert tr["alignment"]["pitch"] is None and np.array_equal(_bits(eng.get_stage("pitch_eff")), _bits(predicted)), kw
