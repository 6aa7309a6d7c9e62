"""MI355X: ev_features -- wav -> mel, energy on the device (include/evhip.h).  Accuracy against the float64 oracle with the reference's own
float32 error as the yardstick (tests/golden/features/feat_*.npz), bit invariance (batch position, int16 / float, precision mode, host / device
input), wav -> alignment end to end against the reference's teacher-forced forward, rejections, lifetime, and the kernel at its edges."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import align_oracle as ao
import features_oracle as fo
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FEAT_DIR = os.path.join(GOLDEN_DIR, "features")
FIXTURES = sorted(glob.glob(os.path.join(FEAT_DIR, "feat_*.npz")))
FLOOR = 2.0 ** -22           # the truncation class of the split-precision product
CLAMP = np.float32(np.log(np.float32(1e-5)))


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
        engs[prec].features_setup()
    gs = {os.path.basename(p)[:-4]: dict(np.load(p)) for p in FIXTURES}
    assert len(gs) == 5
    yield dict(engs=engs, gs=gs)
    for e in engs.values():
        e.close()


def _utt(g):
    return dict(ling=g["in_ling"], speaker=int(g["in_speaker"]), style=g["in_style"], content=g["in_content"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_accuracy_against_the_float64_oracle(ctx):
    """E(device) <= 4 max(E(reference), 2^-22) for mel, energy and feat_mag, per fixture; sure clamps are clamped."""
    eng = ctx["engs"]["mx"]
    bad = []
    for name, g in ctx["gs"].items():
        o = fo.features64(g["wav"])
        out = eng.features([g["wav"]])
        mel, en = out["mel_list"][0], out["energy_list"][0]
        mag = eng.get_stage("feat_mag").reshape(-1, 513)
        assert mel.shape == g["ref_mel"].shape and en.shape == g["ref_energy"].shape and mag.shape == o["mag"].shape and out["mel_lens"][0] == mel.shape[1]
        rows = []
        for what, e_ref, e_dev in (("mel", fo.mel_error(g["ref_mel"], o["mel"]), fo.mel_error(mel, o["mel"])),
                                   ("energy", fo.energy_error(g["ref_energy"], o["energy"]), fo.energy_error(en, o["energy"])),
                                   ("mag", fo.mag_error(g["ref_mag"], o["mag"][g["mag_frames"]]), fo.mag_error(mag[g["mag_frames"]], o["mag"][g["mag_frames"]]))):
            rows.append("%s E(ref) %.3e E(dev) %.3e" % (what, e_ref, e_dev))
            if not e_dev <= 4 * max(e_ref, FLOOR):
                bad.append((name, what, e_ref, e_dev))
        print(name, " | ".join(rows))
        # the fixture's magnitudes cover the frames mag_frames (today: all of them); frames outside that set have no reference yardstick
        rest = np.setdiff1d(np.arange(mag.shape[0]), g["mag_frames"])
        if rest.size and not fo.mag_error(mag[rest], o["mag"][rest]) <= 4 * FLOOR:
            bad.append((name, "mag outside mag_frames", FLOOR, fo.mag_error(mag[rest], o["mag"][rest])))
        sure = o["mel_lin"] < 0.5e-5
        assert np.all(mel[sure] == CLAMP), name
        floor = (o["mag"] ** 2).sum(axis=1) < 0.5e-10
        assert np.all(en[floor] == np.float32(1e-5)), name
    assert not bad, bad


def test_batch_position_and_int16_invariance(ctx):
    eng = ctx["engs"]["mx"]
    gs = ctx["gs"]
    a = gs["feat_a_n48_self"]["wav"]
    alone = eng.features([a])
    rng = np.random.default_rng(3)
    others = [gs["feat_c_chirp_zeros"]["wav"], gs["feat_d_l513"]["wav"], gs["feat_d_l20011"]["wav"],
              (0.2 * rng.standard_normal(16384)).astype(np.float32), (0.2 * rng.standard_normal(777)).astype(np.float32)]
    batch = [a, others[0], others[1], a, others[2], others[3], others[4], a]
    out = eng.features(batch)
    assert out["mel_lens"].tolist() == [len(w) // 256 + 1 for w in batch]
    for pos in (0, 3, 7):
        assert np.array_equal(_bits(out["mel_list"][pos]), _bits(alone["mel_list"][0])), pos
        assert np.array_equal(_bits(out["energy_list"][pos]), _bits(alone["energy_list"][0])), pos
    for j, w in zip((1, 2, 4), others[:3]):
        one = eng.features([w])
        assert np.array_equal(_bits(out["mel_list"][j]), _bits(one["mel_list"][0])), j
    i16 = gs["feat_b_n48_self_i16"]["wav"]
    as_float = i16.astype(np.float32) / np.float32(32768.0)
    oi, of = eng.features([i16]), eng.features([as_float])
    assert np.array_equal(_bits(oi["mel_list"][0]), _bits(of["mel_list"][0])) and np.array_equal(_bits(oi["energy_list"][0]), _bits(of["energy_list"][0]))


def test_precision_mode_and_device_input_invariance(ctx):
    from emotivoice_amd import _ffi
    gs = ctx["gs"]
    wavs = [gs["feat_a_n48_self"]["wav"], gs["feat_d_l20011"]["wav"]]
    ref = ctx["engs"]["mx"].features(wavs, energy_stats=(0.25, 2.0))
    for prec in ("strict", "fast"):
        out = ctx["engs"][prec].features(wavs, energy_stats=(0.25, 2.0))
        for b in range(2):
            assert np.array_equal(_bits(out["mel_list"][b]), _bits(ref["mel_list"][b])), prec
            assert np.array_equal(_bits(out["energy_list"][b]), _bits(ref["energy_list"][b])), prec
    raw = ctx["engs"]["mx"].features(wavs)
    assert np.array_equal(ref["energy_list"][0], (raw["energy_list"][0] - np.float32(0.25)) / np.float32(2.0))
    eng = ctx["engs"]["mx"]
    flat = torch.from_numpy(np.concatenate(wavs)).cuda()
    torch.cuda.synchronize()
    res = eng.features_raw(2, flat.data_ptr(), False, np.array([len(w) for w in wavs], np.int64), 0.25, 2.0, flags=_ffi.EV_FLAG_DEVICE_INPUTS)
    dev = eng.features_to_numpy(res)
    for b in range(2):
        assert np.array_equal(_bits(dev["mel_list"][b]), _bits(ref["mel_list"][b])) and np.array_equal(_bits(dev["energy_list"][b]), _bits(ref["energy_list"][b]))


def test_wav_to_alignment_end_to_end(ctx):
    """Case (a): align_recordings on the wav gives the reference's duration_targets exactly and its -bin_loss within 1e-4."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.alignment import align_recordings
    g = ctx["gs"]["feat_a_n48_self"]
    assert float(g["min_margin"]) >= 1e-4          # checked by the generator on the reference's own log_p_attn
    for prec in ("mx", "strict"):
        eng = ctx["engs"][prec]
        out = align_recordings(eng, [_utt(g)], [g["wav"]], energy_stats=(0.0, 1.0))
        print(prec, "score", out["score"][0], "-bin_loss", -float(g["bin_loss"]))
        assert np.array_equal(out["durations"], g["duration_targets"]), prec
        assert abs(float(out["score"][0]) + float(g["bin_loss"])) <= 1e-4, prec
        assert out["pitch"] is None and out["energy"].shape == g["duration_targets"].shape
    # the same mel through the host: the same bits
    eng = ctx["engs"]["mx"]
    dev = align_recordings(eng, [_utt(g)], [g["wav"]], energy_stats=(0.0, 1.0))
    lp_dev = eng.get_stage("log_p_attn").copy()
    f = eng.features([g["wav"]])
    host = eng.align([_utt(g)], f["mel_list"], energy=f["energy_list"])
    lp_host = eng.get_stage("log_p_attn")
    assert np.array_equal(_bits(lp_dev), _bits(lp_host))
    assert np.array_equal(dev["durations"], host["durations"]) and np.array_equal(_bits(dev["score"]), _bits(host["score"]))
    assert np.array_equal(_bits(dev["energy"]), _bits(host["energy"]))
    # the per-token energy is the mean of the device's frame energy over the aligned spans
    assert np.array_equal(dev["energy"], ao.average_by_duration(dev["durations"], f["energy_list"][0]))
    from emotivoice_amd.alignment import transfer_from_recordings
    dst = dict(_utt(g), speaker=33)
    tr = transfer_from_recordings(eng, [_utt(g)], [g["wav"]], [dst], energy_stats=(0.0, 1.0))
    assert tr["mel_lens"][0] == int(g["duration_targets"].sum()) and np.isfinite(tr["wav"]).all()


def test_rejections_then_a_valid_call(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine, EVError
    from emotivoice_amd.features import mel_filterbank
    lib = _ffi.lib()
    g = ctx["gs"]["feat_d_l513"]
    fresh = EVEngine(precision="mx")
    try:
        with pytest.raises(EVError, match="ev_features_setup"):
            fresh.features_raw(1, g["wav"].ctypes.data, False, np.array([513], np.int64))
        mb = mel_filterbank()

        def setup(**kw):
            c = _ffi.ev_features_config()
            lib.ev_default_features_config(C.byref(c))
            c.mel_basis = mb.ctypes.data
            for k, v in kw.items():
                setattr(c, k, v)
            rc = lib.ev_features_setup(fresh._h, C.byref(c))
            return rc, lib.ev_last_error(fresh._h).decode()
        for kw, needle in ((dict(struct_size=36), "struct_size"), (dict(n_fft=1000), "n_fft"), (dict(n_fft=4096), "n_fft"), (dict(n_mels=129), "n_mels"),
                           (dict(hop=100), "hop"), (dict(mel_basis=None), "mel_basis")):
            rc, msg = setup(**kw)
            assert rc < 0 and needle in msg, (kw, msg)
        rc, msg = setup()
        assert rc == 0, msg
        fresh.feature_config = ctx["engs"]["mx"].feature_config
        wav = g["wav"]

        def call(lens, std=1.0, mean=0.0, size=None):
            r = _ffi.ev_features_result()
            r.struct_size = C.sizeof(r) if size is None else size
            wl = np.asarray(lens, np.int64)
            rc = lib.ev_features(fresh._h, len(wl), wav.ctypes.data_as(C.c_void_p), 0, wl.ctypes.data_as(C.c_void_p), mean, std, 0, C.byref(r))
            return rc, lib.ev_last_error(fresh._h).decode()
        for kw, needle in ((dict(lens=[513], size=40), "struct_size"), (dict(lens=[512]), "wav_lens[0]"), (dict(lens=[16384 * 256]), "EV_ALIGN_MAX_FRAMES"),
                           (dict(lens=[513], std=0.0), "energy_std"), (dict(lens=[513], std=-1.0), "energy_std"),
                           (dict(lens=[513], std=float("nan")), "energy_std"), (dict(lens=[513], std=float("inf")), "energy_std")):
            rc, msg = call(**kw)
            assert rc < 0 and needle in msg, (kw, msg)
            ok = fresh.features([wav])
            assert np.array_equal(_bits(ok["mel_list"][0]), _bits(ctx["engs"]["mx"].features([wav])["mel_list"][0])), kw
    finally:
        fresh.close()


def test_result_survives_synthesis_and_vocoder(ctx):
    from emotivoice_amd.synthetic import synth_inputs
    eng = ctx["engs"]["mx"]
    g = ctx["gs"]["feat_a_n48_self"]
    wl = np.array([g["wav"].size], np.int64)
    res = eng.features_raw(1, g["wav"].ctypes.data, False, wl)
    before = eng.features_to_numpy(res)
    syn = eng.synthesize(synth_inputs(9, [40]))
    eng.vocoder([np.ascontiguousarray(before["mel_list"][0])])
    eng.align([_utt(g)], before["mel_list"])
    after = eng.features_to_numpy(res)
    assert np.array_equal(_bits(before["mel_list"][0]), _bits(after["mel_list"][0])) and np.array_equal(_bits(before["energy"]), _bits(after["energy"]))
    assert np.isfinite(syn["wav"]).all()
    assert eng.get_stage("feat_mag").size == before["mel_lens"][0] * 513


def _op(wavs, mb, n_fft, hop, window=None, want_mag=True):
    from emotivoice_amd import _ffi
    lens = np.array([len(w) for w in wavs], np.int64)
    Ts = [int(n) // hop + 1 for n in lens]
    n_mels, n_bins, TT = mb.shape[0], n_fft // 2 + 1, sum(Ts)
    d_wav = torch.from_numpy(np.concatenate(wavs).astype(np.float32)).cuda()
    d_mel = torch.full((TT * n_mels + 64,), 7.0, device="cuda")
    d_en = torch.full((TT + 64,), 7.0, device="cuda")
    d_mag = torch.full((TT * n_bins + 64,), 7.0, device="cuda")
    torch.cuda.synchronize()
    mbc = np.ascontiguousarray(mb, np.float32)
    rc = _ffi.lib().ev_op_stft_mel(d_wav.data_ptr(), 0, len(wavs), lens.ctypes.data_as(C.c_void_p), mbc.ctypes.data_as(C.c_void_p),
                                   window.ctypes.data_as(C.c_void_p) if window is not None else None, n_fft, hop, n_mels, 1e-5, 1e-10, 0.0, 1.0,
                                   d_mel.data_ptr(), d_en.data_ptr(), d_mag.data_ptr() if want_mag else None, None)
    assert rc == 0
    mel, en, mag = d_mel.cpu().numpy(), d_en.cpu().numpy(), d_mag.cpu().numpy()
    # nothing written past the packed outputs
    assert (mel[TT * n_mels:] == 7.0).all() and (en[TT:] == 7.0).all() and (mag[TT * n_bins:] == 7.0).all()
    if not want_mag:
        assert (mag == 7.0).all()
    outs, o = [], 0
    for T in Ts:
        outs.append((mel[o * n_mels:(o + T) * n_mels].reshape(n_mels, T), en[o:o + T], mag[o * n_bins:(o + T) * n_bins].reshape(T, n_bins)))
        o += T
    return outs


def test_op_stft_mel_at_its_edges(ctx):
    """T = 1, T = 65 (a one-frame second tile), a batch whose last tile is partial, n_mels = 80 (and 20, and 128); no reference fixture here, so the
    bar is 4 * 2^-22 against the float64 oracle."""
    from emotivoice_amd.features import hann_window, mel_filterbank
    rng = np.random.default_rng(11)
    mb80 = mel_filterbank()
    cases = []
    # n_fft = hop = 128: 65 .. 127 samples are ONE frame
    mb20 = mel_filterbank(16000, 128, 20, 0.0, 8000.0)
    cases.append(("T1", [(0.4 * rng.standard_normal(100)).astype(np.float32)], mb20, 128, 128))
    cases.append(("T65", [(0.3 * rng.standard_normal(64 * 256)).astype(np.float32)], mb80, 1024, 256))
    cases.append(("partial_last_tile", [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (64 * 256 - 1, 513, 70 * 256 + 5)], mb80, 1024, 256))
    cases.append(("n_mels128", [(0.3 * rng.standard_normal(5000)).astype(np.float32)], mel_filterbank(16000, 512, 128, 0.0, 8000.0), 512, 128))
    for name, wavs, mb, n_fft, hop in cases:
        outs = _op(wavs, mb, n_fft, hop)
        for w, (mel, en, mag) in zip(wavs, outs):
            o = fo.features64(w, mb, n_fft=n_fft, hop=hop)
            assert mel.shape == o["mel"].shape, name
            e = (fo.mel_error(mel, o["mel"]), fo.energy_error(en, o["energy"]), fo.mag_error(mag, o["mag"]))
            print(name, len(w), "E mel %.3e energy %.3e mag %.3e" % e)
            assert max(e) <= 4 * FLOOR, (name, e)
    assert _op(cases[0][1], mb20, 128, 128)[0][0].shape == (20, 1)
    # an explicit window equal to the default gives the default's bits; no magnitudes requested: none written
    a = _op(cases[1][1], mb80, 1024, 256)[0]
    b = _op(cases[1][1], mb80, 1024, 256, window=hann_window(1024), want_mag=False)[0]
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
