"""CPU checks of the acoustic-feature path (ev_features): the float64 oracle against the reference's own float32 results
(tests/golden/features/feat_*.npz), the Slaney filterbank against an independent implementation, frame counts, the binding of the new
entry points and the Python-side validation."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import features_oracle as fo
from conftest import GOLDEN_DIR, ROOT

from emotivoice_amd import _ffi, features as ft

FEAT_DIR = os.path.join(GOLDEN_DIR, "features")
FIXTURES = sorted(glob.glob(os.path.join(FEAT_DIR, "feat_*.npz")))
# a float32 dot product over the 1024 samples of a frame carries a rounding error of about sqrt(1024) = 32 units of 2^-24 of its largest partial
# sum; the mel product and the float32 log add less than that again: 64 * 2^-24 bounds what the reference's float32 result may differ by
REF_F32_BOUND = 64 * 2.0 ** -24


def test_fixture_set_is_complete():
    names = [os.path.basename(p) for p in FIXTURES]
    assert names == ["feat_a_n48_self.npz", "feat_b_n48_self_i16.npz", "feat_c_chirp_zeros.npz", "feat_d_l20011.npz", "feat_d_l513.npz"]
    for p in FIXTURES:
        assert os.path.getsize(p) < 1_000_000, p
    assert np.load(FIXTURES[1])["wav"].dtype == np.int16 and np.load(FIXTURES[4])["wav"].size == 513
    assert np.load(FIXTURES[3])["wav"].size % 256 != 0
    a, b = np.load(FIXTURES[0])["wav"], np.load(FIXTURES[1])["wav"]
    assert np.array_equal(np.clip(np.round(a * 32768.0), -32768, 32767).astype(np.int16), b)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_oracle_reproduces_the_reference_features(path):
    g = np.load(path)
    o = fo.features64(g["wav"])
    T = g["wav"].size // 256 + 1
    assert g["ref_mel"].shape == (80, T) == o["mel"].shape and g["ref_energy"].shape == (T,)
    e_mel, e_en = fo.mel_error(g["ref_mel"], o["mel"]), fo.energy_error(g["ref_energy"], o["energy"])
    e_mag = fo.mag_error(g["ref_mag"], o["mag"][g["mag_frames"]])
    print(os.path.basename(path), "E_mel(ref) %.3e E_energy(ref) %.3e E_mag(ref) %.3e" % (e_mel, e_en, e_mag))
    assert e_mel <= REF_F32_BOUND and e_en <= REF_F32_BOUND and e_mag <= REF_F32_BOUND
    # the clamps: every cell the float64 result clamps with a margin of two is clamped in the reference, and likewise the energy floor
    clamp = np.float32(np.log(np.float32(1e-5)))
    sure = o["mel_lin"] < 0.5e-5
    assert np.all(np.abs(g["ref_mel"][sure] - clamp) <= 1e-6)
    floor = (o["mag"] ** 2).sum(axis=1) < 0.5e-10
    assert np.allclose(g["ref_energy"][floor], 1e-5, rtol=1e-6)


SHAPE_FIXTURES = sorted(glob.glob(os.path.join(FEAT_DIR, "stft_*.npz")))


def test_the_shape_fixtures_are_the_two_shapes():
    assert [os.path.basename(p)[:-4] for p in SHAPE_FIXTURES] == ["stft_384_48", "stft_640_320"]
    assert all(os.path.getsize(p) < 100_000 and np.load(p)["wav"].size == 2000 for p in SHAPE_FIXTURES)


@pytest.mark.parametrize("path", SHAPE_FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_oracle_reproduces_the_reference_features_at_other_shapes(path):
    """The reference's TacotronSTFT built at 384 / 48 and 640 / 320 (n_fft not a power of two): the same bound as at the default shape, whose
    sqrt(1024) covers these shorter sums."""
    g = np.load(path)
    n_fft, hop = int(g["n_fft"]), int(g["hop"])
    o = fo.features64(g["wav"], ft.mel_filterbank(16000, n_fft, 80, 0.0, 8000.0), n_fft=n_fft, hop=hop)
    T = 2000 // hop + 1
    assert g["ref_mel"].shape == (80, T) == o["mel"].shape and g["ref_mag"].shape == (T, n_fft // 2 + 1) == o["mag"].shape and g["ref_energy"].shape == (T,)
    e_mel, e_en, e_mag = fo.mel_error(g["ref_mel"], o["mel"]), fo.energy_error(g["ref_energy"], o["energy"]), fo.mag_error(g["ref_mag"], o["mag"])
    print(os.path.basename(path), "E_mel(ref) %.3e E_energy(ref) %.3e E_mag(ref) %.3e" % (e_mel, e_en, e_mag))
    assert e_mel <= REF_F32_BOUND and e_en <= REF_F32_BOUND and e_mag <= REF_F32_BOUND


def test_chirp_fixture_exercises_both_clamps():
    o = fo.features64(np.load(os.path.join(FEAT_DIR, "feat_c_chirp_zeros.npz"))["wav"])
    assert (o["mel_lin"] < 0.5e-5).sum() > 1000 and ((o["mag"] ** 2).sum(axis=1) < 0.5e-10).sum() >= 10
    assert (o["mel_lin"] > 1e-5).sum() > 1000


def test_filterbank_matches_an_independent_slaney_implementation():
    au = pytest.importorskip("transformers.audio_utils")
    for sr, n_fft, n_mels, fmin, fmax in ((16000, 1024, 80, 0.0, 8000.0), (22050, 1024, 80, 0.0, 8000.0), (16000, 512, 40, 50.0, 7600.0)):
        mine = ft.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
        theirs = au.mel_filter_bank(n_fft // 2 + 1, n_mels, fmin, fmax, sr, norm="slaney", mel_scale="slaney").T
        assert mine.shape == theirs.shape == (n_mels, n_fft // 2 + 1) and mine.dtype == np.float32
        assert np.abs(mine.astype(np.float64) - theirs).max() <= 1e-6 * theirs.max()
    fb = ft.mel_filterbank()
    assert (fb >= 0).all() and ((fb > 0).sum(axis=0) <= 2).all() and (fb.sum(axis=1) > 0).all()


def test_window_and_frame_counts():
    w = ft.hann_window(1024)
    assert w.dtype == np.float32 and w[0] == 0 and w[512] == 1 and np.array_equal(w[1:], w[1:][::-1])
    assert [ft.frames_for(n) for n in (0, 255, 256, 513, 20011, 20736)] == [1, 1, 2, 3, 79, 82]
    assert ft.frames_for(1000, hop=128) == 8
    with pytest.raises(ValueError):
        ft.frames_for(-1)
    for p in FIXTURES:
        g = np.load(p)
        assert g["ref_mel"].shape[1] == ft.frames_for(g["wav"].size)


def test_new_entry_points_are_bound_and_declared():
    """Fails on a tree without the feature: the structs, the flag and the four signatures."""
    assert _ffi.EV_FLAG_DEVICE_MEL == 16 and _ffi.EV_ABI_VERSION == 7
    for name, nargs in (("ev_default_features_config", 1), ("ev_features_setup", 2), ("ev_features", 9), ("ev_op_stft_mel", 17)):
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_ffi.lib(), name)
    assert C.sizeof(_ffi.ev_features_config) == 40 and C.sizeof(_ffi.ev_features_result) == 48
    c = _ffi.ev_features_config()
    _ffi.lib().ev_default_features_config(C.byref(c))
    assert (c.struct_size, c.n_fft, c.hop, c.n_mels) == (40, 1024, 256, 80) and c.mel_basis is None and c.window is None
    assert c.mel_clip == np.float32(1e-5) and c.energy_floor == np.float32(1e-10)
    hdr = open(os.path.join(ROOT, "include", "evhip.h")).read()
    assert "EV_FLAG_DEVICE_MEL = 16" in hdr and "typedef struct ev_features_result" in hdr
    # the limits the Python side validates against are the header's (ev_audio.cpp asserts them against the kernel's)
    import re
    for name in ("EV_FEATURES_MAX_NFFT", "EV_FEATURES_MAX_MELS", "EV_FEATURES_MAX_RUN", "EV_ALIGN_MAX_FRAMES"):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == getattr(_ffi, name), name
    assert (ft.MAX_NFFT, ft.MAX_MELS, ft.MAX_RUN, ft.MAX_FRAMES) == (_ffi.EV_FEATURES_MAX_NFFT, _ffi.EV_FEATURES_MAX_MELS, _ffi.EV_FEATURES_MAX_RUN,
                                                                     _ffi.EV_ALIGN_MAX_FRAMES)


def test_struct_sizes_match_the_c_header(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not installed")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evhip.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(ev_features_config), '
                   'sizeof(ev_features_result), offsetof(ev_features_config, mel_basis), offsetof(ev_features_result, mel_lens));return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(_ffi.ev_features_config), C.sizeof(_ffi.ev_features_result), _ffi.ev_features_config.mel_basis.offset,
                     _ffi.ev_features_result.mel_lens.offset]


def test_python_side_validation():
    ok = ft.FeatureConfig().validate()
    assert ok.n_bins == 513 and ok.tables()[0].shape == (80, 513) and ok.tables()[1] is None
    for kw, needle in ((dict(n_fft=1000), "n_fft"), (dict(n_fft=4096), "n_fft"), (dict(n_mels=129), "n_mels"), (dict(hop=100), "hop"),
                       (dict(n_fft=2048, hop=512), "64-frame tile"), (dict(mel_clip=0.0), "mel_clip"), (dict(window=np.ones(5)), "window"),
                       (dict(mel_basis=np.ones((80, 5))), "mel_basis")):
        with pytest.raises(ValueError, match=needle):
            ft.FeatureConfig(**kw).validate()
    flat, is16, lens = ft.pack_wavs([np.zeros(600, np.float64), np.ones(513, np.float32)])
    assert flat.dtype == np.float32 and not is16 and lens.tolist() == [600, 513] and lens.dtype == np.int64
    assert ft.pack_wavs([np.zeros(600, np.int16)])[1] is True
    with pytest.raises(ValueError, match=r"wavs\[1\].*513"):
        ft.pack_wavs([np.zeros(600, np.float32), np.zeros(512, np.float32)])
    with pytest.raises(ValueError, match="mixed"):
        ft.pack_wavs([np.zeros(600, np.float32), np.zeros(600, np.int16)])
    with pytest.raises(ValueError, match="EV_ALIGN_MAX_FRAMES"):
        ft.pack_wavs([np.zeros(16384 * 256, np.int16)])
    with pytest.raises(ValueError, match="no utterances"):
        ft.pack_wavs([])
    from emotivoice_amd import alignment
    with pytest.raises(ValueError, match="2 wavs for 1"):
        alignment.align_recordings(None, [dict(ling=[1])], [np.zeros(600), np.zeros(600)])
    with pytest.raises(ValueError, match="phonemes"):
        alignment.transfer_from_recordings(None, [dict(ling=[1, 2])], [np.zeros(600)], [dict(ling=[1, 3])])


def test_setup_and_call_reject_a_null_handle_without_a_device():
    lib = _ffi.lib()
    c = _ffi.ev_features_config()
    lib.ev_default_features_config(C.byref(c))
    assert lib.ev_features_setup(None, C.byref(c)) < 0
    r = _ffi.ev_features_result()
    assert lib.ev_features(None, 1, None, 0, None, 0.0, 1.0, 0, C.byref(r)) < 0
    # the per-kernel entry point refuses shapes before it touches the device
    lens = np.array([513], np.int64)
    mb = ft.mel_filterbank()
    dummy = C.c_void_p(16)
    def op(n_fft=1024, hop=256, n_mels=80, B=1, lens=lens):
        return lib.ev_op_stft_mel(dummy, 0, B, lens.ctypes.data_as(C.c_void_p), mb.ctypes.data_as(C.c_void_p), None, n_fft, hop, n_mels,
                                  1e-5, 1e-10, 0.0, 1.0, dummy, dummy, None, None)
    assert op(n_fft=1000) == -2 and op(n_fft=4096) == -2 and op(hop=100) == -2 and op(n_mels=129) == -2 and op(n_mels=0) == -2
    assert op(B=0) == -2 and op(lens=np.array([512], np.int64)) == -2 and op(lens=np.array([16384 * 256], np.int64)) == -2
