"""Forced alignment without a GPU: the restated aligner / MAS (tests/align_oracle.py) against the reference's own teacher-forced forward
(tests/golden/align/aln_*.npz, tests/golden/make_golden_align.py), hand-made MAS cases, the packer's aln.* entries, the ev_align ABI surface and
the emotivoice_amd.alignment helpers."""
import ctypes as C
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import align_oracle as ao
from conftest import GOLDEN_DIR, ROOT

from emotivoice_amd import _ffi
from emotivoice_amd.alignment import prosody_from_alignment, timestamps, transfer
from emotivoice_amd.packer import MEL_PAD, pack_state_dict
from emotivoice_amd.prosody import MAX_DURATION

# in a directory of their own: the parity tests take every tests/golden/*.npz as an inference fixture
ALIGN_DIR = os.path.join(GOLDEN_DIR, "align")
FIXTURES = sorted(glob.glob(os.path.join(ALIGN_DIR, "aln_*.npz")))


@pytest.fixture(scope="module")
def sd():
    from emotivoice_amd.synthetic import synth_state_dict
    return ao.aligner_state_dict(synth_state_dict(0, "parity"))


def test_fixtures_exist():
    assert len(FIXTURES) == 4, FIXTURES
    for f in FIXTURES:
        assert os.path.getsize(f) < (1 << 20), f


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_restated_aligner_reproduces_the_reference(sd, path):
    g = np.load(path)
    lp = ao.log_p_attn(sd, g["x_proj"], g["in_mel"])
    assert lp.shape == g["log_p_attn"].shape
    np.testing.assert_allclose(lp, g["log_p_attn"], rtol=0, atol=1e-5)
    # MAS on the reference's own log_p: exact durations, exact (1e-6) averages
    A = ao.mas(g["log_p_attn"])
    d = ao.durations(A, g["log_p_attn"].shape[1])
    assert np.array_equal(d, g["duration_targets"])
    assert d.min() >= 1 and d.sum() == g["in_mel"].shape[1]
    np.testing.assert_allclose(ao.average_by_duration(d, g["in_pitch_frames"]), g["pitch_targets"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ao.average_by_duration(d, g["in_energy_frames"]), g["energy_targets"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ao.path_score(g["log_p_attn"], A), -g["bin_loss"], rtol=1e-6)
    assert np.array_equal(ao.mas_fast(g["log_p_attn"]), A)


def test_tn_case_gives_every_token_one_frame():
    g = np.load(os.path.join(ALIGN_DIR, "aln_n24_tn.npz"))
    assert np.array_equal(g["duration_targets"], np.ones(24, np.int64))


def test_mas_ties_take_the_earlier_token():
    # every entry equal: every comparison is a tie, so the backtrack drops a token at every frame it can (>=)
    lp = np.zeros((6, 3), np.float32)
    A = ao.mas(lp)
    assert A.tolist() == [0, 0, 0, 0, 1, 2]
    assert np.array_equal(ao.mas_fast(lp), A)
    assert ao.durations(A, 3).tolist() == [4, 1, 1]


def test_mas_minus_inf_entries():
    # -inf everywhere except a staircase: the only finite path
    T, N = 5, 3
    lp = np.full((T, N), -np.inf, np.float32)
    for t, n in enumerate([0, 1, 1, 1, 2]):
        lp[t, n] = -1.0
    lp[0, 0] = 0.0
    A = ao.mas(lp)
    assert A.tolist() == [0, 1, 1, 1, 2]
    assert np.array_equal(ao.mas_fast(lp), A)
    # a row of -inf everywhere: Q is -inf from there on; every comparison -inf >= -inf is a tie and drops a token
    lp2 = np.zeros((5, 3), np.float32)
    lp2[2, :] = -np.inf
    assert ao.mas(lp2).tolist() == [0, 0, 0, 1, 2]


def test_mas_row0_sums_sequentially_in_fp64():
    rng = np.random.default_rng(3)
    lp = (rng.standard_normal((40, 5)) * 3).astype(np.float32)
    A = ao.mas(lp)
    # a path that stays on token 0 until the last N-1 frames compares against the sequential fp64 prefix sums
    assert A[-1] == 4 and A[0] == 0 and (np.diff(A) >= 0).all() and (np.diff(A) <= 1).all()


def test_packer_aligner_entries(sd):
    from emotivoice_amd.synthetic import synth_state_dict
    blob, man = pack_state_dict(sd)
    m = __import__("json").loads(man)
    H = 384
    for short, name in (("t1", "t_conv1"), ("t2", "t_conv2"), ("f1", "f_conv1"), ("f2", "f_conv2"), ("f3", "f_conv3")):
        w = sd[f"am.alignment_module.{name}.weight"]
        k = w.shape[2]
        K = MEL_PAD if short == "f1" else H
        assert m[f"aln.{short}.w32"]["shape"] == [H, k, K]
        assert m[f"aln.{short}.w32h"]["shape"] == [H, k, K] and m[f"aln.{short}.w32l"]["dtype"] == "f16"
        assert m[f"aln.{short}.b"]["shape"] == [H]
    # the aligner entries come last: a blob without the aligner is the same table and the same bytes up to them
    sd_no = {k: v for k, v in synth_state_dict(0, "parity").items() if not k.startswith("am.alignment_module.")}
    blob_no, man_no = pack_state_dict(sd_no)
    m_no = __import__("json").loads(man_no)
    assert not any(k.startswith("aln.") for k in m_no)
    names = list(m.keys())
    assert names[:len(m_no)] == list(m_no.keys())
    assert all(n.startswith("aln.") for n in names[len(m_no):])
    for n, e in m_no.items():
        assert m[n] == dict(e, offset=m[n]["offset"]), n        # same dtype, shape, size (the data moves by the longer table only)
        a = np.frombuffer(blob, np.uint8, e["nbytes"], m[n]["offset"])
        b = np.frombuffer(blob_no, np.uint8, e["nbytes"], e["offset"])
        assert np.array_equal(a, b), n


def _emulated_conv(blob_entry_w, blob_entry_b, x_rows, taps):
    """The GEMM the engine runs: out[m, n] = b[n] + sum_{tap, k} A[m + tap - center, k] * W[n][tap][k] on zero-padded rows."""
    W = torch.from_numpy(np.array(blob_entry_w))
    c = (taps - 1) // 2
    A = F.pad(torch.from_numpy(x_rows), (0, 0, c, taps - 1 - c))
    out = torch.from_numpy(np.array(blob_entry_b)).expand(x_rows.shape[0], -1).clone().double()
    for t in range(taps):
        out += A[t:t + x_rows.shape[0]].double() @ W[:, t, :].double().t()
    return out.float().numpy()


def test_packed_aligner_weights_are_the_convs(sd):
    blob, man = pack_state_dict(sd)
    m = __import__("json").loads(man)

    def get(n, dt=np.float32):
        e = m[n]
        return np.frombuffer(blob, dt, e["nbytes"] // np.dtype(dt).itemsize, e["offset"]).reshape(e["shape"])

    rng = np.random.default_rng(0)
    x = rng.standard_normal((37, 384)).astype(np.float32)
    mel = rng.standard_normal((80, 53)).astype(np.float32)
    for short, name, inp in (("t1", "t_conv1", x), ("f1", "f_conv1", mel.T), ("f2", "f_conv2", x), ("t2", "t_conv2", x)):
        w = torch.from_numpy(sd[f"am.alignment_module.{name}.weight"])
        b = torch.from_numpy(sd[f"am.alignment_module.{name}.bias"])
        want = F.conv1d(torch.from_numpy(np.ascontiguousarray(inp.T)).unsqueeze(0), w, b, padding=(w.shape[2] - 1) // 2).squeeze(0).t().numpy()
        rows = inp if short != "f1" else np.pad(inp, ((0, 0), (0, MEL_PAD - 80)))
        got = _emulated_conv(get(f"aln.{short}.w32"), get(f"aln.{short}.b"), np.ascontiguousarray(rows, np.float32), w.shape[2])
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
        # the split pair reconstructs the fp32 weight to the split's 2^-22 class
        hi = get(f"aln.{short}.w32h", np.float16).astype(np.float32)
        lo = get(f"aln.{short}.w32l", np.float16).astype(np.float32)
        np.testing.assert_allclose(hi + lo / 2048.0, get(f"aln.{short}.w32"), rtol=0, atol=1e-6)


def test_ffi_align_struct_and_signature():
    assert "ev_align" in _ffi.SIGNATURES
    assert C.sizeof(_ffi.ev_align_result) == 4 * 4 + 8 + 6 * 8
    lib = _ffi.lib()
    assert hasattr(lib, "ev_align")
    # the ABI version and the four pinned struct sizes are untouched
    sizes = (C.c_size_t * 4)()
    assert lib.ev_abi_info(sizes) == 7


def test_align_result_layout_matches_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evhip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(ev_align_result), offsetof(ev_align_result, total_frames), offsetof(ev_align_result, durations),'
                   'offsetof(ev_align_result, score), offsetof(ev_align_result, mel_lens), offsetof(ev_align_result, mel_offsets));return 0;}\n')
    exe = tmp_path / "s"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _ffi.ev_align_result
    assert got == [C.sizeof(S), S.total_frames.offset, S.durations.offset, S.score.offset, S.mel_lens.offset, S.mel_offsets.offset]
    # and the limits the header documents
    hdr = open(os.path.join(ROOT, "include", "evhip.h")).read()
    assert "#define EV_ALIGN_MAX_TOKENS 2048" in hdr and "#define EV_ALIGN_MAX_FRAMES 16384" in hdr
    assert _ffi.EV_ALIGN_MAX_TOKENS >= 2048 and _ffi.EV_ALIGN_MAX_FRAMES >= 16384


def test_timestamps():
    ts = timestamps([2, 1, 3], hop=256, sr=16000)
    f = 256 / 16000
    assert ts == [(0.0, 2 * f), (2 * f, 3 * f), (3 * f, 6 * f)]
    with pytest.raises(ValueError):
        timestamps([1, -1])


def _aligned():
    return dict(cu_seqlens=np.array([0, 3, 5], np.int32), durations=np.array([2, 1, 4, 1, 1], np.int64),
                pitch=np.arange(5, dtype=np.float32), energy=-np.arange(5, dtype=np.float32), mel_lens=np.array([7, 2], np.int32))


def test_prosody_from_alignment():
    pr = prosody_from_alignment(_aligned())
    assert len(pr) == 2
    assert pr[0].durations.tolist() == [2, 1, 4] and pr[1].durations.tolist() == [1, 1]
    assert pr[1].pitch.tolist() == [3.0, 4.0] and pr[0].energy.tolist() == [0.0, -1.0, -2.0]
    pr = prosody_from_alignment(_aligned(), pitch=False, energy=False)
    assert pr[0].pitch is None and pr[0].energy is None
    a = _aligned()
    a["pitch"] = None
    with pytest.raises(ValueError, match="no pitch"):
        prosody_from_alignment(a)
    a = _aligned()
    a["durations"] = np.array([2, 1, 4, MAX_DURATION + 1, 1], np.int64)
    with pytest.raises(ValueError, match="utterance 1, token 0"):
        prosody_from_alignment(a)


def test_transfer_checks_the_phonemes_pair_by_pair():
    class Never:
        def align(self, *a, **k):
            raise AssertionError("must not align")

    src = [dict(ling=np.array([1, 2, 3]), speaker=0, style=np.zeros(768), content=np.zeros(768))]
    dst = [dict(ling=np.array([1, 2, 4]), speaker=5, style=np.zeros(768), content=np.zeros(768))]
    with pytest.raises(ValueError, match="utterance 0"):
        transfer(Never(), src, [np.zeros((80, 5), np.float32)], dst)
    with pytest.raises(ValueError, match="1 source and 2 target"):
        transfer(Never(), src, [np.zeros((80, 5), np.float32)], dst * 2)


def test_transfer_feeds_the_alignment_to_synthesize():
    calls = {}

    class Fake:
        def align(self, utts, mels, pitch=None, energy=None):
            calls["align"] = (utts, pitch)
            return dict(cu_seqlens=np.array([0, 3], np.int32), durations=np.array([1, 2, 2], np.int64),
                        pitch=np.array([0.5, 0.25, 0.0], np.float32) if pitch is not None else None, energy=None)

        def synthesize(self, utts, prosody=None, vocoder=True):
            calls["syn"] = (utts, prosody)
            return dict(wav=np.zeros(1))

    src = [dict(ling=np.array([1, 2, 3]), speaker=0, style=np.zeros(768), content=np.zeros(768))]
    dst = [dict(ling=np.array([1, 2, 3]), speaker=9, style=np.ones(768), content=np.zeros(768))]
    out = transfer(Fake(), src, [np.zeros((80, 5), np.float32)], dst, pitch_frames=[np.zeros(5, np.float32)])
    assert calls["align"][0] is src and calls["syn"][0] is dst
    p = calls["syn"][1][0]
    assert p.durations.tolist() == [1, 2, 2] and p.pitch.tolist() == [0.5, 0.25, 0.0] and p.energy is None
    assert out["alignment"]["durations"].tolist() == [1, 2, 2]
