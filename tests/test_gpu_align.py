"""MI355X: ev_align -- forced alignment on the device (include/evhip.h).  Against the reference's own teacher-forced forward
(tests/golden/align/aln_*.npz): durations, per-token averages, score and log_p_attn; the MAS bit for bit against the host restatement on the
device's own log_p_attn; the aligned prosody through ev_synthesize_prosody against the reference's teacher-forced dec_outputs /
wav_predictions; batch, precision-mode, fp16 and device-input invariance; lifetime and state; rejections."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import align_oracle as ao
from conftest import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# in a directory of their own: the parity tests take every tests/golden/*.npz as an inference fixture
ALIGN_DIR = os.path.join(GOLDEN_DIR, "align")
FIXTURES = sorted(glob.glob(os.path.join(ALIGN_DIR, "aln_*.npz")))
PRECS = ("mx", "strict")
TOL_MX, TOL_STRICT = 1e-3, 2e-5          # tests/test_gpu_parity.py's bars for dec_outputs / wav (the DC-free measure too)
NEAR_TIE = 1e-4                          # |Q[i-1, j] - Q[i, j]| below this at a path decision of the golden: reported, not loosened


def rel_l2_ac(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b - b.mean()), 1e-30))


def _utt(g):
    return dict(ling=g["in_ling"], speaker=int(g["in_speaker"]), style=g["in_style"], content=g["in_content"])


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    sd = ao.aligner_state_dict(synth_state_dict(0, "parity"))
    blob, man = pack_state_dict(sd)
    engs = {}
    for prec in PRECS + ("fast",):
        engs[prec] = EVEngine(precision=prec, keep_stages=(prec == "mx"))
        engs[prec].load_blob(blob, man)
    gs = {os.path.basename(p)[:-4]: dict(np.load(p)) for p in FIXTURES}
    yield dict(engs=engs, gs=gs, sd=sd, blob=blob, man=man)
    for e in engs.values():
        e.close()


def _align_one(eng, g, f16=False):
    mel = g["in_mel"].astype(np.float16) if f16 else g["in_mel"]
    return eng.align([_utt(g)], [mel], pitch=[g["in_pitch_frames"]], energy=[g["in_energy_frames"]])


@pytest.mark.parametrize("prec", PRECS)
def test_matches_the_reference_teacher_forced_alignment(ctx, prec):
    eng = ctx["engs"][prec]
    report = {}
    for name, g in ctx["gs"].items():
        out = _align_one(eng, g)
        lp = eng.get_stage("log_p_attn").reshape(g["log_p_attn"].shape)
        # 1e-5, widened to one fp32 ulp (1.2e-7 relative) where |log_p| >= 128 and the ulp itself is 1.5e-5
        np.testing.assert_allclose(lp, g["log_p_attn"], rtol=2.5e-7, atol=1e-5, err_msg=name)
        m = ao.margins(g["log_p_attn"], ao.mas(g["log_p_attn"]))
        near = int((m < NEAR_TIE).sum())
        report[name] = dict(near_ties=near, min_margin=float(m.min()) if m.size else None)
        if not np.array_equal(out["durations"], g["duration_targets"]):
            assert near > 0, (name, "durations differ without a near tie in the golden", report[name])
            continue
        np.testing.assert_allclose(out["pitch"], g["pitch_targets"], rtol=1e-6, atol=1e-6, err_msg=name)
        np.testing.assert_allclose(out["energy"], g["energy_targets"], rtol=1e-6, atol=1e-6, err_msg=name)
        np.testing.assert_allclose(out["score"][0], -g["bin_loss"], rtol=1e-6, err_msg=name)
    print("near ties (margin < %g) per fixture, %s:" % (NEAR_TIE, prec), report)


def test_exact_mas_on_the_device_log_p(ctx):
    eng = ctx["engs"]["mx"]
    for name, g in ctx["gs"].items():
        out = _align_one(eng, g)
        lp = eng.get_stage("log_p_attn").reshape(g["log_p_attn"].shape)
        A = ao.mas_fast(lp)
        assert np.array_equal(ao.durations(A, lp.shape[1]), out["durations"]), name
        assert out["score"][0] == ao.path_score(lp, A), name
        d = out["durations"]
        assert np.array_equal(ao.average_by_duration(d, g["in_pitch_frames"]), out["pitch"]), name
        assert np.array_equal(ao.average_by_duration(d, g["in_energy_frames"]), out["energy"]), name


def _seeded_batch(B=32, N=256, seed=5):
    from emotivoice_amd.synthetic import synth_inputs
    rng = np.random.default_rng(seed)
    utts = synth_inputs(seed, [N] * B)
    Ts = [int(rng.integers(N, 6 * N + 1)) for _ in range(B)]
    Ts[0], Ts[1] = N, 6 * N
    mels = []
    for T in Ts:
        x = rng.standard_normal((80, T + 8)).astype(np.float32)
        mels.append(np.ascontiguousarray(sum(x[:, k:k + T] for k in range(9)) / 3.0, np.float32))
    return utts, mels, Ts


def test_exact_mas_on_a_seeded_32x256_batch(ctx):
    eng = ctx["engs"]["mx"]
    utts, mels, Ts = _seeded_batch()
    out = eng.align(utts, mels)
    lp_all = eng.get_stage("log_p_attn")
    o = 0
    for b, T in enumerate(Ts):
        N = len(utts[b]["ling"])
        lp = lp_all[o:o + T * N].reshape(T, N)
        o += T * N
        A = ao.mas_fast(lp)
        assert np.array_equal(ao.durations(A, N), out["durations_list"][b]), b
        assert out["score"][b] == ao.path_score(lp, A), b
    assert o == lp_all.size
    assert out["pitch"] is None and out["energy"] is None


@pytest.mark.parametrize("prec", PRECS)
def test_aligned_prosody_reproduces_teacher_forced_decode(ctx, prec):
    from emotivoice_amd.alignment import prosody_from_alignment
    eng = ctx["engs"][prec]
    tol = TOL_MX if prec == "mx" else TOL_STRICT
    for name, g in ctx["gs"].items():
        al = _align_one(eng, g)
        if not np.array_equal(al["durations"], g["duration_targets"]):
            continue                      # a near tie (reported by the test above): another path, another decode
        out = eng.synthesize([_utt(g)], prosody=prosody_from_alignment(al))
        assert int(out["mel_lens"][0]) == g["in_mel"].shape[1]
        e = dict(mel=rel_l2(out["mel"], g["dec_outputs"]), wav=rel_l2(out["wav"], g["wav_predictions"]),
                 wav_ac=rel_l2_ac(out["wav"], g["wav_predictions"]))
        assert e["mel"] < tol and e["wav"] < tol and e["wav_ac"] < tol, (name, prec, e)


def test_batch_precision_fp16_and_device_inputs(ctx):
    gs = list(ctx["gs"].values())
    utts = [_utt(g) for g in gs]
    mels = [g["in_mel"] for g in gs]
    P = [g["in_pitch_frames"] for g in gs]
    E = [g["in_energy_frames"] for g in gs]
    eng = ctx["engs"]["mx"]
    batch = eng.align(utts, mels, P, E)
    lp_batch = eng.get_stage("log_p_attn")
    o = 0
    for b, g in enumerate(gs):             # the mixed batch equals each utterance alone, bitwise
        one = _align_one(eng, g)
        n = g["log_p_attn"].size
        assert np.array_equal(eng.get_stage("log_p_attn"), lp_batch[o:o + n]), b
        o += n
        cu = batch["cu_seqlens"]
        for k in ("durations", "pitch", "energy"):
            assert np.array_equal(batch[k][cu[b]:cu[b + 1]], one[k]), (b, k)
        assert batch["score"][b] == one["score"][0]
    for prec in ("strict", "fast"):        # every precision mode: the same bits
        other = ctx["engs"][prec].align(utts, mels, P, E)
        for k in ("durations", "pitch", "energy", "score"):
            assert np.array_equal(other[k], batch[k]), (prec, k)
    # fp16 mel == fp32 mel rounded to fp16
    m16 = [m.astype(np.float16) for m in mels]
    a16 = eng.align(utts, m16, P, E)
    a32 = eng.align(utts, [m.astype(np.float32) for m in m16], P, E)
    for k in ("durations", "pitch", "energy", "score"):
        assert np.array_equal(a16[k], a32[k]), k
    # device inputs: the same bits as host inputs
    dev = torch.device("cuda", 0)
    ling = torch.from_numpy(np.concatenate([u["ling"] for u in utts]).astype(np.int64)).to(dev)
    spk = torch.tensor([u["speaker"] for u in utts], dtype=torch.int64, device=dev)
    sty = torch.from_numpy(np.stack([u["style"] for u in utts]).astype(np.float32)).to(dev)
    con = torch.from_numpy(np.stack([u["content"] for u in utts]).astype(np.float32)).to(dev)
    mel_d = torch.from_numpy(np.concatenate([m.ravel() for m in mels]).astype(np.float32)).to(dev)
    pf = torch.from_numpy(np.concatenate(P).astype(np.float32)).to(dev)
    ef = torch.from_numpy(np.concatenate(E).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    from emotivoice_amd import _ffi
    lens = np.array([m.shape[1] for m in mels], np.int32)
    res = eng.align_raw(len(utts), ling.data_ptr(), batch["cu_seqlens"], spk.data_ptr(), sty.data_ptr(), con.data_ptr(), mel_d.data_ptr(), False,
                        lens, pf.data_ptr(), ef.data_ptr(), _ffi.EV_FLAG_DEVICE_INPUTS)
    d = eng.align_to_numpy(res)
    for k in ("durations", "pitch", "energy", "score"):
        assert np.array_equal(d[k], batch[k]), k


def test_lifetime_and_state(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.prosody import Prosody, pack_prosody
    eng = ctx["engs"]["mx"]
    gs = list(ctx["gs"].values())[:2]
    utts = [_utt(g) for g in gs]
    # a plain synthesis: the same bits and launch records before and after an ev_align on the same handle
    eng.set_profiling(True)
    before = eng.synthesize(utts)
    rec_before = [(r["name"], r["M"], r["N"], r["K"], r["taps"]) for r in eng.launch_records()]
    res = eng.align_raw(*_raw_align_args(utts, gs))
    st = eng.kernel_stats()
    assert {"align_score", "align_mas", "align_f32_gemm"} <= {s["name"] for s in st}, st
    eng.set_profiling(False)
    with pytest.raises(Exception):
        eng.get_stage("dur")               # no synthesis' durations survive an ev_align
    host = eng.align_to_numpy(res)
    eng.set_profiling(True)
    after = eng.synthesize(utts)
    rec_after = [(r["name"], r["M"], r["N"], r["K"], r["taps"]) for r in eng.launch_records()]
    eng.set_profiling(False)
    assert rec_before == rec_after
    for k in ("wav", "mel", "durations", "pitch", "energy"):
        assert np.array_equal(before[k], after[k]), k
    # the align result survives a synthesis, and passed back as device overrides gives the host-override result bitwise
    pr_host = [Prosody(durations=host["durations"][a:b], pitch=host["pitch"][a:b], energy=host["energy"][a:b])
               for a, b in zip(res_cu(utts)[:-1], res_cu(utts)[1:])]
    want = eng.synthesize(utts, prosody=pr_host)
    again = eng.align_to_numpy(res)
    for k in ("durations", "pitch", "energy", "score"):
        assert np.array_equal(again[k], host[k]), k
    dev = torch.device("cuda", 0)
    ling = torch.from_numpy(np.concatenate([u["ling"] for u in utts]).astype(np.int64)).to(dev)
    spk = torch.tensor([u["speaker"] for u in utts], dtype=torch.int64, device=dev)
    sty = torch.from_numpy(np.stack([u["style"] for u in utts]).astype(np.float32)).to(dev)
    con = torch.from_numpy(np.stack([u["content"] for u in utts]).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    p = pack_prosody([Prosody(), Prosody()], [len(u["ling"]) for u in utts], 1.0)
    st_ = p.struct
    st_.durations, st_.pitch, st_.energy = res.durations, res.pitch, res.energy
    r = eng.synthesize_prosody_raw(len(utts), ling.data_ptr(), res_cu(utts), spk.data_ptr(), sty.data_ptr(), con.data_ptr(), 1.0, _DevPacked(st_),
                                   _ffi.EV_FLAG_DEVICE_INPUTS)
    got = eng.result_to_numpy(r)
    for k in ("wav", "mel"):
        assert np.array_equal(got[k], want[k]), k


class _DevPacked:
    device = True

    def __init__(self, st):
        self.struct = st


def res_cu(utts):
    cu = np.zeros(len(utts) + 1, np.int32)
    cu[1:] = np.cumsum([len(u["ling"]) for u in utts])
    return cu


_KEEP = []


def _raw_align_args(utts, gs, lens=None, ling=None, spk=None):
    ling = np.ascontiguousarray(np.concatenate([u["ling"] for u in utts]).astype(np.int64)) if ling is None else ling
    spk = np.array([u["speaker"] for u in utts], np.int64) if spk is None else spk
    sty = np.ascontiguousarray(np.stack([u["style"] for u in utts]).astype(np.float32))
    con = np.ascontiguousarray(np.stack([u["content"] for u in utts]).astype(np.float32))
    mel = np.ascontiguousarray(np.concatenate([g["in_mel"].ravel() for g in gs]).astype(np.float32))
    pf = np.ascontiguousarray(np.concatenate([g["in_pitch_frames"] for g in gs]).astype(np.float32))
    ef = np.ascontiguousarray(np.concatenate([g["in_energy_frames"] for g in gs]).astype(np.float32))
    lens = np.array([g["in_mel"].shape[1] for g in gs], np.int32) if lens is None else lens
    _KEEP[:] = [ling, spk, sty, con, mel, pf, ef]
    return (len(utts), ling.ctypes.data, res_cu(utts), spk.ctypes.data, sty.ctypes.data, con.ctypes.data, mel.ctypes.data, False, lens,
            pf.ctypes.data, ef.ctypes.data, 0)


def test_rejections_launch_nothing(ctx):
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVError, EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    eng = ctx["engs"]["mx"]
    gs = list(ctx["gs"].values())[:2]
    utts = [_utt(g) for g in gs]
    eng.set_profiling(True)

    def rejected(args, match, struct_size=None):
        res = _ffi.ev_align_result()
        res.struct_size = C.sizeof(_ffi.ev_align_result) if struct_size is None else struct_size
        B, ling, cu, spk, sty, con, mel, f16, lens, pf, ef, flags = args
        rc = eng._lib.ev_align(eng._h, B, C.c_void_p(ling), np.ascontiguousarray(cu, np.int32).ctypes.data_as(C.c_void_p), C.c_void_p(spk),
                               C.c_void_p(sty), C.c_void_p(con), C.c_void_p(mel), 0, np.ascontiguousarray(lens, np.int32).ctypes.data_as(C.c_void_p),
                               C.c_void_p(pf), C.c_void_p(ef), flags, C.byref(res))
        assert rc != 0
        msg = eng._lib.ev_last_error(eng._h).decode()
        assert match in msg, msg
        assert eng.launch_records() == rec0, match        # still the records of the synthesis before: nothing was launched

    eng.synthesize(utts[:1])
    rec0 = eng.launch_records()
    assert rec0
    short = np.array([g["in_mel"].shape[1] for g in gs], np.int32)
    short[1] = len(utts[1]["ling"]) - 1
    rejected(_raw_align_args(utts, gs, lens=short), "mel_lens[1]")
    bad = np.concatenate([u["ling"] for u in utts]).astype(np.int64)
    bad[5] = 10 ** 6
    rejected(_raw_align_args(utts, gs, ling=bad), "position 5")
    rejected(_raw_align_args(utts, gs, spk=np.array([0, -1], np.int64)), "utterance 1")
    rejected(_raw_align_args(utts, gs), "struct_size", struct_size=8)
    big = np.array([g["in_mel"].shape[1] for g in gs], np.int32)
    big[0] = _ffi.EV_ALIGN_MAX_FRAMES + 1
    rejected(_raw_align_args(utts, gs, lens=big), "EV_ALIGN_MAX_FRAMES")
    eng.set_profiling(False)
    # a blob without the aligner
    sd_no = {k: v for k, v in synth_state_dict(0, "parity").items() if not k.startswith("am.alignment_module.")}
    e2 = EVEngine()
    try:
        e2.load_blob(*pack_state_dict(sd_no))
        with pytest.raises(EVError, match="aligner"):
            e2.align(utts, [g["in_mel"] for g in gs])
    finally:
        e2.close()


def test_keep_stages_taps(ctx):
    eng = ctx["engs"]["mx"]
    g = ctx["gs"]["aln_n48_selfmel"]
    _align_one(eng, g)
    text = eng.get_stage("aln_text").reshape(-1, 384)
    feats = eng.get_stage("aln_feats").reshape(-1, 384)
    assert text.shape[0] == len(g["in_ling"]) and feats.shape[0] == g["in_mel"].shape[1]
    np.testing.assert_allclose(eng.get_stage("x_proj").reshape(-1, 384), g["x_proj"], rtol=0, atol=1e-4)
