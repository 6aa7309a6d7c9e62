"""MI355X: ev_score -- log-mel -> integer cepstra, local distances, DTW and the sums along its path on the device (include/evhip.h) -- compared
exactly, with no tolerance, against the numpy / Python-integer oracle (tests/score_oracle.py): cq_a, cq_b, both path arrays, every count, sum_dist
and nonfinite; the two fp64 F0 sums within the derived 1e-9.  Lane, run and wave edges of the skewed wavefront, the tie case, a pair that crosses
every staging chunk of the backtrack, the linear path, non-finite input, device inputs, the int64 headroom, then the scores end to end on
synthesised speech (emotivoice_amd/scoring.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import score_oracle as so
from conftest import ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# Ta from {1, 2, 63, 64, 65, 128, 129, 257} (one row, the last lane of a run of 1, the first run of 2, its last lane, the first run of 4 and 8) against
# Tb from {1, 3, 64, 65, 200} (one column, fewer columns than lanes, a staging chunk of the backtrack, one past it, several)
EDGE_PAIRS = [(1, 1), (1, 200), (257, 1), (2, 3), (63, 64), (64, 65), (65, 200), (128, 3), (129, 64), (257, 65), (64, 1), (2, 200), (128, 200)]
REPORT = {}


def _report(key, val):
    """score_report.json, next to parity_report.json"""
    from test_gpu_parity import _report as write_report
    write_report(key, val, "score_report.json", REPORT)


def _mel(T, seed, n_mels=80):
    """Log-mel-like noise keyed by (T, seed): the same signal in every batch it appears in."""
    rng = np.random.default_rng(seed * 100003 + T * 131 + n_mels)
    return (rng.standard_normal((n_mels, T)) * 1.5 - 4.0).astype(np.float32)


def _edge_batch():
    return [_mel(ta, 1) for ta, _ in EDGE_PAIRS], [_mel(tb, 2) for _, tb in EDGE_PAIRS]


def _f0(T, seed):
    """Voiced and unvoiced runs of random lengths, one NaN."""
    rng = np.random.default_rng(seed * 7919 + T)
    f = (120.0 * np.exp2(rng.uniform(-0.5, 0.5, T))).astype(np.float32)
    t = 0
    while t < T:
        n = int(rng.integers(3, 30))
        if rng.random() < 0.4:
            f[t:t + n] = 0.0
        t += n
    f[T // 2] = np.nan
    return f


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd.engine import EVEngine
    e = EVEngine(precision="mx")          # ev_score needs no weights
    yield e
    e.close()


@pytest.fixture(scope="module")
def edges(eng):
    a, b = _edge_batch()
    f0a, f0b = [_f0(x.shape[1], 3) for x in a], [_f0(y.shape[1], 4) for y in b]
    want = so.score(a, b, f0a, f0b)
    eng.score_load(0, a, f0a)
    eng.score_load(1, b, f0b)
    got = eng.score_to_numpy(eng.score_raw(), with_cq=True)
    return dict(a=a, b=b, f0a=f0a, f0b=f0b, want=want, got=got)


def _pair(res, b):
    """Pair b of a result as a one-pair result."""
    out = {k: np.asarray(res[k])[b:b + 1] for k in so.EXACT_KEYS + ("sum_c", "sum_c2", "mcd_db", "vuv_error", "warp", "f0_rmse_cents", "f0_bias_cents")}
    if "sum_abs_c" in res:
        out["sum_abs_c"] = res["sum_abs_c"][b:b + 1]
    out["path_list"] = res["path_list"][b:b + 1]
    out["path_offsets"] = np.array([0, res["path_len"][b]], np.int64)
    for side in ("a", "b"):
        out["cq_%s_list" % side] = res["cq_%s_list" % side][b:b + 1]
    return out


def test_edges_of_the_skewed_wavefront_against_the_oracle(edges):
    got, want = edges["got"], edges["want"]
    assert got["batch"] == len(EDGE_PAIRS) and not got["linear"]
    so.assert_exact(got, want, "edges")
    so.assert_f0_sums(got, want, "edges")
    for b, (ta, tb) in enumerate(EDGE_PAIRS):
        K = got["path_len"][b]
        assert max(ta, tb) <= K <= ta + tb - 1 and K == 1 + got["n_diag"][b] + got["n_a"][b] + got["n_b"][b]
        assert got["n_vv"][b] + got["n_vu"][b] + got["n_uv"][b] + got["n_uu"][b] == K
    assert got["path_len"][0] == 1 and got["path_len"][1] == 200 and got["path_len"][2] == 257          # (1, 1), (1, 200), (257, 1)
    assert got["n_b"][1] == 199 and got["n_a"][2] == 256
    assert got["n_vv"].sum() > 100 and got["n_vu"].sum() > 0 and got["n_uv"].sum() > 0 and got["n_uu"].sum() > 0


def test_a_pair_alone_gives_the_bits_it_gives_in_the_batch(eng, edges):
    for b in range(len(EDGE_PAIRS)):
        eng.score_load(0, edges["a"][b:b + 1], edges["f0a"][b:b + 1])
        eng.score_load(1, edges["b"][b:b + 1], edges["f0b"][b:b + 1])
        solo = eng.score_to_numpy(eng.score_raw(), with_cq=True)
        so.assert_exact(solo, _pair(edges["got"], b), "solo %d" % b)
        assert solo["sum_c"].tobytes() == edges["got"]["sum_c"][b:b + 1].tobytes() and solo["sum_c2"].tobytes() == edges["got"]["sum_c2"][b:b + 1].tobytes()


def test_the_tie_case_on_the_device(eng):
    a, b = so.tie_case()
    want = so.score([a], [b])
    so.assert_exact(eng.score([a], [b], with_cq=True), want, "tie")
    for tie in so.TIE_RULES[1:]:          # the input does tell the wrong orders apart
        wrong = so.score_pair(want["cq_a_list"][0], want["cq_b_list"][0], tie=tie)["path"]
        assert wrong.shape != want["path_list"][0].shape or not np.array_equal(wrong, want["path_list"][0]), tie


def test_a_long_pair_across_every_staging_chunk(eng):
    a, b = _mel(1100, 5), _mel(1030, 6)          # a run of 32 rows per lane (two decision words), 1064 steps: 34 chunks of the backtrack
    want = so.score([a], [b])
    got = eng.score([a], [b], with_cq=True)
    so.assert_exact(got, want, "long")
    assert got["n_a"][0] > 0 and got["n_b"][0] > 0 and got["n_diag"][0] > 0


def test_the_longest_run_against_the_oracle(eng):
    """Ta above 2048: 64 rows per lane, four decision words per lane and step, 16 steps per staging chunk of the backtrack; Ta = 4096 is the limit."""
    shapes = [(2049, 300), (4096, 70), (2100, 40), (4096, 1)]
    a, b = [_mel(ta, 12) for ta, _ in shapes], [_mel(tb, 13) for _, tb in shapes]
    want = so.score(a, b)
    got = eng.score(a, b, with_cq=True)
    so.assert_exact(got, want, "run of 64")
    assert got["path_len"][3] == 4096 and got["n_a"][0] > 0 and got["n_diag"][0] > 0


def test_a_batch_beyond_the_workspace_runs_in_passes(eng):
    """Fourteen pairs of 4096 x 4096 frames fill 0.94 GiB of EV_SCORE_WORKSPACE; a fifteenth, of other signals, starts a second pass at offset 0 of
    the same workspace, and three short pairs of further signals (runs of 1, 64 and 4) follow it there.  A pass that never ran, or an offset
    taken from the first pass, would hand the second pass the first one's distances: the short pairs are held to the oracle, the two long signal
    pairs to their solo runs (the oracle takes 7.5 s per 16.7 M cells; the run of 64 is held to it at 4096 x 70 above)."""
    from emotivoice_amd import _ffi
    big, other = (_mel(4096, 21), _mel(4096, 22)), (_mel(4096, 23), _mel(4096, 24))
    small = [(_mel(64, 25), _mel(300, 26)), (_mel(2049, 27), _mel(300, 28)), (_mel(129, 29), _mel(64, 30))]
    a = [big[0]] * 14 + [other[0]] + [x for x, _ in small]
    b = [big[1]] * 14 + [other[1]] + [y for _, y in small]
    la, lb = np.array([x.shape[1] for x in a], np.int32), np.array([y.shape[1] for y in b], np.int32)
    pass_of, pass_bytes = np.zeros(len(a), np.int32), np.zeros(len(a), np.int64)
    n_pass = _ffi.lib().ev_score_plan(len(a), la.ctypes.data_as(C.c_void_p), lb.ctypes.data_as(C.c_void_p), pass_of.ctypes.data_as(C.c_void_p),
                                      pass_bytes.ctypes.data_as(C.c_void_p))
    assert n_pass == 2 and pass_of.tolist() == [0] * 14 + [1] * 4 and (pass_bytes[:2] <= _ffi.EV_SCORE_WORKSPACE).all()
    solo_big, solo_other = eng.score([big[0]], [big[1]]), eng.score([other[0]], [other[1]])
    want_small = so.score([x for x, _ in small], [y for _, y in small])
    got = eng.score(a, b, with_cq=True)
    assert 4096 <= solo_big["path_len"][0] < 8191 and solo_big["sum_dist"][0] != solo_other["sum_dist"][0]
    for k in so.EXACT_KEYS:
        assert (np.asarray(got[k])[:14] == np.asarray(solo_big[k])[0]).all(), (k, got[k], solo_big[k])
        assert np.asarray(got[k])[14] == np.asarray(solo_other[k])[0], (k, got[k], solo_other[k])
    for p in got["path_list"][:14]:
        assert np.array_equal(p, solo_big["path_list"][0])
    assert np.array_equal(got["path_list"][14], solo_other["path_list"][0])
    for i in range(3):
        so.assert_exact(_pair(got, 15 + i), _pair(want_small, i), "second pass, short pair %d" % i)
    steps = np.diff(got["path_list"][14], axis=0)
    assert np.array_equal(got["path_list"][14][0], [0, 0]) and np.array_equal(got["path_list"][14][-1], [4095, 4095])
    assert (steps >= 0).all() and (steps.max(axis=1) == 1).all()


def test_linear_on_unequal_lengths(eng, edges):
    sel = [3, 4, 6, 9, 0, 1]
    a, b = [edges["a"][i] for i in sel], [edges["b"][i] for i in sel]
    f0a, f0b = [edges["f0a"][i] for i in sel], [edges["f0b"][i] for i in sel]
    want = so.score(a, b, f0a, f0b, linear=True)
    got = eng.score(a, b, f0a, f0b, linear=True, with_cq=True)
    assert got["linear"]
    so.assert_exact(got, want, "linear")
    so.assert_f0_sums(got, want, "linear")
    assert list(got["path_len"]) == [min(EDGE_PAIRS[i]) for i in sel] and (got["n_a"] == 0).all() and (got["n_b"] == 0).all()


def test_nonfinite_mel_frames_are_counted_and_zeroed(eng):
    a, b = _mel(70, 7), _mel(90, 8)
    a[5, 10], a[60, 10], a[3, 64] = np.nan, np.inf, -np.inf          # two values in one frame count once; a second frame in the next tile
    b[0, 89], b[79, 89] = np.inf, np.nan          # a NaN and an inf in one frame of each side
    want = so.score([a], [b])
    got = eng.score([a], [b], with_cq=True)
    so.assert_exact(got, want, "nonfinite")
    assert got["nonfinite_a"][0] == 2 and got["nonfinite_b"][0] == 1
    assert not got["cq_a_list"][0][10].any() and not got["cq_a_list"][0][64].any() and not got["cq_b_list"][0][89].any()
    assert got["cq_a_list"][0][11].any() and np.isfinite(got["mcd_db"]).all() and got["sum_dist"][0] > 0


def test_device_inputs_give_the_bits_of_host_inputs(eng, edges):
    DEV = 1
    sides = []
    for mels, f0 in ((edges["a"], edges["f0a"]), (edges["b"], edges["f0b"])):
        flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mels])).cuda()
        f0d = torch.from_numpy(np.concatenate(f0)).cuda()
        sides.append((flat, f0d, np.array([m.shape[1] for m in mels], np.int32)))
    torch.cuda.synchronize()
    for side, (flat, f0d, lens) in enumerate(sides):
        eng.score_load_raw(side, len(lens), 80, 13, flat.data_ptr(), lens, f0d.data_ptr(), DEV)
    got = eng.score_to_numpy(eng.score_raw(), with_cq=True)
    so.assert_exact(got, edges["got"], "device inputs")
    assert got["sum_c"].tobytes() == edges["got"]["sum_c"].tobytes() and got["sum_c2"].tobytes() == edges["got"]["sum_c2"].tobytes()


@pytest.mark.parametrize("n_ceps,n_mels", [(1, 80), (32, 80), (1, 128), (32, 128)])
def test_shapes_and_the_int64_headroom(eng, n_ceps, n_mels):
    """Mel values of +-1e4 in half of the frames: the clamp at 2^27 engages, differences reach 2^28 and s approaches 2^61 at n_ceps = 32."""
    a, b = [_mel(t, 9, n_mels) for t in (130, 40)], [_mel(t, 10, n_mels) for t in (70, 66)]
    rng = np.random.default_rng(11)
    for m in a + b:
        m[:, ::2] = (rng.choice([-1e4, 1e4], m[:, ::2].shape)).astype(np.float32)
    want = so.score(a, b, n_ceps=n_ceps)
    got = eng.score(a, b, n_ceps=n_ceps, with_cq=True)
    so.assert_exact(got, want, "headroom")
    top = max(np.abs(c).max() for c in got["cq_a_list"] + got["cq_b_list"])
    assert top == so.CLAMP and got["n_ceps"] == n_ceps and got["cq_a_list"][0].shape == (130, n_ceps)
    assert got["sum_dist"].max() > 2 ** 31          # past int32 at one coefficient already
    if n_ceps == 32:          # a single distance near 2^30.5, the sum past uint32
        assert got["sum_dist"].max() > 2 ** 32 and so.dist_matrix(want["cq_a_list"][0], want["cq_b_list"][0]).max() > 2 ** 30


def test_rejections_leave_the_previous_result_valid(eng, edges):
    from emotivoice_amd import _ffi
    from emotivoice_amd.engine import EVEngine, EVError
    a, b = edges["a"][3:6], edges["b"][3:6]
    eng.score_load(0, a)
    eng.score_load(1, b)
    res = eng.score_raw()
    before = eng.score_to_numpy(res, with_cq=True)
    flat = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in a]))
    lens = np.array([m.shape[1] for m in a], np.int32)
    for kw, needle in ((dict(side=2), "side = 2"), (dict(B=0), "B = 0"), (dict(n_mels=0), "n_mels = 0"), (dict(n_mels=129), "n_mels = 129"),
                       (dict(n_ceps=0), "n_ceps = 0"), (dict(n_ceps=33, n_mels=80), "n_ceps = 33"), (dict(n_ceps=80, n_mels=80), "n_ceps = 80"),
                       (dict(lens=np.array([2, 0, 3], np.int32)), "lens[1] = 0"), (dict(lens=np.array([2, 3, 4097], np.int32)), "lens[2] = 4097"),
                       (dict(mel=0), "mel is NULL")):
        args = dict(side=0, B=3, n_mels=80, n_ceps=13, mel=flat.ctypes.data, lens=lens)
        args.update(kw)
        with pytest.raises(EVError, match="ev_score_load") as ei:
            eng.score_load_raw(args["side"], args["B"], args["n_mels"], args["n_ceps"], args["mel"], args["lens"])
        assert needle in str(ei.value), (kw, str(ei.value))
    bad = _ffi.ev_score_result()
    bad.struct_size = C.sizeof(_ffi.ev_score_result) - 8
    assert eng._lib.ev_score(eng._h, 0, C.byref(bad)) != 0 and b"struct_size" in eng._lib.ev_last_error(eng._h)
    assert eng._lib.ev_score(eng._h, 0, None) != 0 and b"out is NULL" in eng._lib.ev_last_error(eng._h)
    so.assert_exact(eng.score_to_numpy(res, with_cq=True), before, "after rejected calls")
    # sides that differ: a successful load replaces side 1, the result (its cq copies included) stays; ev_score is rejected
    eng.score_load(1, b[:2])
    with pytest.raises(EVError, match="differ in B"):
        eng.score_raw()
    eng.score_load(1, [m[:40] for m in b])
    with pytest.raises(EVError, match="differ in n_mels"):
        eng.score_raw()
    eng.score_load(1, b, n_ceps=5)
    with pytest.raises(EVError, match="differ in n_ceps"):
        eng.score_raw()
    so.assert_exact(eng.score_to_numpy(res, with_cq=True), before, "after replaced sides")
    fresh = EVEngine(precision="mx")
    try:
        with pytest.raises(EVError, match="side 0 .a. is not loaded"):
            fresh.score_raw()
        fresh.score_load(0, a)
        with pytest.raises(EVError, match="side 1 .b. is not loaded"):
            fresh.score_raw()
    finally:
        fresh.close()


# ---------------------------------------------------------------- end to end on synthesised speech
UTT_LENS, UTT_SPK = [24, 40], [3, 8]          # the small batch of the parity tests' kind


def _engine(precision):
    from emotivoice_amd.engine import EVEngine
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    blob, man = pack_state_dict(synth_state_dict(0, "parity"), pe_len=1024)
    e = EVEngine(device_id=0, precision=precision)
    e.load_blob(blob, man)
    return e


@pytest.fixture(scope="module")
def tts():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd.synthetic import synth_inputs
    e = _engine("mx")
    yield dict(eng=e, utts=synth_inputs(7, UTT_LENS, UTT_SPK))
    e.close()


def _host_features(e):
    """The features and the F0 tracks of the engine's last ev_features / ev_pitch, copied to the host."""
    return e.features_to_numpy(e.last_features)["mel_list"], e.pitch_to_numpy(e.last_pitch)["f0_list"]


def _as_result(rep):
    """A scoring.py report as per-pair arrays."""
    return {k: np.array([u[k] for u in rep["utterances"]]) for k in rep["utterances"][0]}


def test_score_recordings_closes_the_loop_on_the_engines_own_output(tts):
    """The synthesised waveform, copied to the host and passed back as the recording at 16 kHz without trimming.  ev_resample at equal rates is a
    copy, and ev_features / ev_pitch give a signal the same bits from host or device memory and anywhere in a batch, so both sides hold the same
    features: distance 0, a pure diagonal, no voicing error."""
    from emotivoice_amd.scoring import score_recordings
    e, utts = tts["eng"], tts["utts"]
    wavs = [w.copy() for w in e.synthesize(utts)["wav_list"]]
    rep = score_recordings(e, utts, wavs, sample_rate=16000, trim=False)
    for u in rep["utterances"]:
        assert u["sum_dist"] == 0 and u["n_a"] == 0 and u["n_b"] == 0 and u["path_len"] == u["lens_a"] == u["lens_b"] == u["n_diag"] + 1, u
        assert u["vuv_error"] == 0.0 and u["mcd_db"] == 0.0 and u["nonfinite_a"] == 0 and u["nonfinite_b"] == 0, u
        assert u["n_vv"] + u["n_uu"] == u["path_len"] and (u["n_vv"] == 0 or u["f0_rmse_cents"] == 0.0), u
    assert rep["corpus"]["mcd_db"] == 0.0 and rep["corpus"]["path_len"] == sum(u["path_len"] for u in rep["utterances"])


def test_warped_scores_equal_the_oracle_on_the_copied_features(tts):
    """The same utterances at alpha = 1.0 and 1.2 (ev_synthesize_prosody): the renderings differ in length, every figure equals the oracle's on the
    two feature sets copied to the host.  No bar on the MCD itself."""
    from emotivoice_amd.prosody import Prosody
    from emotivoice_amd.scoring import _load_side, _wav_lens
    e, utts = tts["eng"], tts["utts"]
    host = []
    for side, alpha in ((0, 1.0), (1, 1.2)):
        res, _ = e._synthesize_call(utts, 1.0, 0, None, Prosody(alpha=alpha))
        _load_side(e, side, res.wav, _wav_lens(e, res), len(utts), 13, None)
        host.append(_host_features(e))
    got = e.score_to_numpy(e.score_raw(), with_cq=True)
    want = so.score(host[0][0], host[1][0], host[0][1], host[1][1])
    so.assert_exact(got, want, "warped")
    so.assert_f0_sums(got, want, "warped")
    assert (got["path_len"] >= np.maximum(got["lens_a"], got["lens_b"])).all() and (got["lens_b"] > got["lens_a"]).all()
    _report("warped_alpha_1.0_vs_1.2", dict(mcd_db=got["mcd_db"].tolist(), warp=got["warp"].tolist(), lens_a=got["lens_a"].tolist(), lens_b=got["lens_b"].tolist()))


def test_score_engines_mx_against_strict(tts):
    """score_engines runs and equals the oracle (linear) on the features of the two renderings; the mcd_db it reports is recorded, with no bar."""
    from emotivoice_amd.scoring import _load_side, _wav_lens, score_engines
    e, utts = tts["eng"], tts["utts"]
    strict = _engine("strict")
    try:
        rep = score_engines(e, strict, utts)
        got = _as_result(rep)
        # the same two renderings once more, their features copied to the host
        res_a, _ = e._synthesize_call(utts, 1.0, 0, None, None)
        dur = e.d2h(res_a.durations, (res_a.total_tokens,), np.int64)
        _load_side(e, 0, res_a.wav, _wav_lens(e, res_a), len(utts), 13, None)
        fa = _host_features(e)
        res_b, _ = strict._synthesize_call(utts, 1.0, 0, dur, None)
        _load_side(e, 1, res_b.wav, _wav_lens(strict, res_b), len(utts), 13, None)
        fb = _host_features(e)
    finally:
        strict.close()
    want = so.score(fa[0], fb[0], fa[1], fb[1], linear=True)
    assert rep["linear"] and rep["n_ceps"] == 13
    for k in so.EXACT_KEYS + ("mcd_db", "vuv_error", "warp"):
        assert np.array_equal(got[k], np.asarray(want[k]).astype(got[k].dtype)), (k, got[k], want[k])
    so.assert_f0_sums(got, want, "score_engines")
    assert (got["lens_a"] == got["lens_b"]).all() and np.isfinite(got["mcd_db"]).all()
    _report("mx_vs_strict", dict(mcd_db=got["mcd_db"].tolist(), corpus=rep["corpus"], sum_dist=got["sum_dist"].tolist(), path_len=got["path_len"].tolist()))


def test_score_corpus_tool_on_a_directory_of_recordings(tts, tmp_path):
    """tools/score_corpus.py end to end: a config folder, a text file in the reference's line format (one line with an unknown speaker, skipped) and
    <line number>.wav recordings -- here the engine's own rendering of the two lines as 16-bit PCM -- give one JSON line per utterance and one for
    the corpus.  The renderings have the recordings' lengths; no bar on the figures (int16 rounding is in them)."""
    import importlib.util

    import yaml
    from emotivoice_amd.text_io import HashStyleEmbedder, wav_float_to_int16, write_wav_int16
    root = tmp_path
    (root / "cfg").mkdir()
    toks = ["_", "<sos/eos>"] + ["p%d" % i for i in range(500)]
    (root / "tokenlist").write_text("\n".join(toks) + "\n")
    (root / "speaker2").write_text("\n".join(["8051"] + ["s%d" % i for i in range(2013)]) + "\n")
    model = dict(encoder_n_hidden=384, encoder_n_heads=8, encoder_n_layers=4, encoder_kernel_size_conv_mod=3, decoder_n_hidden=384,
                 decoder_n_layers=4, variance_n_hidden=384, variance_n_layers=3, variance_kernel_size=3, variance_embed_kernel_size=9,
                 duration_n_layers=2, duration_kernel_size=3, bert_embedding=768, resblock="1", upsample_rates=[8, 8, 2, 2],
                 upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512, resblock_kernel_sizes=[3, 7, 11],
                 resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]])
    (root / "cfg" / "config.yaml").write_text(yaml.safe_dump(dict(n_mels=80, sr=16000, hop_length=256, segment_size=32, model=model)))
    (root / "cfg" / "config.py").write_text(
        "ROOT = %r\nclass Config:\n    output_directory = ROOT + '/outputs'\n    model_config_path = ROOT + '/cfg/config.yaml'\n"
        "    token_list_path = ROOT + '/tokenlist'\n    speaker2id_path = ROOT + '/speaker2'\n"
        "    n_symbols = 502\n    speaker_n_labels = 2014\n    sampling_rate = 16000\n" % str(root))
    rng = np.random.default_rng(0)
    ids = [rng.integers(2, 502, n) for n in (30, 12)]
    lines = ["8051|Happy|%s|some content" % " ".join(["<sos/eos>"] + [toks[int(i)] for i in x] + ["<sos/eos>"]) for x in ids]
    lines.insert(1, "nobody|Happy|<sos/eos> p1 <sos/eos>|skipped: unknown speaker")
    (root / "text").write_text("\n".join(lines) + "\n")
    emb = HashStyleEmbedder(768)
    utts = [dict(ling=np.concatenate([[1], x, [1]]).astype(np.int64), speaker=0, style=emb("Happy"), content=emb("some content")) for x in ids]
    (root / "wavs").mkdir()
    for line_no, w in zip((1, 3), tts["eng"].synthesize(utts)["wav_list"]):
        write_wav_int16(str(root / "wavs" / ("%d.wav" % line_no)), wav_float_to_int16(w), 16000)
    spec = importlib.util.spec_from_file_location("score_corpus", os.path.join(ROOT, "tools", "score_corpus.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(["-c", str(root / "cfg"), "--synthetic-weights", "-t", str(root / "text"), "--wavs", str(root / "wavs"), "--out", str(root / "scores.jsonl")])
    rows = [json.loads(x) for x in (root / "scores.jsonl").read_text().splitlines()]
    assert [r.get("line") for r in rows] == [1, 3, None] and rows[2]["corpus"]["pairs"] == 2
    for r in rows[:2]:
        assert r["lens_a"] == r["lens_b"] and r["path_len"] >= r["lens_a"] and np.isfinite(r["mcd_db"]) and r["mcd_db"] >= 0.0 and r["sample_rate"] == 16000
    assert rows[2]["corpus"]["path_len"] == rows[0]["path_len"] + rows[1]["path_len"] and np.isfinite(rows[2]["corpus"]["mcd_db"])
