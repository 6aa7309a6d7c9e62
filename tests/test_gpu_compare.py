"""MI355X: ev_compare -- two packed signals -> per-segment fp64 sums, ratios and maxima on the device (include/evhip.h) -- bit for bit against the
numpy oracle (tests/compare_oracle.py) at the edges of the thread stride, the chunk and the chunk table; invariance, rejections; then the
precision guard on hardware: mx against strict on a fixture, the ladder, and the verified load."""
import ctypes as C
import os

import numpy as np
import pytest

import compare_oracle as co
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# the edges: one element, one short of / exactly / one past the 256-thread stride, the same around the 4096-element chunk, three chunks and a rest.
# In this order segment 0 and the first three chunks of segment 1 start 16-byte aligned (the float4 path), everything after them does not.
LENS = [4096, 3 * 4096 + 5, 4097, 256, 1, 255, 257, 4095]
SAME, ZERO, BAD = 3, 6, 1          # the segment with a == b, the one with an all-zero b, the one with planted non-finite values
KEYS = co.PER_SEGMENT + ("chunk_d2", "chunk_y2", "chunk_offsets")


def _batch(lens, seed=11):
    """b: noise on a DC offset three times its amplitude; a = b + 1e-3 noise.  Keyed by length, so a segment is the same data in every order."""
    a_list, b_list = [], []
    for n in lens:
        rng = np.random.default_rng(seed * 100003 + n)
        b = (0.1 * rng.standard_normal(n) + 0.3).astype(np.float32)
        a = (b + (1e-3 * rng.standard_normal(n)).astype(np.float32)).astype(np.float32)
        if n == LENS[SAME]:
            a = b.copy()
        if n == LENS[ZERO]:
            b = np.zeros(n, np.float32)
        if n == LENS[BAD]:          # on both sides of the first chunk border, and the first element of the third chunk
            a[4095], a[4096], b[8192] = np.nan, np.inf, np.nan
        a_list.append(a)
        b_list.append(b)
    return a_list, b_list


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd.engine import EVEngine
    eng = EVEngine(precision="mx")          # ev_compare needs no weights
    a_list, b_list = _batch(LENS)
    want = co.compare(a_list, b_list)
    got = eng.compare(a_list, b_list)
    yield dict(eng=eng, a=a_list, b=b_list, want=want, got=got)
    eng.close()


def _same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _assert_bits(got, want, name, keys=KEYS):
    for k in keys:
        w = np.asarray(want[k])
        assert _same_bits(np.asarray(got[k]), w.astype(np.asarray(got[k]).dtype)), (name, k, got[k], want[k])


def _segment_view(res, s):
    """Segment s of a result as a one-segment result."""
    o = res["chunk_offsets"]
    out = {k: np.asarray(res[k])[s:s + 1] for k in co.PER_SEGMENT}
    out["chunk_d2"], out["chunk_y2"] = res["chunk_d2"][o[s]:o[s + 1]], res["chunk_y2"][o[s]:o[s + 1]]
    out["chunk_offsets"] = np.array([0, o[s + 1] - o[s]], np.int64)
    return out


def test_bits_against_the_oracle(ctx):
    got, want = ctx["got"], ctx["want"]
    assert got["batch"] == len(LENS) and got["total"] == sum(LENS)
    _assert_bits(got, want, "batch")
    assert got["sum_d2"][SAME] == 0.0 and got["sum_d"][SAME] == 0.0 and got["rel_l2"][SAME] == 0.0 and got["rel_l2_ac"][SAME] == 0.0
    assert got["max_abs_d"][SAME] == 0.0 and got["argmax_d"][SAME] == 0
    assert got["sum_y2"][ZERO] == 0.0 and got["peak_y"][ZERO] == 0.0          # the floor branch: a finite, huge ratio
    assert got["rel_l2"][ZERO] == np.sqrt(got["sum_d2"][ZERO]) / np.sqrt(co.FLOOR) and np.isfinite(got["rel_l2_ac"][ZERO])
    assert list(got["nonfinite"]) == [3 if s == BAD else 0 for s in range(len(LENS))]
    assert all(np.isfinite(got[k]).all() for k in ("sum_d", "sum_d2", "sum_y", "sum_y2", "rel_l2", "rel_l2_ac", "max_abs_d", "chunk_d2", "chunk_y2"))
    ok = [s for s in range(len(LENS)) if s not in (SAME, ZERO) and LENS[s] > 1]          # 1e-3 noise on 0.1 AC + 0.3 DC
    assert (np.abs(got["rel_l2_ac"][ok] - 1e-2) < 3e-3).all() and (np.abs(got["rel_l2"][ok] - 1e-3 / np.hypot(0.1, 0.3)) < 1e-3).all()


def test_chunk_arrays_sum_to_the_segment_sums(ctx):
    got = ctx["got"]
    offs = got["chunk_offsets"]
    assert list(np.diff(offs)) == [-(-n // co.CHUNK) for n in LENS]
    for s in range(len(LENS)):
        for ck, sk in (("chunk_d2", "sum_d2"), ("chunk_y2", "sum_y2")):
            tot = np.float64(0.0)
            for c in got[ck][offs[s]:offs[s + 1]]:
                tot = tot + c
            assert tot.tobytes() == got[sk][s].tobytes(), (s, ck)


def test_position_and_memory_invariance(ctx):
    from emotivoice_amd import _ffi
    eng, a, b, got = ctx["eng"], ctx["a"], ctx["b"], ctx["got"]
    for s in range(len(LENS)):          # alone: offset 0, so the long segments take the float4 path
        _assert_bits(eng.compare([a[s]], [b[s]]), _segment_view(got, s), "alone %d" % s)
    order = list(reversed(range(len(LENS))))
    rev = eng.compare([a[s] for s in order], [b[s] for s in order])
    for p, s in enumerate(order):
        _assert_bits(_segment_view(rev, p), _segment_view(got, s), "moved %d" % s)
    d_a, d_b = torch.from_numpy(np.concatenate(a)).cuda(), torch.from_numpy(np.concatenate(b)).cuda()
    torch.cuda.synchronize()
    dev = eng.compare_to_numpy(eng.compare_raw(len(LENS), d_a.data_ptr(), d_b.data_ptr(), np.array(LENS, np.int64), _ffi.EV_FLAG_DEVICE_INPUTS))
    _assert_bits(dev, got, "device pointers")


def test_misaligned_offsets(ctx):
    """A first segment of one element puts every later chunk off 16-byte alignment: the element-wise path everywhere, the same bits."""
    from emotivoice_amd import _ffi
    lens = [1] + [n for n in LENS if n != 1]
    a, b = _batch(lens)
    want = co.compare(a, b)
    _assert_bits(ctx["eng"].compare(a, b), want, "host")
    d_a, d_b = torch.from_numpy(np.concatenate(a)).cuda(), torch.from_numpy(np.concatenate(b)).cuda()
    torch.cuda.synchronize()
    eng = ctx["eng"]
    _assert_bits(eng.compare_to_numpy(eng.compare_raw(len(lens), d_a.data_ptr(), d_b.data_ptr(), np.array(lens, np.int64), _ffi.EV_FLAG_DEVICE_INPUTS)),
                 want, "device")
    for s, n in enumerate(lens):          # and each segment's bits are those it has in the aligned batch
        _assert_bits(_segment_view(want, s), _segment_view(ctx["got"], LENS.index(n)), "segment %d" % n)


# Segments of 64, 65, 130 and 63 chunks (plus rests of 1, 7 and 100 elements): compare_finish adds chunk sums in groups of 64 with the next group in
# flight, and its fifth wave walks the chunks at stride 64, so only a segment beyond 64 chunks reaches the second and later rounds of either loop.
LONG = [64 * 4096, 65 * 4096 + 1, 130 * 4096 + 7, 63 * 4096 + 100]
LONG_ARGMAX = [63 * 4096 + 11, 64 * 4096 + 5, 70 * 4096 + 9, 62 * 4096 + 4095]
LONG_NONFINITE = [0, 1, 3, 0]


def _long_batch():
    a, b = _batch(LONG, seed=13)
    for s, i in enumerate(LONG_ARGMAX):          # |d| = 0.5 exactly, far above the 1e-3 noise
        b[s][i], a[s][i] = 0.25, 0.75
    b[1][65 * 4096], a[1][65 * 4096] = 0.25, -0.25          # the same |d| again in the one-element rest (chunk 65): the first index wins
    b[2][129 * 4096 + 3], a[2][129 * 4096 + 3] = 0.25, -0.25          # and in the last full chunk of the third group
    a[1][64 * 4096 + 4095] = np.nan          # the last element of chunk 64
    a[2][3 * 4096 + 1], a[2][64 * 4096], b[2][128 * 4096 + 4095] = np.inf, np.nan, -np.inf          # chunks 3, 64 and 128: one per group of 64
    return a, b


def test_segments_beyond_64_chunks(ctx):
    from emotivoice_amd import _ffi
    eng = ctx["eng"]
    a, b = _long_batch()
    want = co.compare(a, b)
    assert list(want["argmax_d"]) == LONG_ARGMAX and list(want["nonfinite"]) == LONG_NONFINITE and (want["max_abs_d"] == 0.5).all()
    assert list(np.diff(want["chunk_offsets"])) == [64, 66, 131, 64]
    got = eng.compare(a, b)
    _assert_bits(got, want, "long batch")
    for s in range(len(LONG)):          # alone (offset 0: the float4 path in every full chunk; in the batch everything after segment 1 is misaligned)
        _assert_bits(eng.compare([a[s]], [b[s]]), _segment_view(want, s), "long alone %d" % s)
    order = [2, 0, 3, 1]
    rev = eng.compare([a[s] for s in order], [b[s] for s in order])
    for p, s in enumerate(order):
        _assert_bits(_segment_view(rev, p), _segment_view(want, s), "long moved %d" % s)
    d_a, d_b = torch.from_numpy(np.concatenate(a)).cuda(), torch.from_numpy(np.concatenate(b)).cuda()
    torch.cuda.synchronize()
    dev = eng.compare_to_numpy(eng.compare_raw(len(LONG), d_a.data_ptr(), d_b.data_ptr(), np.array(LONG, np.int64), _ffi.EV_FLAG_DEVICE_INPUTS))
    _assert_bits(dev, want, "long device pointers")


def test_rejections_leave_the_previous_result_readable(ctx):
    from emotivoice_amd import _ffi
    eng, lib = ctx["eng"], _ffi.lib()
    a, b = np.concatenate(ctx["a"][:3]), np.concatenate(ctx["b"][:3])
    lens = np.array(LENS[:3], np.int64)
    good = eng.compare_raw(3, a.ctypes.data, b.ctypes.data, lens)
    before = eng.compare_to_numpy(good)

    def call(B=3, pa=a.ctypes.data, pb=b.ctypes.data, ln=lens, size=C.sizeof(_ffi.ev_compare_result), out=True):
        res = _ffi.ev_compare_result()
        res.struct_size = size
        rc = lib.ev_compare(eng._h, B, C.c_void_p(pa), C.c_void_p(pb), ln.ctypes.data_as(C.c_void_p) if ln is not None else None, 0,
                            C.byref(res) if out else None)
        return rc, lib.ev_last_error(eng._h).decode()

    zero, huge = lens.copy(), lens.copy()
    zero[1], huge[2] = 0, 1 << 62          # a length no chunk table can hold: refused, not attempted
    for kw, needle in ((dict(size=C.sizeof(_ffi.ev_compare_result) - 8), "struct_size"), (dict(B=0), "B = 0"), (dict(B=65536), "B = 65536"),
                       (dict(ln=zero), "lens[1]"), (dict(ln=huge), "lens[2]"), (dict(pa=None), "a is NULL"), (dict(pb=None), "b is NULL"), (dict(ln=None), "lens is NULL"),
                       (dict(out=False), "out is NULL")):
        rc, msg = call(**kw)
        assert rc < 0 and needle in msg, (kw, rc, msg)
        _assert_bits(eng.compare_to_numpy(good), before, str(kw))          # the arrays the earlier struct points at are untouched
    assert call()[0] == 0


# ------------------------------------------------------------------------------------------------------------- the guard on hardware
def _fixture(name):
    from emotivoice_amd.packer import pack_state_dict
    from emotivoice_amd.synthetic import synth_state_dict
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    sd = synth_state_dict(int(g["weight_seed"]), str(g["dur_mode"]))
    utt = dict(ling=g["in_ling"], speaker=int(g["in_speaker"]), style=g["in_style"], content=g["in_content"])
    return sd, pack_state_dict(sd), utt


def _parity_engine(prec, blob):
    """An engine as tests/test_gpu_parity.py's _engine builds it."""
    from emotivoice_amd.engine import EVEngine
    from test_gpu_parity import MODES
    dp, vp = MODES[prec]
    eng = EVEngine(decoder_precision=dp, vocoder_precision=vp, keep_stages=True, mx_residual="planes", token_splitk=True, mx_act_format="e5m2", mx_group=True)
    eng.load_blob(*blob)
    return eng


def test_mx_against_strict_on_the_device_equals_the_host_measure():
    from emotivoice_amd import _ffi
    from test_gpu_parity import rel_l2_ac
    _, blob, utt = _fixture("n28_zero_dc")
    strict, mx = _parity_engine("strict", blob), _parity_engine("mx", blob)
    try:
        ys, _ = strict._synthesize_call([utt], 1.0, 0, None, None)
        dur = strict.d2h(ys.durations, (ys.total_tokens,), np.int64)
        xs, _ = mx._synthesize_call([utt], 1.0, 0, dur, None)
        assert xs.total_samples == ys.total_samples > 0
        n = int(ys.total_samples)
        got = strict.compare_to_numpy(strict.compare_raw(1, xs.wav, ys.wav, np.array([n], np.int64), _ffi.EV_FLAG_DEVICE_INPUTS))
        host = rel_l2_ac(mx.d2h(xs.wav, (n,), np.float32), strict.d2h(ys.wav, (n,), np.float32))
        print("mx vs strict on n28_zero_dc: device rel_l2_ac %.6e, host %.6e, max |d| %.3e" % (got["rel_l2_ac"][0], host, got["max_abs_d"][0]))
        assert got["nonfinite"][0] == 0
        assert abs(got["rel_l2_ac"][0] - host) <= 1e-9 * host
        assert got["rel_l2_ac"][0] < 1e-3
    finally:
        strict.close()
        mx.close()


def test_ladder_on_hardware_rejects_fast_and_picks_mx():
    """fp16 operands measure 2.6e-3 .. 4.3e-3 on zero-mean audio (README; profiles/r6_l_parity_report.json has 2.7e-3 for this fixture), mx 4.6e-4."""
    from emotivoice_amd.config import EVShapes
    from emotivoice_amd.precision_guard import choose_precision
    _, blob, utt = _fixture("n64_hot_zdc")
    ladder = [("fast", {}), ("mx", {}), ("strict", {})]
    rep = choose_precision(EVShapes(), blob, probe=[utt], ladder=ladder, bar=1e-3)
    print(rep.line())
    assert [r["name"] for r in rep.rungs] == ["fast", "mx"] and [r["accepted"] for r in rep.rungs] == [False, True]
    assert rep.rungs[0]["worst_rel_l2_ac"] > 1e-3 >= rep.rungs[1]["worst_rel_l2_ac"] > 0 and rep.rungs[0]["nonfinite"] == 0
    assert (rep.chosen, rep.chosen_kwargs, rep.chosen_index) == ("mx", {}, 1)
    wc = rep.rungs[1]["worst_chunk"]
    assert wc["utterance"] == 0 and wc["offset"] % co.CHUNK == 0 and wc["ratio"] >= rep.rungs[1]["worst_rel_l2_ac"] * 0.5
    assert len(rep.rungs[1]["mel_rel_l2"]) == 1 and 0 < rep.rungs[1]["mel_rel_l2"][0] < 1e-3
    rep = choose_precision(EVShapes(), blob, probe=[utt], ladder=ladder, bar=1e-9)
    assert (rep.chosen, rep.chosen_index) == ("strict", 2) and [r["accepted"] for r in rep.rungs] == [False, False, True]


def test_verified_load_keeps_the_bits_of_mx():
    import warnings
    from emotivoice_amd.generator import JETSGeneratorHIP
    from emotivoice_amd.synthetic import synth_inputs, synth_state_dict
    sd = synth_state_dict(0, "parity")
    u = synth_inputs(7, [40])[0]
    args = (u["ling"][None], np.array([40]), np.array([u["speaker"]]), u["style"][None], u["content"][None])
    plain = JETSGeneratorHIP(None).to("cuda:0")
    gen = JETSGeneratorHIP(None).to("cuda:0")
    try:
        plain.load_state_dict(sd)
        assert plain.precision_report is None
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert gen.load_state_dict(sd, verify=True) is gen
        rep = gen.precision_report
        print(rep.line())
        assert rep is not None and rep.as_dict()["rungs"]
        # this seeded checkpoint sits at 4.2e-4 on the default probe (profiles/compare_cost.json): mx holds the 1e-3 bar, nothing escalates
        assert (rep.chosen, rep.chosen_kwargs, rep.escalated) == ("mx", {}, False) and len(w) == 0
        assert (gen._precision, gen._engine_kwargs) == (rep.chosen, rep.chosen_kwargs)
        out, base = gen(*args), plain(*args)
        assert np.isfinite(out["wav_predictions"]).all()
        for k in ("wav_predictions", "dec_outputs", "log_duration_predictions"):
            assert np.array_equal(np.asarray(out[k]), np.asarray(base[k])), k
    finally:
        plain.close()
        gen.close()
