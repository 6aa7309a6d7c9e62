"""Per-kernel parity tests (MI355X) of the non-GEMM kernels: every kernel of ev_misc.hip below attention and both kernels of
ev_align.hip, launched through their ev_op_* entry points (include/evhip_ops.h) against float64 references written from the
operation's definition (tests/misc_ops_ref.py; tests/test_misc_ops_ref.py ties those to oracle/ on the CPU).

Measure: the WORST ROW's relative L2 (max-abs for scalar-per-row outputs), not the whole tensor.  Bound of every floating-point case:
4 x what the plain fp32 torch op on the CPU measures against the same reference on the same inputs (misc_ops_ref.BASELINES),
floored at 4 fp32 ulp of the row norm.  Gathers, maps, integer durations, MAS paths and wav_to_i16 are compared exactly.  Every output
buffer carries sentinel guard rows that must survive; rows the contract zeroes must be exactly zero; rows a kernel must not use hold NaN.
What the kernels measured on the card is written to misc_ops_report.json, next to parity_report.json (key -> [measured, bound]).

Measured on an MI355X (worst case of each family in misc_ops_report.json of one full run; measured / bound):
    align_score 3.35e-07 / 8.68e-07 (max-abs 2.40e-04 / 9.59e-04)    bert_pooler 9.82e-08 / 1.05e-06    cond_vector 9.71e-08 / 9.90e-07
    conv_post fp16 1.55e-05 / 3.44e-05, fp32 k = 7 7.27e-06 / 3.07e-05, fp32 other k 1.46e-05 / 7.37e-05 (max-abs of the sample)
    durations, float alpha: centres 5.90e-08 / 4.77e-07 (6.4e-07 before the kernel summed them in double: the one failure this file found)
    gauss_upsample 1.71e-07 / 9.19e-07    pe_extend 2.93e-08 / 4.77e-07    var_embed_add 8.81e-08 / 4.77e-07
Attention and LayerNorm (tests/test_gpu_ops.py, same rules): DESIGN.md section 4, "Test layers".
"""
import numpy as np
import pytest

import misc_ops_ref as R
from test_gpu_parity import _report as write_report

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPORT = {}
SENT = 12345.0


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from emotivoice_amd import _ffi
    return _ffi.lib()


def _report(key, measured, bnd):
    """keeps the worst figure per key, asserts it, and rewrites the report file"""
    old = REPORT.get(key, [0.0, bnd])
    write_report(key, [max(old[0], float(measured)), float(bnd)], "misc_ops_report.json", REPORT)
    print("%-40s measured %.3e bound %.3e" % (key, measured, bnd))


def _check(key, measured, subkey=None):
    bnd = R.bound(R.BASELINES[key])
    _report(key if subkey is None else key + ":" + subkey, measured, bnd)
    assert measured <= bnd, (key, subkey, measured, bnd)


_KEEP = []


def dev(a):
    """numpy -> device tensor, kept alive until the test ends (a launch takes raw pointers: a temporary would be freed and its block reused)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_device_inputs():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


class Guarded:
    """[pre | rows | post] x cols device buffer filled with a sentinel; .p = pointer of the logical row 0"""

    def __init__(self, rows, cols, dtype=torch.float32, pre=8, post=8, fill=SENT):
        self.rows, self.pre = rows, pre
        self.full = torch.full((pre + rows + post, cols) if cols else (pre + rows + post,), fill, dtype=dtype, device="cuda")
        self.view = self.full[pre:pre + rows]
        self.p = self.view.data_ptr()
        self.fill = fill

    def get(self):
        torch.cuda.synchronize()
        f = self.full.cpu().numpy()
        g = np.concatenate([f[:self.pre].ravel(), f[self.pre + self.rows:].ravel()])
        assert (g == np.asarray(self.fill).astype(g.dtype)).all(), "guard rows overwritten"
        return f[self.pre:self.pre + self.rows]


def layout(lens, gap=4, lead=4):
    """gap layout: first row of each utterance, total rows, and the (seq, pos, valid) maps"""
    offs, r = [], lead
    for n in lens:
        offs.append(r)
        r += n + gap
    seq, pos, valid = np.full(r, -1, np.int32), np.zeros(r, np.int32), np.zeros(r, np.uint8)
    for b, (o, n) in enumerate(zip(offs, lens)):
        seq[o:o + n], pos[o:o + n], valid[o:o + n] = b, np.arange(n), 1
    return np.array(offs, np.int32), r, seq, pos, valid


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def i32(a):
    return dev(np.asarray(a, np.int32))


# --------------------------------------------------------------------------- exact: row maps, gathers, packing, int16
@pytest.mark.parametrize("B,rows_mod", [(1, 0), (3, 1), (256, 77)])
def test_row_maps_exact(lib, B, rows_mod):
    """row_maps_kernel: binary search over the utterance offsets; utterances of length 1, B = 1 and B = 256, rows not a multiple of 256"""
    rng = np.random.default_rng(B)
    lens = rng.integers(1, 40, B)
    lens[0] = 1
    offs, rows, seq, pos, valid = layout(lens, gap=4, lead=0 if B == 1 else 4)
    rows += rows_mod
    seq, pos, valid = (np.concatenate([a, np.full(rows_mod, f, a.dtype)]) for a, f in ((seq, -1), (pos, 0), (valid, 0)))
    gs, gp, gv = Guarded(rows, 0, torch.int32, fill=77), Guarded(rows, 0, torch.int32, fill=77), Guarded(rows, 0, torch.uint8, pre=16, post=16, fill=77)
    assert lib.ev_op_row_maps(i32(offs).data_ptr(), i32(lens).data_ptr(), B, gs.p, gp.p, gv.p, rows, None) == 0
    assert np.array_equal(gs.get(), seq) and np.array_equal(gp.get(), pos) and np.array_equal(gv.get(), valid)
    assert lib.ev_op_row_maps(None, None, 0, gs.p, gp.p, gv.p, rows, None) == -2


@pytest.mark.parametrize("C_", [384, 768])
def test_embed_pe_and_bert_embed_exact(lib, C_):
    """embed_pe_kernel / bert_embed_kernel: gathers + fp32 adds in the documented order; out-of-range ids clamp, type_ids NULL = type 0,
    position >= max_pos clamps to the last row, gap rows zero"""
    rng = np.random.default_rng(C_)
    lens = [1, 7, 40]
    offs, rows, seq, pos, valid = layout(lens)
    cu = cu_of(lens)
    V, max_pos, n_types = 50, 32, 2
    ids = rng.integers(0, V, cu[-1]).astype(np.int64)
    ids[[0, 3, 9]] = [-5, V, V + 1000]                         # documented clamping
    types = rng.integers(0, n_types, cu[-1]).astype(np.int64)
    types[5] = 7
    emb, pe = rng.standard_normal((V, C_)).astype(np.float32), rng.standard_normal((64, C_)).astype(np.float32)
    temb = rng.standard_normal((n_types, C_)).astype(np.float32)
    cid = np.clip(ids, 0, V - 1)
    d = dict(ids=dev(ids), cu=i32(cu), seq=i32(seq), pos=i32(pos), emb=dev(emb), pe=dev(pe), temb=dev(temb), types=dev(types))
    for alpha in (1.0, 0.5, 1.7):
        out, tap = Guarded(rows, C_), Guarded(rows, C_)
        assert lib.ev_op_embed_pe(d["ids"].data_ptr(), d["cu"].data_ptr(), d["seq"].data_ptr(), d["pos"].data_ptr(), d["emb"].data_ptr(), V,
                                  d["pe"].data_ptr(), alpha, out.p, tap.p, rows, C_, None) == 0
        got, gtap = out.get(), tap.get()
        assert not got[valid == 0].any() and not gtap[valid == 0].any()
        for b, (o, n) in enumerate(zip(offs, lens)):
            e = emb[cid[cu[b]:cu[b] + n]]
            assert np.array_equal(gtap[o:o + n], e)
            two_step = e + np.float32(alpha) * pe[:n]                      # mul then add, each rounded
            fused = R.fma32(np.float32(alpha), pe[:n], e)                   # a contracted multiply-add rounds once
            if alpha in (1.0, 0.5):
                assert np.array_equal(two_step, fused)                      # the product is exact: one possible result
            assert ((got[o:o + n] == two_step) | (got[o:o + n] == fused)).all(), (alpha, b)
    for with_types in (True, False):
        out = Guarded(rows, C_)
        assert lib.ev_op_bert_embed(d["ids"].data_ptr(), d["types"].data_ptr() if with_types else None, d["cu"].data_ptr(), d["seq"].data_ptr(),
                                    d["pos"].data_ptr(), d["emb"].data_ptr(), d["pe"].data_ptr(), d["temb"].data_ptr(), V, max_pos, n_types, out.p,
                                    rows, C_, None) == 0
        got = out.get()
        assert not got[valid == 0].any()
        for b, (o, n) in enumerate(zip(offs, lens)):
            tt = np.clip(types[cu[b]:cu[b] + n], 0, n_types - 1) if with_types else np.zeros(n, np.int64)
            want = (emb[cid[cu[b]:cu[b] + n]] + temb[tt]) + pe[np.minimum(np.arange(n), max_pos - 1)]       # BertEmbeddings.forward's order
            assert np.array_equal(got[o:o + n], want), (with_types, b)
    assert lib.ev_op_embed_pe(None, None, None, None, None, V, None, 1.0, out.p, None, rows, 383, None) == -2


def test_prosody_tracks_exact(lib):
    """prosody_tracks_kernel: identity copies bit for bit (-0, denormals), NaN / inf overrides mean "predicted", gap rows +0, per-utterance
    controls in one batch; a non-identity transform is ONE fma"""
    rng = np.random.default_rng(5)
    lens = [1, 9, 300, 17]
    B = len(lens)
    offs, rows, seq, pos, valid = layout(lens)
    cu = cu_of(lens)
    pitch, energy = (rng.standard_normal(rows).astype(np.float32) for _ in range(2))
    pitch[offs[1]:offs[1] + 4] = [-0.0, 1e-42, -1e-42, 0.0]
    pitch[valid == 0] = np.nan                                  # gap rows of the predictions are not used
    energy[valid == 0] = np.nan
    povr, eovr = (rng.standard_normal(cu[-1]).astype(np.float32) for _ in range(2))
    povr[::3] = np.nan
    povr[1::7] = np.inf
    eovr[::2] = -np.inf
    eovr[cu[1] + 2] = -0.0
    ctrl = np.array([[1, 1, 1, 1], [1, 1, 1.25, 0.5], [0, 0, -0.3, 2.0], [1, 0.7, 1, 1.0], [0, 0.1, 0.0, -1.0]], np.float32)     # [5][B]
    for use_ovr in (False, True):
        po, eo = Guarded(rows, 0), Guarded(rows, 0)
        assert lib.ev_op_prosody_tracks(dev(pitch).data_ptr(), dev(energy).data_ptr(), i32(seq).data_ptr(), i32(pos).data_ptr(), i32(cu).data_ptr(),
                                        dev(povr).data_ptr() if use_ovr else None, dev(eovr).data_ptr() if use_ovr else None, dev(ctrl).data_ptr(), B,
                                        po.p, eo.p, rows, None) == 0
        for got, src, ovr, (sc, sh) in ((po.get(), pitch, povr, (1, 2)), (eo.get(), energy, eovr, (3, 4))):
            assert np.array_equal(got[valid == 0].view(np.uint32), np.zeros(int((valid == 0).sum()), np.uint32))       # +0, bit pattern included
            for b, (o, n) in enumerate(zip(offs, lens)):
                s = src[o:o + n].copy()
                if use_ovr:
                    v = ovr[cu[b]:cu[b] + n]
                    s = np.where(np.isfinite(v), v, s)
                want = s if (ctrl[sc, b] == 1 and ctrl[sh, b] == 0) else R.fma32(ctrl[sc, b], s, ctrl[sh, b])
                assert np.array_equal(got[o:o + n].view(np.uint32), want.view(np.uint32)), (use_ovr, b)


@pytest.mark.parametrize("in16,out32", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_mel_to_rows_exact(lib, in16, out32):
    """mel_to_rows_kernel<_Float16> / <float>: transposing gather, zero gap rows, zero pad channels (ldo > n_mels)"""
    rng = np.random.default_rng(3)
    n_mels, ldo, lens = 80, 96, [1, 5, 257, 30]
    offs, rows, seq, pos, valid = layout(lens)
    mels = [rng.standard_normal((n_mels, n)).astype(np.float16 if in16 else np.float32) for n in lens]
    eoff = np.concatenate([[0], np.cumsum([m.size for m in mels])])[:-1].astype(np.int64)
    flat = np.concatenate([m.ravel() for m in mels])
    out = Guarded(rows, ldo, torch.float32 if out32 else torch.float16, fill=7.0)
    assert lib.ev_op_mel_to_rows(dev(flat).data_ptr(), in16, dev(eoff).data_ptr(), i32(seq).data_ptr(), i32(pos).data_ptr(), i32(lens).data_ptr(), out.p,
                                 out32, rows, n_mels, ldo, None) == 0
    got = out.get()
    want = np.zeros((rows, ldo), np.float32 if out32 else np.float16)
    for o, n, m in zip(offs, lens, mels):
        want[o:o + n, :n_mels] = m.T.astype(want.dtype)
    assert np.array_equal(got, want)
    assert lib.ev_op_mel_to_rows(dev(flat).data_ptr(), in16, None, None, None, None, out.p, out32, rows, n_mels, 64, None) == -2


@pytest.mark.parametrize("in16", [0, 1])
def test_pack_rows_exact(lib, in16):
    """pack_rows_kernel: utterances of 1 row, a source pitch wider than C, and one utterance of more than 4096 x 256 elements (grid-stride loop)"""
    rng = np.random.default_rng(4)
    C_, ld, lens = 96, 128, [1, 11500, 33]                      # 11500 x 96 = 1.1 M elements > 4096 x 256
    offs, rows, _, _, _ = layout(lens)
    src = rng.standard_normal((rows, ld)).astype(np.float16 if in16 else np.float32)
    oo = cu_of(lens)[:-1].astype(np.int64)
    out = Guarded(int(sum(lens)), C_)
    assert lib.ev_op_pack_rows(dev(src).data_ptr(), in16, ld, C_, dev(offs.astype(np.int64)).data_ptr(), dev(oo).data_ptr(), i32(lens).data_ptr(), len(lens),
                               max(lens), out.p, None) == 0
    want = np.concatenate([src[o:o + n, :C_] for o, n in zip(offs, lens)]).astype(np.float32)
    assert np.array_equal(out.get(), want)


@pytest.mark.parametrize("n", [1, 255, 256, 2 ** 21 + 3])
def test_wav_to_i16_exact(lib, n):
    """wav_to_i16_kernel against the float64 statement of the C cast and against oracle.jets_oracle.wav_to_int16; 2^21 + 3 samples = the
    grid-stride tail (8192 blocks x 256 threads)"""
    from oracle.jets_oracle import wav_to_int16
    rng = np.random.default_rng(n)
    edge = R.wav_edge_values()
    w = rng.uniform(-1, 1, n).astype(np.float32)
    w[:min(n, len(edge))] = edge[:n]
    w[-min(n, len(edge)):] = edge[:min(n, len(edge))]
    out = Guarded(n, 0, torch.int16, pre=16, post=16, fill=1234)
    assert lib.ev_op_wav_to_i16(dev(w).data_ptr(), out.p, n, None) == 0
    got = out.get()
    assert np.array_equal(got, R.wav_to_i16(w)) and np.array_equal(got, wav_to_int16(w))
    assert lib.ev_op_wav_to_i16(None, None, 0, None) == -2


# --------------------------------------------------------------------------- durations (both instantiations)
DUR_NS = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2048]


def _dur_batch(seed, zero_utt=None):
    rng = np.random.default_rng(seed)
    logd = [R.draw_log_d(rng, n) for n in DUR_NS]
    if zero_utt is not None:
        logd[zero_utt] = np.full(DUR_NS[zero_utt], -2.0, np.float32)      # exp(-2) - 1 < 0: every prediction is 0 -> the all-zero guard
    for ld in logd:
        assert (R.durations(ld)[1] > R.DUR_NEAR).all()                   # no token near a rounding boundary: every token is compared exactly
    return logd


def _run_durations(lib, logd, pros, alpha=1.0, alpha_b=None, forced=None, partial=None, cap=1024):
    lens = [len(x) for x in logd]
    B = len(lens)
    offs, rows, _, _, valid = layout(lens)
    cu = cu_of(lens)
    rows_ld = np.full(rows, np.nan, np.float32)                           # gap rows of log_d are never read
    for o, x in zip(offs, logd):
        rows_ld[o:o + len(x)] = x
    tot = int(cu[-1])
    dp, de, lp = Guarded(tot, 0, torch.int64, fill=-7), Guarded(tot, 0, torch.int64, fill=-7), Guarded(tot, 0)
    ce, ml = Guarded(rows, 0), Guarded(B, 0, torch.int32, fill=-7)
    keep = [dev(rows_ld), i32(offs), i32(lens), i32(cu)]
    f = dev(forced) if forced is not None else None
    pa = dev(partial) if partial is not None else None
    ab = dev(np.asarray(alpha_b, np.float32)) if alpha_b is not None else None
    if pros:
        rc = lib.ev_op_durations_prosody(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), B, alpha, ab.data_ptr() if ab is not None else None,
                                         pa.data_ptr() if pa is not None else None, cap, keep[3].data_ptr(), dp.p, de.p, lp.p, ce.p, ml.p, None)
    else:
        rc = lib.ev_op_durations(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), B, alpha, f.data_ptr() if f is not None else None,
                                 keep[3].data_ptr(), dp.p, lp.p, ce.p, ml.p, None)
    assert rc == 0
    cen = ce.get()
    assert (cen[valid == 0] == np.float32(SENT)).all()                    # centre rows of gaps are not written
    return dict(offs=offs, cu=cu, dur=dp.get(), eff=de.get() if pros else None, logd=lp.get(), centre=cen, mel_len=ml.get())


@pytest.mark.parametrize("pros", [False, True], ids=["durations_kernel<false>", "durations_kernel<true>"])
@pytest.mark.parametrize("mode", ["predicted", "forced", "forced_zero", "predicted_zero"])
def test_durations_alpha1_exact(lib, pros, mode):
    """alpha = 1: integer durations, mel_len and centres exact, B = 11 utterances of 1 .. 2048 tokens in one launch (the 256-token chunks, the
    cross-wave carry and the chunk carry are all crossed); the all-zero guard per utterance"""
    logd = _dur_batch(11, zero_utt=4 if mode == "predicted_zero" else None)
    rng = np.random.default_rng(12)
    tot = sum(DUR_NS)
    forced = partial = None
    if mode.startswith("forced"):
        fd = rng.integers(0, 20, tot).astype(np.int64)
        if mode == "forced_zero":
            c = cu_of(DUR_NS)
            fd[c[5]:c[6]] = 0
            fd[c[0]:c[1]] = 0
        forced, partial = (None, fd) if pros else (fd, None)
    r = _run_durations(lib, logd, pros, forced=forced, partial=partial, cap=1 << 20)
    for b, ld in enumerate(logd):
        n, c0, o = len(ld), r["cu"][b], r["offs"][b]
        pred = R.durations(ld)[0]
        assert np.array_equal(r["logd"][c0:c0 + n], ld)
        if pros or forced is None:
            assert np.array_equal(r["dur"][c0:c0 + n], pred), b
        eff = pred if not mode.startswith("forced") else (forced if forced is not None else partial)[c0:c0 + n]
        if pros:
            assert np.array_equal(r["eff"][c0:c0 + n], eff), b
        else:
            assert np.array_equal(r["dur"][c0:c0 + n], eff), b
        cen, T = R.centres(eff, 1.0)
        assert r["mel_len"][b] == T, b
        assert np.array_equal(r["centre"][o:o + n], cen.astype(np.float32)), b      # integers and halves below 2^24: exact in fp32


def test_durations_prosody_mixed_alpha_and_partial(lib):
    """durations_kernel<true>: alpha in {1, 0.5, 1.3} per utterance in one batch (each block takes its own branch), partial overrides clamped to
    dur_cap.  Integer outputs exact; alpha = 1 centres exact; float-alpha centres against the float64 cumsum, mel_len = int(float64 sum)"""
    logd = _dur_batch(21)
    rng = np.random.default_rng(22)
    tot = sum(DUR_NS)
    partial = np.where(rng.uniform(size=tot) < 0.4, rng.integers(0, 3000, tot), -1).astype(np.int64)
    alpha_b = [1.0, 0.5, 1.3, 1.0, 0.5, 1.3, 1.0, 0.5, 1.3, 1.0, 1.3]
    cap = 1024
    r = _run_durations(lib, logd, True, alpha=1.0, alpha_b=alpha_b, partial=partial, cap=cap)
    for b, ld in enumerate(logd):
        n, c0, o = len(ld), r["cu"][b], r["offs"][b]
        pred = R.durations(ld)[0]
        pa = partial[c0:c0 + n]
        eff = np.where(pa >= 0, np.minimum(pa, cap), pred)
        assert np.array_equal(r["dur"][c0:c0 + n], pred) and np.array_equal(r["eff"][c0:c0 + n], eff), b
        cen, T = R.centres(eff, alpha_b[b])
        assert r["mel_len"][b] == T, b
        if alpha_b[b] == 1.0:
            assert np.array_equal(r["centre"][o:o + n], cen.astype(np.float32)), b
        else:
            # these inputs are not the baseline's: the bound is 4 x what the fp32 CPU cumsum measures on THIS utterance (floor: 4 ulp)
            den = np.maximum(cen, 1.0)
            bnd = R.bound(R.max_abs(R.centres_f32(eff, alpha_b[b]) / den, cen / den))
            got = R.max_abs(r["centre"][o:o + n] / den, cen / den)
            _report("durations_alpha_centres:partial-n%d" % n, got, bnd)
            assert got <= bnd, (b, got, bnd)


def test_durations_float_alpha_centres(lib):
    """the float-alpha branch (a sequential fp32 running sum on one thread) on the baseline's own inputs, n up to 2048"""
    for key, cid, (d, alpha), ref, _ in R.alpha_centre_cases():
        n = len(d)
        lens = [n]
        offs, rows, _, _, _ = layout(lens)
        ld = np.zeros(rows, np.float32)
        dp, lp, ce, ml = Guarded(n, 0, torch.int64, fill=-7), Guarded(n, 0), Guarded(rows, 0), Guarded(1, 0, torch.int32, fill=-7)
        assert lib.ev_op_durations(dev(ld).data_ptr(), i32(offs).data_ptr(), i32(lens).data_ptr(), 1, alpha, dev(d).data_ptr(), i32([0, n]).data_ptr(),
                                   dp.p, lp.p, ce.p, ml.p, None) == 0
        got = ce.get()[offs[0]:offs[0] + n]
        assert np.array_equal(dp.get(), d) and ml.get()[0] == R.centres(d, alpha)[1], cid
        _check(key, R.max_abs(got / np.maximum(ref, 1.0), ref / np.maximum(ref, 1.0)), cid)


# --------------------------------------------------------------------------- Gaussian upsampling
@pytest.mark.parametrize("case", list(range(len(R.GAUSS_CASES))), ids=["C%d-%s-%s" % (c, "_".join(map(str, t)), k) for c, t, k in R.GAUSS_CASES])
def test_gauss_upsample(lib, case):
    """gauss_upsample_kernel: C in {128, 384, 512}, tokens 1 .. 2048, 16384 frames (two cases), runs of zero durations, one very long token, windows
    [jlo, jhi] of 1 .. 5 tokens (the 4-row unroll and its tail), tap NULL and non-NULL, out - tap == pe_alpha * pe as computed"""
    key, cid, utts = list(R.gauss_cases())[case]
    C_ = utts[0][0].shape[1]
    tl, fl = [u[0].shape[0] for u in utts], [u[2] for u in utts]
    toff, trows, _, _, _ = layout(tl)
    foff, frows, fseq, fpos, fvalid = layout(fl)
    x = np.full((trows, C_), np.nan, np.float32)                          # token gap rows are not used
    cen = np.full(trows, np.nan, np.float32)
    for o, u in zip(toff, utts):
        x[o:o + len(u[0])], cen[o:o + len(u[0])] = u[0], u[1]
    pe = np.random.default_rng(1).standard_normal((max(fl), C_)).astype(np.float32)
    keep = [dev(x), dev(cen), i32(toff), i32(tl), i32(fseq), i32(fpos), dev(pe)]
    if cid.endswith("wide"):
        assert {1, 4, 5} <= set(R.gauss_window_widths(utts[0][1], fl[0], 0.1).tolist())      # windows [jlo, jhi] of 1, 4 and 5 tokens occur
    first_tap = None
    for pe_alpha, with_tap in ((1.0, True), (0.75, True), (1.3, False)):
        out, tap = Guarded(frows, C_), Guarded(frows, C_)
        assert lib.ev_op_gauss_upsample(*(k.data_ptr() for k in keep), pe_alpha, 0.1, out.p, tap.p if with_tap else None, frows, C_, None) == 0
        got, gtap = out.get(), tap.get() if with_tap else None
        assert not got[fvalid == 0].any() and (gtap is None or not gtap[fvalid == 0].any())
        if with_tap:
            first_tap = gtap if first_tap is None else first_tap
            assert np.array_equal(gtap, first_tap)                         # the same bits whatever pe_alpha
        for o, u in zip(foff, utts):
            T = u[2]
            if with_tap:
                _check(key, R.worst_row_rel(gtap[o:o + T], u[3]), cid)
                two_step = gtap[o:o + T] + np.float32(pe_alpha) * pe[:T]   # mul then add, each rounded
                fused = R.fma32(np.float32(pe_alpha), pe[:T], gtap[o:o + T])     # a contracted multiply-add rounds once
                assert ((got[o:o + T] == two_step) | (got[o:o + T] == fused)).all()
            else:
                fused = R.fma32(np.float32(pe_alpha), pe[:T], first_tap[o:o + T])
                two_step = first_tap[o:o + T] + np.float32(pe_alpha) * pe[:T]
                assert ((got[o:o + T] == two_step) | (got[o:o + T] == fused)).all()      # tap == NULL changes nothing in out
    assert lib.ev_op_gauss_upsample(*(k.data_ptr() for k in keep), 1.0, 0.1, out.p, None, frows, 640, None) == -2      # channels above 512 would be dropped


# --------------------------------------------------------------------------- pitch / energy embedding add
def test_var_embed_add(lib):
    """var_embed_add_kernel: k in {1, 3, 9} x C in {128, 384}; utterances of 1, 2, k - 1, k rows at the minimum gap ((k - 1) / 2 zero rows), so every
    halo position is hit; invalid rows exactly zero"""
    for key, cid, (wp, bp, we, be), utts in R.var_embed_cases():
        k, C_ = wp.shape
        half = (k - 1) // 2
        lens = [u[0].shape[0] for u in utts]
        offs, rows, _, _, valid = layout(lens, gap=max(half, 1), lead=max(half, 1))
        x = np.full((rows, C_), np.nan, np.float32)                       # x on invalid rows is not used
        p, e = np.zeros(rows, np.float32), np.zeros(rows, np.float32)     # gap scalars are the conv's zero padding: read, so they stay zero
        for o, u in zip(offs, utts):
            n = len(u[1])
            x[o:o + n], p[o:o + n], e[o:o + n] = u[0], u[1], u[2]
        out = Guarded(rows, C_)
        assert lib.ev_op_var_embed_add(dev(x).data_ptr(), dev(p).data_ptr(), dev(e).data_ptr(), dev(wp).data_ptr(), dev(bp).data_ptr(), dev(we).data_ptr(),
                                       dev(be).data_ptr(), dev(valid).data_ptr(), out.p, rows, C_, k, None) == 0
        got = out.get()
        assert not got[valid == 0].any()
        for o, u in zip(offs, utts):
            _check(key, R.worst_row_rel(got[o:o + len(u[1])], u[3]), cid)
    assert lib.ev_op_var_embed_add(None, None, None, None, None, None, None, dev(valid).data_ptr(), out.p, rows, C_, 4, None) == -2


# --------------------------------------------------------------------------- conv_post (three kernels behind one launcher)
@pytest.mark.parametrize("kind", list(R.CONV_POST_KINDS), ids=["conv_post_kernel<32,__half>", "conv_post_f32_kernel<32,7>", "conv_post_kernel<32,float>"])
def test_conv_post(lib, kind):
    """launch_conv_post picks conv_post_kernel<32, __half> for fp16 input, conv_post_f32_kernel<32, 7> for fp32 input with k == 7 and
    conv_post_kernel<32, float> for fp32 input with any other k.  rows {1, 255, 256, 257, 1000}: the 256-row blocks' halo rows; the utterance
    starts at row 0 of the layout, so the k / 2 rows on both sides are the zero rows the contract requires; valid_shift {0, 8}"""
    is_f32, _ = R.CONV_POST_KINDS[kind]
    for key, cid, (x, w, bias, slope), ref, _ in R.conv_post_cases(kind):
        rows, k = x.shape[0], w.shape[0]
        blocks = (rows + 255) // 256
        xin = torch.zeros(16 + blocks * 256 + 16, 32, dtype=torch.float32 if is_f32 else torch.float16, device="cuda")     # readable zero halo
        xin[16:16 + rows] = dev(x)
        for shift in (0, 8):
            nv = ((rows - 1) >> shift) + 1
            valid = np.ones(nv, np.uint8)
            if shift == 0 and rows > 20:
                valid[17] = 0
            wav = Guarded(rows, 0, pre=16, post=16)
            assert lib.ev_op_conv_post(xin[16:].data_ptr(), int(is_f32), 32, dev(w).data_ptr(), bias, k, 1.0 if slope is None else slope, dev(valid).data_ptr(),
                                       shift, wav.p, rows, 32, None) == 0
            got = wav.get()
            want = ref.copy()
            if shift == 0 and rows > 20:
                assert got[17] == 0
                want[17] = 0
            _check(key, R.max_abs(got, want), cid)
            sat = np.abs(want) == 1.0                                     # float64 tanh saturates to exactly +-1 beyond |a| ~ 19
            if rows >= 255:
                assert sat.any()
            assert np.array_equal(got[sat], want[sat].astype(np.float32))
    v1 = torch.ones(4, dtype=torch.uint8, device="cuda")
    for bad in (dict(C=64), dict(k=4), dict(k=17), dict(slope=1.5), dict(ldx=33)):
        a = dict(C=32, k=7, slope=0.5, ldx=32)
        a.update(bad)
        assert lib.ev_op_conv_post(xin[16:].data_ptr(), int(is_f32), a["ldx"], dev(w).data_ptr(), 0.0, a["k"], a["slope"], v1.data_ptr(), 0, wav.p, 4, a["C"],
                                   None) == -2, bad


# --------------------------------------------------------------------------- cond_vector / bert_pooler / pe_extend
def test_cond_vector_and_bert_pooler(lib):
    """cond_vector_kernel, bert_pooler_kernel: C in {384, 768}, B in {1, 5}, speaker ids 0 and n_speaker - 1"""
    for key, cid, inp, ref, _ in R.dense_cases():
        if key == "cond_vector":
            spk, style, content, emb, W, bias = inp
            B, C_ = ref.shape
            out = Guarded(B, C_)
            assert lib.ev_op_cond_vector(dev(spk).data_ptr(), dev(style).data_ptr(), dev(content).data_ptr(), dev(emb).data_ptr(), emb.shape[0],
                                         dev(W).data_ptr(), dev(bias).data_ptr(), out.p, B, C_, style.shape[1], None) == 0
        else:
            h0, W, bias = inp
            B, C_ = ref.shape
            offs, rows, _, _, _ = layout([3] * B)
            x = np.full((rows, C_ + 8), np.nan, np.float32)               # only the first row of each text is read
            x[offs, :C_] = h0
            out = Guarded(B, C_)
            assert lib.ev_op_bert_pooler(dev(x).data_ptr(), C_ + 8, i32(offs).data_ptr(), dev(W).data_ptr(), dev(bias).data_ptr(), out.p, B, C_, None) == 0
        _check(key, R.worst_row_rel(out.get(), ref), cid)


def test_pe_extend(lib):
    """pe_extend_kernel: rows [4096, 16384) at C = 384 against sin / cos in float64 of the fp32-rounded angle float32(t) * div[i]"""
    div = R.pe_div(384)
    pe = Guarded(16384, 384)
    for key, cid, (r0, r1, _), ref, _ in R.pe_cases():
        assert lib.ev_op_pe_extend(pe.p, dev(div).data_ptr(), r0, r1, 384, None) == 0
        got = pe.get()
        assert (got[:4096] == np.float32(SENT)).all()
        _check(key, R.worst_row_rel(got[r0:r1], ref), cid)
    assert lib.ev_op_pe_extend(pe.p, dev(div).data_ptr(), 8, 8, 384, None) == -2


# --------------------------------------------------------------------------- aligner: score
def _host(a, t):
    return np.ascontiguousarray(np.asarray(a, t))


def _align_score(lib, text, feats):
    N, C_ = text.shape
    T = feats.shape[0]
    lp = Guarded(T * N, 0, pre=64, post=64)
    tr, fr = np.full((4 + N + 4, C_), np.nan, np.float32), np.full((4 + T + 4, C_), np.nan, np.float32)
    tr[4:4 + N], fr[4:4 + T] = text, feats
    hs = [_host([4], np.int32), _host([N], np.int32), _host([4], np.int32), _host([T], np.int32), _host([0], np.int64)]
    assert lib.ev_op_align_score(dev(tr).data_ptr(), dev(fr).data_ptr(), C_, 1, *(h.ctypes.data for h in hs), lp.p, None) == 0
    return lp.get().reshape(T, N)


def test_align_score(lib):
    """align_score_kernel: C in {32, 384}, (T, N) from (1, 1) to (4096, 1024), a frame equal to a token (distance 0), all distances large"""
    for key, cid, (text, feats), ref, _ in R.align_score_cases():
        got = _align_score(lib, text, feats)
        assert np.isfinite(got).all()
        _check(key, R.worst_row_rel(got, ref), cid)
        _check(key + "/maxabs", R.max_abs(got, ref), cid)
    z = np.zeros(1, np.int32)
    assert lib.ev_op_align_score(None, None, 48, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, None, None, None) == -2


# --------------------------------------------------------------------------- aligner: monotonic alignment search, every RM
MAS_NS = [1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048]


def _mas_shapes():
    out = []
    for N in MAS_NS:
        for T in sorted({N, N + 1, 3 * N}):
            out.append((N, T))
    return out + [(2048, 16384), (300, 16384)]


def _rm(n):
    rm = 1
    while rm * 64 < n:
        rm *= 2
    return rm


def _run_mas(lib, lps, tracks=None):
    """one launch over the utterances lps[b] (T_b, N_b); returns per-utterance (dur, score, pitch_tok, energy_tok)"""
    B = len(lps)
    Ts, Ns = [lp.shape[0] for lp in lps], [lp.shape[1] for lp in lps]
    lp_off = np.concatenate([[0], np.cumsum([lp.size for lp in lps])]).astype(np.int64)
    tokp, frmp = cu_of(Ns).astype(np.int64), cu_of(Ts).astype(np.int64)
    flat = dev(np.concatenate([lp.ravel() for lp in lps]))
    bits = torch.zeros(int(frmp[-1]) * 64 + 64, dtype=torch.int32, device="cuda")
    dur, sc = Guarded(int(tokp[-1]), 0, torch.int64, fill=-7), Guarded(B, 0)
    pt, et = Guarded(int(tokp[-1]), 0), Guarded(int(tokp[-1]), 0)
    pf = dev(np.concatenate(tracks[0])) if tracks else None
    ef = dev(np.concatenate(tracks[1])) if tracks else None
    hs = [_host(Ns, np.int32), _host(Ts, np.int32), lp_off[:-1].copy(), tokp[:-1].copy(), frmp[:-1].copy(), (frmp[:-1] * 64).copy()]
    assert lib.ev_op_align_mas(flat.data_ptr(), B, *(h.ctypes.data for h in hs), bits.data_ptr(), pf.data_ptr() if tracks else None,
                               ef.data_ptr() if tracks else None, dur.p, pt.p if tracks else None, et.p if tracks else None, sc.p, None) == 0
    d, s, p, e = dur.get(), sc.get(), pt.get(), et.get()
    return [(d[tokp[b]:tokp[b + 1]], s[b], p[tokp[b]:tokp[b + 1]], e[tokp[b]:tokp[b + 1]]) for b in range(B)]


@pytest.mark.parametrize("kind", ["random", "quantised"])
def test_align_mas_every_rm(lib, kind):
    """mas_kernel<1>, <2>, <4>, <8>, <16>, <32>: launch_align_mas picks RM = the power of two with 64 RM >= the batch's longest utterance, so N = 1 / 64
    run <1>, 65 / 128 <2>, 129 / 256 <4>, 257 / 512 <8>, 513 / 1024 <16>, 1025 / 2048 <32> when launched alone, and everything runs <32> in the mixed
    batch; both must give the same bits.  T in {N (the diagonal is the only path), N + 1, 3 N}, and 16384 for N = 2048 and N = 300.
    random: negative fp32 log_p.  quantised: multiples of 1 / 8 in [-16, 0] -- fp64 sums are exact, ties are frequent, and the path is then decided by the
    `>=` rule on the forward bit and in the backtrack.  Path (durations), score and per-token means against tests/align_oracle.py: mas_fast, exact."""
    import align_oracle as AO
    rng = np.random.default_rng(77 if kind == "random" else 78)
    shapes = _mas_shapes()
    lps, tracks = [], ([], [])
    for N, T in shapes:
        if kind == "random":
            lp = (-rng.gamma(2.0, 2.0, (T, N))).astype(np.float32)
        else:
            lp = (-rng.integers(0, 129, (T, N)) / 8.0).astype(np.float32)
        lps.append(lp)
        tracks[0].append(rng.standard_normal(T).astype(np.float32))
        tracks[1].append(rng.standard_normal(T).astype(np.float32))
    want = []
    for lp, pf, ef in zip(lps, *tracks):
        A = AO.mas_fast(lp)
        want.append(R.mas_outputs(lp, A, (pf, ef)))
    mixed = _run_mas(lib, lps, tracks)
    seen_rm = set()
    for i, ((N, T), lp) in enumerate(zip(shapes, lps)):
        d, s, (pm, em) = want[i]
        assert d.sum() == T and (T != N or (d == 1).all())
        solo = _run_mas(lib, [lp], ([tracks[0][i]], [tracks[1][i]]))[0]
        notrack = _run_mas(lib, [lp], None)[0]
        seen_rm.add(_rm(N))
        for name, got in (("mixed<32>", mixed[i]), ("solo<%d>" % _rm(N), solo)):
            assert np.array_equal(got[0], d), (name, N, T)
            assert got[1].view(np.uint32) == np.float32(s).view(np.uint32), (name, N, T, got[1], s)
            assert np.array_equal(got[2].view(np.uint32), pm.view(np.uint32)) and np.array_equal(got[3].view(np.uint32), em.view(np.uint32)), (name, N, T)
        assert np.array_equal(notrack[0], d) and notrack[1] == solo[1]
        assert (notrack[2] == np.float32(SENT)).all()                    # NULL tracks: the per-token outputs are not written
    assert seen_rm == {1, 2, 4, 8, 16, 32}
    t, z = torch.zeros(64, device="cuda"), np.zeros(1, np.int64)
    for N, T in ((5, 4), (2049, 4000), (8, 16385)):                      # fewer frames than tokens; more than 2048 tokens; more than 16384 frames
        assert lib.ev_op_align_mas(t.data_ptr(), 1, _host([N], np.int32).ctypes.data, _host([T], np.int32).ctypes.data, z.ctypes.data, z.ctypes.data,
                                   z.ctypes.data, z.ctypes.data, t.data_ptr(), None, None, t.data_ptr(), None, None, t.data_ptr(), None) == -2
