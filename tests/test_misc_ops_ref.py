"""CPU check of the float64 references in tests/misc_ops_ref.py against the matching pieces of oracle/jets_oracle.py, oracle/bert_oracle.py and
tests/align_oracle.py on small inputs: they must agree to fp32 rounding.  test_oracle_golden.py ties the oracle to the reference's own outputs; this
ties the per-kernel references to the oracle, so a GPU failure in tests/test_gpu_misc_ops.py cannot be a mistake in the test's formula."""
import math

import numpy as np
import pytest

import misc_ops_ref as R

torch = pytest.importorskip("torch")
F = torch.nn.functional
TOL = 2e-6          # fp32 rounding of the oracle's own arithmetic (a few dozen ulp over a 384-term reduction)


def _rng(seed):
    return np.random.default_rng(seed)


def test_layernorm_matches_oracle():
    from oracle.jets_oracle import layer_norm
    x, g, b, _ = R.layernorm_inputs("gauss", 9, 384, 1)
    sd = {"n.weight": torch.from_numpy(g), "n.bias": torch.from_numpy(b)}
    assert R.worst_row_rel(layer_norm(torch.from_numpy(x), sd, "n").numpy(), R.layernorm(x, g, b, 1e-12)) < TOL


def test_attention_matches_oracle():
    from oracle.jets_oracle import self_attention
    C, H, n = 96, 2, 37
    x = _rng(2).standard_normal((n, C)).astype(np.float32)
    w = {k: (_rng(3 + i).standard_normal((C, C)) / math.sqrt(C)).astype(np.float32) for i, k in enumerate("qkv")}
    sd = {"a.linear_%s.weight" % k: torch.from_numpy(v) for k, v in w.items()}
    sd.update({"a.linear_%s.bias" % k: torch.zeros(C) for k in "qkv"})
    sd.update({"a.linear_out.weight": torch.eye(C), "a.linear_out.bias": torch.zeros(C)})
    qkv = np.concatenate([x @ w[k].T for k in "qkv"], axis=1).astype(np.float32)
    assert R.worst_row_rel(self_attention(torch.from_numpy(x), sd, "a", H).numpy(), R.attention(qkv, H)) < 1e-5
    for mode in (0, 1, 2):          # the CPU evaluations that set the bounds are the same operation
        q = qkv.astype(np.float16) if mode == 1 else qkv
        assert R.worst_row_rel(R.attention_f32(q, H, mode), R.attention(q, H)) < (2e-3 if mode == 1 else 1e-5)


def test_durations_and_centres_match_oracle():
    from oracle.jets_oracle import duration_from_log, gaussian_upsampling
    rng = _rng(4)
    for seed in (11, 21, 800 + 2048):          # the seeds the GPU tests draw from: no token within DUR_NEAR of a rounding boundary
        ld = R.draw_log_d(_rng(seed), 513)
        d, dist = R.durations(ld)
        assert (dist > R.DUR_NEAR).all()
        assert np.array_equal(duration_from_log(torch.from_numpy(ld)).numpy(), d)
    x = rng.standard_normal((len(d), 16)).astype(np.float32)
    for alpha in (1.0, 0.5, 1.3):
        up, T = gaussian_upsampling(torch.from_numpy(x), torch.from_numpy(d), alpha)
        cen, T64 = R.centres(d, alpha)
        assert T == T64
        c32 = R.centres_f32(d, alpha)                  # the oracle's own fp32 centres (its cumsum's rounding is amplified by exp(-0.1 (t - c)^2))
        assert np.abs(c32 / cen - 1).max() < 1e-6
        assert R.worst_row_rel(up.numpy(), R.gauss_upsample(x, c32, T, 0.1)) < 1e-5
    z = np.zeros(5, np.int64)
    assert R.centres(z, 1.0)[1] == 5 and gaussian_upsampling(torch.zeros(5, 4), torch.from_numpy(z))[1] == 5      # the all-zero guard


def test_gauss_windows_of_the_wide_case():
    for key, cid, utts in R.gauss_cases():
        if cid.endswith("wide"):
            assert {1, 4, 5} <= set(R.gauss_window_widths(utts[0][1], utts[0][2], 0.1).tolist())
        for x, c, T, ref, base in utts:
            assert R.worst_row_rel(base, ref) <= R.BASELINES[key] * 1.0000001


def test_var_embed_and_conv_post_match_oracle_ops():
    """am_forward's pitch / energy embedding (F.conv1d 1 -> C) and hifigan_forward's leaky_relu -> conv_post -> tanh, on the packed weight layouts"""
    for key, cid, (wp, bp, we, be), utts in R.var_embed_cases():
        k = wp.shape[0]
        for x, p, e, ref, base in utts:
            pe_ = F.conv1d(torch.from_numpy(p).view(1, 1, -1), torch.from_numpy(np.ascontiguousarray(wp.T[:, None, :])), torch.from_numpy(bp),
                           padding=(k - 1) // 2).squeeze(0).t()
            ee_ = F.conv1d(torch.from_numpy(e).view(1, 1, -1), torch.from_numpy(np.ascontiguousarray(we.T[:, None, :])), torch.from_numpy(be),
                           padding=(k - 1) // 2).squeeze(0).t()
            assert R.worst_row_rel((torch.from_numpy(x) + pe_ + ee_).numpy(), ref) < TOL
    rng = _rng(6)
    x = rng.standard_normal((300, 32)).astype(np.float32)
    w = (rng.standard_normal((7, 32)) * 0.1).astype(np.float32)
    y = torch.tanh(F.conv1d(F.leaky_relu(torch.from_numpy(x).t().unsqueeze(0)), torch.from_numpy(np.ascontiguousarray(w.T[None])), torch.tensor([0.05]), padding=3))
    assert R.max_abs(y.view(-1).numpy(), R.conv_post(x, w, 0.05, 0.01)) < 1e-5


def test_pe_and_wav_match_oracle():
    from oracle.jets_oracle import sinusoid_table, wav_to_int16
    div = R.pe_div(384)
    assert R.worst_row_rel(sinusoid_table(5000, 384).numpy()[4096:], R.pe_rows(4096, 5000, div)) < TOL
    w = np.concatenate([R.wav_edge_values(), _rng(7).uniform(-1, 1, 1000).astype(np.float32)])
    assert np.array_equal(wav_to_int16(w), R.wav_to_i16(w))


def test_fma32_is_the_correctly_rounded_fma():
    rng = _rng(8)
    a, b, c = (rng.standard_normal(2000).astype(np.float32) for _ in range(3))
    from fractions import Fraction
    got = R.fma32(a, b, c)
    for i in range(0, 2000, 37):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = [np.nextafter(got[i], np.float32(-np.inf)), got[i], np.nextafter(got[i], np.float32(np.inf))]
        assert min(near, key=lambda v: abs(Fraction(float(v)) - exact)) == got[i]


def test_bert_pooler_and_cond_vector_match_torch():
    for key, cid, inp, ref, base in R.dense_cases():
        assert R.worst_row_rel(base, ref) < TOL, cid
    # cond_vector is embed_projection1 on the time-constant columns (model_open_source.py:109-111): x-part + cond-part == the full Linear
    rng = _rng(9)
    C, bert = 64, 32
    W = rng.standard_normal((C, 2 * C + 2 * bert)).astype(np.float32)
    bias, x = rng.standard_normal(C).astype(np.float32), rng.standard_normal((5, C)).astype(np.float32)
    emb, st, co = rng.standard_normal((3, C)).astype(np.float32), rng.standard_normal((1, bert)).astype(np.float32), rng.standard_normal((1, bert)).astype(np.float32)
    cat = np.concatenate([x, np.repeat(emb[2:3], 5, 0), np.repeat(st, 5, 0), np.repeat(co, 5, 0)], axis=1)
    full = F.linear(torch.from_numpy(cat), torch.from_numpy(W), torch.from_numpy(bias)).numpy()
    u = R.cond_vector(np.array([2]), st, co, emb, np.ascontiguousarray(W[:, C:]), bias)
    assert R.worst_row_rel(x.astype(np.float64) @ W[:, :C].astype(np.float64).T + u, full) < 1e-5


def test_align_references_match_align_oracle():
    import align_oracle as AO
    rng = _rng(10)
    text, feats = rng.standard_normal((13, 32)).astype(np.float32), rng.standard_normal((40, 32)).astype(np.float32)
    ref = R.align_score(text, feats)
    assert R.worst_row_rel(R.align_score_f32(text, feats), ref) < TOL
    # align_oracle.log_p_attn's tail (score -> log_softmax -> + prior) on the same features
    from scipy.stats import betabinom
    f, x = torch.from_numpy(feats), torch.from_numpy(text)
    lp = F.log_softmax(-torch.norm(f.unsqueeze(1) - x.unsqueeze(0), p=2, dim=2), dim=-1)
    a = np.arange(1, 41, dtype=float)
    want = (lp + torch.from_numpy(betabinom.logpmf(np.arange(13)[:, None], 13, a, 40 - a + 1)).t().to(torch.float32)).numpy()
    assert R.worst_row_rel(want, ref) < TOL
    for quant in (False, True):
        lpq = (-rng.integers(0, 129, (40, 13)) / 8.0).astype(np.float32) if quant else ref.astype(np.float32)
        A = AO.mas(lpq)
        assert np.array_equal(A, AO.mas_fast(lpq))
        tr = rng.standard_normal(40).astype(np.float32)
        d, s, (m,) = R.mas_outputs(lpq, A, (tr,))
        assert np.array_equal(d, AO.durations(A, 13)) and s == AO.path_score(lpq, A) and np.array_equal(m, AO.average_by_duration(d, tr))


def test_baselines_are_current_for_the_cheap_cases():
    """BASELINES is a pasted table: recompute the cheap entries so it cannot drift from the generators"""
    got = {}
    for key, _, _, ref, base in R.dense_cases():
        got[key] = max(got.get(key, 0.0), R.worst_row_rel(base, ref))
    for key, _, _, ref, base in R.conv_post_cases("f32k7"):
        got[key] = max(got.get(key, 0.0), R.max_abs(base, ref))
    for key, _, (x, g, b, w), ref, base in R.layernorm_cases(Cs=(128, 768), rows_list=(1, 3)):
        assert R.worst_row_rel(base, ref) <= R.BASELINES[key] * 1.0000001
    for k, v in got.items():
        assert abs(v - R.BASELINES[k]) <= 1e-3 * R.BASELINES[k], (k, v, R.BASELINES[k])
