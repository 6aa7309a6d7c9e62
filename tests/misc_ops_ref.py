"""Float64 references of the non-GEMM kernels (ev_misc.hip, ev_align.hip), written from each operation's definition, plus the plain fp32
CPU evaluation of the same operation that sets each tolerance.  Used by tests/test_gpu_misc_ops.py and tests/test_gpu_ops.py (the device
against the float64 reference) and by tests/test_misc_ops_ref.py (the float64 reference against oracle/ and tests/align_oracle.py, no GPU).

Tolerances: BOUND = 4 x the worst-row error of the fp32 CPU evaluation (BASELINES below) against the float64 reference on the same
inputs, floored at 4 fp32 ulp of the row norm.  ``python tests/misc_ops_ref.py`` recomputes BASELINES; nothing in it comes from a kernel.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F32_EPS = float(np.finfo(np.float32).eps)      # 2^-23
FLOOR = 4 * F32_EPS                            # 4 fp32 ulp of the row norm (relative)


# --------------------------------------------------------------------------- measures
def worst_row_rel(got, ref):
    """max over rows of ||got - ref|| / ||ref|| (rows with ref == 0 must be exactly 0 and count as 0)."""
    got = np.asarray(got, np.float64).reshape(len(ref), -1)
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    num = np.linalg.norm(got - ref, axis=1)
    den = np.linalg.norm(ref, axis=1)
    assert not num[den == 0].any(), "non-zero output where the reference row is exactly zero"
    return float(np.max(np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0))) if len(ref) else 0.0


def max_abs(got, ref):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float(d.max()) if d.size else 0.0


def bound(baseline):
    return max(4.0 * baseline, FLOOR)


def fma32(a, b, c):
    """Correctly rounded fp32 fma(a, b, c) of fp32 arrays: the float64 product is exact, the float64 sum is rounded once; the few results
    that land exactly on an fp32 rounding boundary in float64 (where a second rounding could differ) are redone in rationals."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = s.astype(np.float32)
    tie = np.isfinite(s) & ((s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28))
    for i in zip(*np.nonzero(tie)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        if exact == Fraction(float(s[i])):            # a true tie: the single rounding above already went to even
            continue
        lo, hi = np.nextafter(out[i], np.float32(-np.inf)), np.nextafter(out[i], np.float32(np.inf))
        out[i] = min((lo, out[i], hi), key=lambda v: abs(Fraction(float(v)) - exact))
    return out


# --------------------------------------------------------------------------- LayerNorm (modules/encoder.py:112-127)
def layernorm(x, gamma, beta, eps):
    x = np.asarray(x, np.float32).astype(np.float64)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    return (x - mu) / np.sqrt(var + float(np.float32(eps))) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def layernorm_f32(x, gamma, beta, eps):
    import torch
    return torch.nn.functional.layer_norm(torch.from_numpy(np.asarray(x, np.float32)), (x.shape[1],), torch.from_numpy(gamma), torch.from_numpy(beta),
                                          eps).numpy()


def layernorm_inputs(family, rows, C, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, C))
    if family == "mean1e3":
        x = x + 1e3
    elif family == "nearconst":
        x = 0.7 + 1e-6 * x
    elif family == "outlier":
        x[:, C // 3] = 1e4
    g = (rng.standard_normal(C) * 0.5 + 1.0).astype(np.float32)
    b = (rng.standard_normal(C) * 0.2).astype(np.float32)
    w = rng.standard_normal(C).astype(np.float32)
    return x.astype(np.float32), g, b, w


LN_FAMILIES = ("gauss", "mean1e3", "nearconst", "outlier")
LN_CS = (128, 256, 384, 512, 640, 768, 1024)
LN_ROWS = (1, 2, 3, 5, 300)


# --------------------------------------------------------------------------- attention (modules/encoder.py:72-109, one utterance)
def attention(qkv, heads):
    """qkv (n, 3 C) -> softmax(q k^T / sqrt(d_k)) v per head, (n, C), float64."""
    qkv = np.asarray(qkv).astype(np.float64)
    n, C = qkv.shape[0], qkv.shape[1] // 3
    dk = C // heads
    q, k, v = (qkv[:, i * C:(i + 1) * C].reshape(n, heads, dk).transpose(1, 0, 2) for i in range(3))
    s = q @ k.transpose(0, 2, 1) / math.sqrt(dk)
    s -= s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return (p @ v).transpose(1, 0, 2).reshape(n, C)


def split_f16(x):
    """the split-precision operand the kernel forms: hi = fp16(x), lo = fp16((x - hi) * 2048); the value it multiplies is hi + lo / 2048"""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16).astype(np.float32)
    lo = ((x - hi) * np.float32(2048)).astype(np.float16).astype(np.float32)
    return hi + lo / np.float32(2048)


def attention_f32(qkv, heads, mode):
    """The plain fp32 torch evaluation.  mode 0: fp32 operands.  mode 1 (fp16 rows): fp32 math on the fp16 operands with the probabilities
    (exp(s - max), before normalisation) rounded to fp16 where the kernel packs them for the P.V product.  mode 2 (split precision): the
    operands q / sqrt(d_k) . log2 e, k, v replaced by their hi + lo / 2048 fp16 pairs, the kernel's stated operand rounding."""
    import torch
    t = torch.from_numpy(np.asarray(qkv).astype(np.float32))
    n, C = t.shape[0], t.shape[1] // 3
    dk = C // heads
    q, k, v = (t[:, i * C:(i + 1) * C].reshape(n, heads, dk).transpose(0, 1) for i in range(3))
    if mode == 2:
        sc = np.float32(1.4426950408889634) / np.sqrt(np.float32(dk))
        q = torch.from_numpy(split_f16(q.numpy() * sc)) * float(np.float32(math.log(2.0)))
        k, v = torch.from_numpy(split_f16(k.numpy())), torch.from_numpy(split_f16(v.numpy()))
        s = q @ k.transpose(1, 2)
    else:
        s = q @ k.transpose(1, 2) / math.sqrt(dk)
    if mode == 1:
        p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        o = (p.half().float() @ v) / p.sum(dim=-1, keepdim=True)
    else:
        o = torch.softmax(s, dim=-1) @ v
    return o.transpose(0, 1).reshape(n, C).numpy()


ATT_LENS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
ATT_FAMILIES = ("gauss", "peaked", "ascending", "constant", "bigv")


def attention_inputs(family, n, C, heads, seed):
    """(n, 3 C) fp32 q | k | v.  peaked: logits span +-60 (one key dominates, the others underflow); ascending: key j's logit grows with j
    (every tile rescales); constant: all logits equal (the result is the mean of v); bigv: |v| ~ 1e4 under a peaked softmax."""
    rng = np.random.default_rng(seed)
    dk = C // heads
    x = rng.standard_normal((n, 3 * C))
    if family in ("peaked", "bigv"):
        x[:, :2 * C] *= math.sqrt(60.0 / 3.0) / dk ** 0.25           # logit std ~ 20, extremes ~ +-60
        if family == "bigv":
            x[:, 2 * C:] *= 1e4
    elif family == "ascending":
        x[:, :C] = 1.0 + 0.01 * x[:, :C]
        x[:, C:2 * C] = (np.arange(n)[:, None] * (40.0 / max(n - 1, 1)) / math.sqrt(dk)) + 0.01 * x[:, C:2 * C]
    elif family == "constant":
        x[:, :C] = 0.5
        x[:, C:2 * C] = 0.25
    return x.astype(np.float32)


# --------------------------------------------------------------------------- durations (variance.py:47-51, alignment.py:183-202)
DUR_NEAR = 2e-4


def durations(log_d):
    """d = clamp(round(exp(x) - 1), 0) in float64 (round half to even), and the distance of exp(x) - 1 from the nearest rounding boundary"""
    v = np.exp(np.asarray(log_d, np.float32).astype(np.float64)) - 1.0
    return np.maximum(np.rint(v), 0).astype(np.int64), np.abs(v - np.floor(v) - 0.5)


def draw_log_d(rng, n, zero_frac=0.2):
    """log-durations whose exp(x) - 1 stays DUR_NEAR away from every half-integer: an ulp of expf cannot flip rint"""
    out = np.empty(n, np.float32)
    i = 0
    while i < n:
        x = np.float32(rng.uniform(-1.5, 3.2))
        if rng.uniform() < zero_frac:
            x = np.float32(rng.uniform(-3.0, 0.3))
        if durations(np.array([x]))[1][0] > DUR_NEAR:
            out[i] = x
            i += 1
    return out


def centres(d_eff, alpha):
    """alignment.py:202 c = cumsum(ds alpha) - ds alpha / 2 in float64, with ds alpha the fp32 product the reference forms; mel_len = int(sum)"""
    ds = (np.asarray(d_eff, np.float32) * np.float32(alpha)).astype(np.float64)
    if ds.sum() == 0:
        ds = np.ones_like(ds)
    return np.cumsum(ds) - ds / 2, int(ds.sum())


def centres_f32(d_eff, alpha):
    import torch
    ds = torch.from_numpy(np.asarray(d_eff, np.float32)) * float(alpha)
    if ds.sum() == 0:
        ds = torch.ones_like(ds)
    return (ds.cumsum(0) - ds / 2).numpy()


# --------------------------------------------------------------------------- Gaussian upsampling (alignment.py:204-210)
def gauss_upsample(x, c, T, delta):
    x = np.asarray(x, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    out = np.empty((T, x.shape[1]))
    for t0 in range(0, T, 1024):
        t = np.arange(t0, min(t0 + 1024, T), dtype=np.float64)[:, None]
        e = -float(np.float32(delta)) * (t - c[None, :]) ** 2
        p = np.exp(e - e.max(axis=1, keepdims=True))
        out[t0:t0 + len(t)] = (p / p.sum(axis=1, keepdims=True)) @ x
    return out


def gauss_upsample_f32(x, c, T, delta):
    import torch
    x, c = torch.from_numpy(np.asarray(x, np.float32)), torch.from_numpy(np.asarray(c, np.float32))
    out = []
    for t0 in range(0, T, 1024):
        t = torch.arange(t0, min(t0 + 1024, T)).float()
        out.append(torch.softmax(-1 * delta * (t.unsqueeze(-1) - c.unsqueeze(0)) ** 2, dim=1) @ x)
    return torch.cat(out).numpy()


def gauss_window_widths(c, T, delta):
    """per frame, how many tokens have a non-zero fp32 weight exp(e - max): the kernel's window [jlo, jhi] (its 4-row unroll has a tail)"""
    c = np.asarray(c, np.float32)
    t = np.arange(T, dtype=np.float32)[:, None]
    e = -np.float32(delta) * (t - c[None, :]) ** 2
    return (np.exp((e - e.max(axis=1, keepdims=True)).astype(np.float64)).astype(np.float32) > 0).sum(axis=1)


# --------------------------------------------------------------------------- pitch / energy embedding add (model_open_source.py:131-134)
def var_embed_add(x, pitch, energy, wp, bp, we, be):
    """One utterance.  x (n, C); pitch / energy (n,); wp / we (k, C).  Conv1d(1 -> C, k, zero pad (k-1)/2)."""
    n, k = x.shape[0], wp.shape[0]
    h = (k - 1) // 2
    pp = np.pad(np.asarray(pitch, np.float64), h)
    ee = np.pad(np.asarray(energy, np.float64), h)
    out = x.astype(np.float64) + bp.astype(np.float64) + be.astype(np.float64)
    for t in range(k):
        out += pp[t:t + n, None] * wp[t].astype(np.float64) + ee[t:t + n, None] * we[t].astype(np.float64)
    return out


def var_embed_add_f32(x, pitch, energy, wp, bp, we, be):
    import torch
    Fn = torch.nn.functional
    k = wp.shape[0]
    conv = lambda s, w, b: Fn.conv1d(torch.from_numpy(s).view(1, 1, -1), torch.from_numpy(np.ascontiguousarray(w.T[:, None, :])), torch.from_numpy(b),  # noqa: E731
                                     padding=(k - 1) // 2).squeeze(0).t()
    return (torch.from_numpy(x) + conv(pitch, wp, bp) + conv(energy, we, be)).numpy()


# --------------------------------------------------------------------------- conv_post + tanh (models/hifigan/models.py:127-129)
def conv_post(x, w, bias, pre_slope=None):
    """x (n, C) (already rounded to the kernel's operand type), w (k, C) -> tanh(conv) (n,).  pre_slope: leaky_relu applied to x first (fp32 input)."""
    x = np.asarray(x).astype(np.float64)
    if pre_slope is not None:
        x = np.where(x >= 0, x, x * float(np.float32(pre_slope)))
    k = w.shape[0]
    h = (k - 1) // 2
    xp = np.pad(x, ((h, h), (0, 0)))
    a = np.full(x.shape[0], float(np.float32(bias)))
    for t in range(k):
        a += xp[t:t + x.shape[0]] @ w[t].astype(np.float64)
    return np.tanh(a)


def conv_post_f32(x, w, bias, pre_slope=None):
    import torch
    Fn = torch.nn.functional
    t = torch.from_numpy(np.asarray(x).astype(np.float32))
    if pre_slope is not None:
        t = Fn.leaky_relu(t, float(np.float32(pre_slope)))
    k = w.shape[0]
    y = Fn.conv1d(t.t().unsqueeze(0), torch.from_numpy(np.ascontiguousarray(w.T[None])), torch.tensor([bias], dtype=torch.float32), padding=(k - 1) // 2)
    return torch.tanh(y).view(-1).numpy()


# --------------------------------------------------------------------------- small dense ops
def cond_vector(speaker, style, content, spk_emb, W, bias):
    """model_open_source.py:109-111: the time-constant part of embed_projection1.  W (C, C + 2 bert)."""
    s = np.clip(np.asarray(speaker), 0, spk_emb.shape[0] - 1)
    cat = np.concatenate([spk_emb[s], style, content], axis=1).astype(np.float64)
    return cat @ W.astype(np.float64).T + bias.astype(np.float64)


def cond_vector_f32(speaker, style, content, spk_emb, W, bias):
    import torch
    s = np.clip(np.asarray(speaker), 0, spk_emb.shape[0] - 1)
    cat = torch.from_numpy(np.concatenate([spk_emb[s], style, content], axis=1))
    return torch.nn.functional.linear(cat, torch.from_numpy(W), torch.from_numpy(bias)).numpy()


def bert_pooler(h0, W, bias):
    """transformers BertPooler: tanh(W h[first token] + b)"""
    return np.tanh(h0.astype(np.float64) @ W.astype(np.float64).T + bias.astype(np.float64))


def bert_pooler_f32(h0, W, bias):
    import torch
    return torch.tanh(torch.nn.functional.linear(torch.from_numpy(h0), torch.from_numpy(W), torch.from_numpy(bias))).numpy()


def pe_div(C):
    """encoder.py:216-237: div[i] = exp(2 i * -(ln 1e4 / d)) as the reference forms it (fp32)"""
    import torch
    return torch.exp(torch.arange(0, C, 2, dtype=torch.float32) * -(math.log(10000.0) / C)).numpy()


def pe_rows(row0, row1, div):
    """sin / cos in float64 of the fp32-ROUNDED angle float32(t) * div[i]"""
    ang = (np.arange(row0, row1, dtype=np.float32)[:, None] * div[None, :].astype(np.float32)).astype(np.float64)
    out = np.empty((row1 - row0, 2 * len(div)))
    out[:, 0::2], out[:, 1::2] = np.sin(ang), np.cos(ang)
    return out


def pe_rows_f32(row0, row1, div):
    import torch
    ang = torch.arange(row0, row1, dtype=torch.float32).unsqueeze(1) * torch.from_numpy(div)
    out = torch.zeros(row1 - row0, 2 * len(div))
    out[:, 0::2], out[:, 1::2] = torch.sin(ang), torch.cos(ang)
    return out.numpy()


def wav_to_i16(w):
    """(x * 32768.0).astype(int16) as a C cast: the product by 2^15 is exact, truncation toward zero, wrap-around"""
    return np.trunc(np.asarray(w, np.float32).astype(np.float64) * 32768.0).astype(np.int64).astype(np.int16)


def wav_edge_values():
    one = np.float32(1.0)
    below = np.nextafter(one, np.float32(0))                       # 1 - 2^-24
    vals = [one, -one, below, -below, np.float32(2.0 ** -16), np.float32(-2.0 ** -16), np.float32(0.0), np.float32(-0.0)]
    for k in (1, 7, 100, 32767, -1, -7, -100, -32767, -32768):     # products just below / at / just above an integer
        e = np.float32(k / 32768.0)
        vals += [e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(2 * np.sign(k)))]
    return np.array(vals, np.float32)


# --------------------------------------------------------------------------- aligner score (alignment.py:27-55)
def align_score(text, feats):
    """text (N, C), feats (T, C) fp32 -> (T, N) float64: log_softmax_n(-||f_t - x_n||) + log betabinom.pmf(n; N, t + 1, T - t)"""
    from scipy.stats import betabinom
    x, f = np.asarray(text, np.float32).astype(np.float64), np.asarray(feats, np.float32).astype(np.float64)
    T, N = f.shape[0], x.shape[0]
    s = np.empty((T, N))
    for t0 in range(0, T, 256):
        s[t0:t0 + 256] = -np.sqrt(((f[t0:t0 + 256, None, :] - x[None, :, :]) ** 2).sum(-1))
    m = s.max(axis=1, keepdims=True)
    lp = s - (m + np.log(np.exp(s - m).sum(axis=1, keepdims=True)))
    a = np.arange(1, T + 1, dtype=np.float64)
    return lp + betabinom.logpmf(np.arange(N)[:, None], N, a, T - a + 1).T


def align_score_f32(text, feats):
    import torch
    from scipy.stats import betabinom
    x, f = torch.from_numpy(np.asarray(text, np.float32)), torch.from_numpy(np.asarray(feats, np.float32))
    T, N = f.shape[0], x.shape[0]
    lp = torch.cat([torch.log_softmax(-torch.norm(f[t0:t0 + 256].unsqueeze(1) - x.unsqueeze(0), p=2, dim=2), dim=-1) for t0 in range(0, T, 256)])
    a = np.arange(1, T + 1, dtype=float)
    return (lp + torch.from_numpy(betabinom.logpmf(np.arange(N)[:, None], N, a, T - a + 1)).t().to(torch.float32)).numpy()


def mas_outputs(lp, A, tracks=()):
    """durations (bincount of the path), the mean log_p along it (fp64 sum, one rounding) and the per-token fp64 means of the frame tracks"""
    lp = np.asarray(lp, np.float32)
    T, N = lp.shape
    d = np.bincount(np.asarray(A), minlength=N).astype(np.int64)
    score = np.float32(lp[np.arange(T), A].astype(np.float64).sum() / T)
    ends = np.cumsum(d)
    means = []
    for tr in tracks:
        tr = np.asarray(tr, np.float32).astype(np.float64)
        means.append(np.array([np.float32(tr[a:e].sum() / (e - a)) for a, e in zip(ends - d, ends)], np.float32))
    return d, score, means


# --------------------------------------------------------------------------- the floating-point cases (inputs, float64 reference, fp32 CPU evaluation)
# Every generator yields (baseline key, case id, inputs, float64 reference, fp32 CPU result); the GPU tests walk the same generators, so a
# kernel is measured on exactly the inputs its baseline was measured on.
def _h(x):
    return np.asarray(x, np.float32).astype(np.float16)


def layernorm_cases(Cs=LN_CS, rows_list=LN_ROWS):
    for fam in LN_FAMILIES:
        for C in Cs:
            for rows in rows_list:
                x, g, b, w = layernorm_inputs(fam, rows, C, 1000 + C + rows)
                yield "layernorm/" + fam, "%s-C%d-r%d" % (fam, C, rows), (x, g, b, w), layernorm(x, g, b, 1e-12), layernorm_f32(x, g, b, 1e-12)


ATT_MODES = {"f32_dk48": (0, 384, 8), "f32_dk64": (0, 768, 12), "f16_dk48": (1, 384, 8), "x3_dk48": (2, 384, 8)}


def attention_cases(mode_name, lens=ATT_LENS, families=ATT_FAMILIES):
    mode, C, heads = ATT_MODES[mode_name]
    for fam in families:
        for n in lens:
            qkv = attention_inputs(fam, n, C, heads, 7000 + n)
            if mode == 1:
                qkv = np.clip(qkv, -6e4, 6e4).astype(np.float16)
            base = attention_f32(qkv, heads, mode)
            if mode == 1:
                base = _h(base)
            yield "attention/%s/%s" % (mode_name, fam), "%s-%s-n%d" % (mode_name, fam, n), qkv, attention(qkv, heads), base


GAUSS_CASES = (  # (C, token counts per utterance, kind of durations)
    (128, (1, 2, 63), "mixed"), (384, (64, 65, 400), "mixed"), (512, (5, 1), "mixed"), (384, (2048,), "short"), (128, (300,), "long16k"),
    (384, (24,), "wide"))


def gauss_durations(kind, n, rng):
    if kind == "short":                      # 2048 tokens, 8 frames each = 16384 frames
        return np.full(n, 8, np.int64)
    if kind == "long16k":                    # runs of zeros (coincident centres) and one very long token, 16384 frames in all
        d = rng.integers(0, 12, n)
        d[rng.uniform(size=n) < 0.3] = 0
        d[10:14] = 0
        d[n // 2] = 0
        d[n // 2] = 16384 - d.sum()
        return d.astype(np.int64)
    if kind == "wide":                       # long tokens: windows [jlo, jhi] of 1 .. 5 tokens (delta = 0.1: exp underflows beyond ~32 frames)
        return np.array([80, 1, 1, 1, 60, 30, 30, 30, 30, 70, 20, 20, 20, 20, 20, 90] + [3] * (n - 16), np.int64)
    d = rng.integers(0, 9, n)
    if n > 4:
        d[1:3] = 0
    if d.sum() == 0:
        d[0] = 3
    return d.astype(np.int64)


def gauss_cases():
    for C, toks, kind in GAUSS_CASES:
        rng = np.random.default_rng(9000 + C + sum(toks))
        utts = []
        for n in toks:
            d = gauss_durations(kind, n, rng)
            c = centres_f32(d, 1.0)
            x = rng.standard_normal((n, C)).astype(np.float32)
            T = int(d.sum())
            utts.append((x, c, T, gauss_upsample(x, c, T, 0.1), gauss_upsample_f32(x, c, T, 0.1)))
        yield "gauss_upsample", "C%d-%s-%s" % (C, "_".join(map(str, toks)), kind), utts


def var_embed_cases():
    for k in (1, 3, 9):
        for C in (128, 384):
            rng = np.random.default_rng(300 + 10 * k + C)
            wp, we = (rng.standard_normal((k, C)).astype(np.float32) for _ in range(2))
            bp, be = (rng.standard_normal(C).astype(np.float32) for _ in range(2))
            utts = []
            for n in sorted({1, 2, max(k - 1, 1), k, 37}):
                x = rng.standard_normal((n, C)).astype(np.float32)
                p, e = (rng.standard_normal(n).astype(np.float32) * 2 for _ in range(2))
                utts.append((x, p, e, var_embed_add(x, p, e, wp, bp, we, be), var_embed_add_f32(x, p, e, wp, bp, we, be)))
            yield "var_embed_add", "k%d-C%d" % (k, C), (wp, bp, we, be), utts


CONV_POST_KINDS = {"f16": (False, (7, 3)), "f32k7": (True, (7,)), "f32gen": (True, (3, 5, 9, 15))}


def conv_post_cases(kind):
    is_f32, ks = CONV_POST_KINDS[kind]
    for k in ks:
        for rows in (1, 255, 256, 257, 1000):
            for slope in ((1.0, 0.01, 0.0) if is_f32 else (None,)):
                rng = np.random.default_rng(500 + k + rows)
                x = rng.standard_normal((rows, 32)).astype(np.float32)
                x[::5] *= 40.0                                    # rows whose pre-activation is large enough for tanh to saturate to +-1
                x = x if is_f32 else x.astype(np.float16)
                w = (rng.standard_normal((k, 32)) * 0.1).astype(np.float32)
                yield ("conv_post/" + kind, "%s-k%d-r%d-s%s" % (kind, k, rows, slope), (x, w, 0.05, slope), conv_post(x, w, 0.05, slope),
                       conv_post_f32(x, w, 0.05, slope))


def dense_cases():
    for C in (384, 768):
        for B in (1, 5):
            rng = np.random.default_rng(40 + C + B)
            bert, nspk = 768, 11
            spk = np.array(([0, nspk - 1, 3, 10, 0])[:B], np.int64)
            style, content = (rng.standard_normal((B, bert)).astype(np.float32) for _ in range(2))
            emb = rng.standard_normal((nspk, C)).astype(np.float32)
            W = (rng.standard_normal((C, C + 2 * bert)) / math.sqrt(C + 2 * bert)).astype(np.float32)
            bias = rng.standard_normal(C).astype(np.float32)
            yield ("cond_vector", "C%d-B%d" % (C, B), (spk, style, content, emb, W, bias), cond_vector(spk, style, content, emb, W, bias),
                   cond_vector_f32(spk, style, content, emb, W, bias))
            h0 = rng.standard_normal((B, C)).astype(np.float32)
            Wp = (rng.standard_normal((C, C)) / math.sqrt(C) * 1.5).astype(np.float32)
            yield "bert_pooler", "C%d-B%d" % (C, B), (h0, Wp, bias), bert_pooler(h0, Wp, bias), bert_pooler_f32(h0, Wp, bias)


ALIGN_SHAPES = ((32, 1, 1), (384, 64, 64), (32, 65, 63), (384, 129, 65), (32, 1536, 256), (32, 4096, 1024))     # (C, T, N)


def align_score_cases(shapes=ALIGN_SHAPES):
    for C, T, N in shapes:
        rng = np.random.default_rng(60 + T + N)
        text = rng.standard_normal((N, C)).astype(np.float32)
        feats = (text[np.minimum(np.arange(T) * N // T, N - 1)] + 0.5 * rng.standard_normal((T, C))).astype(np.float32)
        yield "align_score", "C%d-T%d-N%d" % (C, T, N), (text, feats), align_score(text, feats), align_score_f32(text, feats)
    rng = np.random.default_rng(61)
    text = rng.standard_normal((65, 32)).astype(np.float32)
    feats = rng.standard_normal((129, 32)).astype(np.float32)
    feats[5] = text[3]                                   # distance exactly 0
    yield "align_score", "exact-hit", (text, feats), align_score(text, feats), align_score_f32(text, feats)
    text = (rng.standard_normal((130, 32)) * 40).astype(np.float32)        # every distance large: only the maximum survives the online sum
    feats = (rng.standard_normal((70, 32)) * 40).astype(np.float32)
    yield "align_score", "all-far", (text, feats), align_score(text, feats), align_score_f32(text, feats)


def alpha_centre_cases():
    """the float-alpha branch of the durations kernel: centres against the float64 cumsum of the fp32 products d * alpha"""
    for n in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2048):
        for alpha in (0.5, 1.3):
            rng = np.random.default_rng(800 + n)
            d = durations(draw_log_d(rng, n))[0]
            yield "durations_alpha_centres", "n%d-a%s" % (n, alpha), (d, alpha), centres(d, alpha)[0], centres_f32(d, alpha)


def pe_cases():
    div = pe_div(384)
    for r0, r1 in ((4096, 8192), (8192, 16384)):
        yield "pe_extend", "rows%d-%d" % (r0, r1), (r0, r1, div), pe_rows(r0, r1, div), pe_rows_f32(r0, r1, div)


# --------------------------------------------------------------------------- fp32 baselines (worst-row relative error of the plain fp32 CPU op)
# Filled by ``python tests/misc_ops_ref.py`` on the CPU: worst-row ||fp32 torch op - float64 reference|| / ||reference|| on the inputs of the named
# case, maximised over the case's shapes.  The device bound of a case is bound(BASELINES[case]).
BASELINES = {
    "align_score": 2.170e-07,
    "align_score/maxabs": 2.397e-04,
    "attention/f16_dk48/ascending": 3.260e-04,
    "attention/f16_dk48/bigv": 2.864e-04,
    "attention/f16_dk48/constant": 2.263e-04,
    "attention/f16_dk48/gauss": 3.249e-04,
    "attention/f16_dk48/peaked": 3.044e-04,
    "attention/f32_dk48/ascending": 5.447e-06,
    "attention/f32_dk48/bigv": 2.178e-06,
    "attention/f32_dk48/constant": 3.358e-07,
    "attention/f32_dk48/gauss": 9.761e-07,
    "attention/f32_dk48/peaked": 2.113e-06,
    "attention/f32_dk64/ascending": 6.290e-06,
    "attention/f32_dk64/bigv": 1.718e-06,
    "attention/f32_dk64/constant": 3.421e-07,
    "attention/f32_dk64/gauss": 8.233e-07,
    "attention/f32_dk64/peaked": 1.679e-06,
    "attention/x3_dk48/ascending": 5.375e-06,
    "attention/x3_dk48/bigv": 1.563e-06,
    "attention/x3_dk48/constant": 3.290e-07,
    "attention/x3_dk48/gauss": 6.858e-07,
    "attention/x3_dk48/peaked": 1.624e-06,
    "bert_pooler": 2.637e-07,
    "cond_vector": 2.475e-07,
    "conv_post/f16": 8.589e-06,
    "conv_post/f32gen": 1.842e-05,
    "conv_post/f32k7": 7.663e-06,
    "durations_alpha_centres": 1.026e-07,
    "gauss_upsample": 2.298e-07,
    "layernorm/gauss": 1.509e-07,
    "layernorm/gauss/dot": 3.612e-08,
    "layernorm/gauss/f16": 2.744e-04,
    "layernorm/mean1e3": 1.159e-04,
    "layernorm/mean1e3/dot": 1.965e-05,
    "layernorm/mean1e3/f16": 2.740e-04,
    "layernorm/nearconst": 1.027e-01,
    "layernorm/nearconst/dot": 1.473e-02,
    "layernorm/nearconst/f16": 1.027e-01,
    "layernorm/outlier": 2.685e-07,
    "layernorm/outlier/dot": 5.911e-08,
    "layernorm/outlier/f16": 4.008e-04,
    "pe_extend": 2.405e-08,
    "var_embed_add": 8.546e-08,
}


def compute_baselines():
    out = {}

    def put(key, v):
        out[key] = max(out.get(key, 0.0), v)
    for key, _, (x, g, b, w), ref, base in layernorm_cases():
        put(key, worst_row_rel(base, ref))
        put(key + "/f16", worst_row_rel(_h(base), ref))
        put(key + "/dot", dot_err(base @ w, ref, w))
    for mode in ATT_MODES:
        for key, _, _, ref, base in attention_cases(mode):
            put(key, worst_row_rel(base, ref))
    for key, _, utts in gauss_cases():
        for _, _, _, ref, base in utts:
            put(key, worst_row_rel(base, ref))
    for key, _, _, utts in var_embed_cases():
        for _, _, _, ref, base in utts:
            put(key, worst_row_rel(base, ref))
    for kind in CONV_POST_KINDS:
        for key, _, _, ref, base in conv_post_cases(kind):
            put(key, max_abs(base, ref))                 # scalar per row: max-abs (|tanh| <= 1)
    for key, _, _, ref, base in dense_cases():
        put(key, worst_row_rel(base, ref))
    for key, _, _, ref, base in align_score_cases():
        put(key, worst_row_rel(base, ref))
        put(key + "/maxabs", max_abs(base, ref))
    for key, _, _, ref, base in alpha_centre_cases():
        put(key, max_abs(base / np.maximum(ref, 1.0), ref / np.maximum(ref, 1.0)))       # scalar per token: error relative to the centre itself
    for key, _, _, ref, base in pe_cases():
        put(key, worst_row_rel(base, ref))
    return out


def dot_err(got, ref_y, w):
    """the fused Linear(C, 1) head: |got - <y, w>| / (||y|| ||w||), maximised over rows"""
    ref = ref_y @ w.astype(np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / (np.linalg.norm(ref_y, axis=1) * np.linalg.norm(w.astype(np.float64)))))


if __name__ == "__main__":
    for k_, v_ in sorted(compute_baselines().items()):
        print('    "%s": %.3e,' % (k_, v_))
