"""CPU restatement of the forced alignment ev_align runs (include/evhip.h), for tests/test_alignment.py and tests/test_gpu_align.py.

The aligner (reference modules/alignment.py:27-55) is restated in torch fp32 from the embed_projection1 output; the monotonic alignment
search (:93-122) with Q in fp64 and its first row summed SEQUENTIALLY in fp64 -- the one deliberate deviation of ev_align -- so that,
given the device's own log_p_attn, the durations it must return are determined bit for bit.  ``aligner_state_dict`` is the weight draw the
alignment fixtures use: synth_state_dict leaves the aligner's biases at zero (every other fixture depends on that dict staying as it
is), so a separate seeded draw gives them values.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

ALIGNER_BIAS_SEED = 4242
ALIGNER_BIAS_STD = 0.05
CONVS = ("t_conv1", "t_conv2", "f_conv1", "f_conv2", "f_conv3")


def aligner_state_dict(sd):
    """``sd`` (numpy state dict of synth_state_dict) with the aligner's five biases drawn from ALIGNER_BIAS_SEED (a new dict)."""
    out = dict(sd)
    rng = np.random.default_rng(ALIGNER_BIAS_SEED)
    for nm in CONVS:
        k = f"am.alignment_module.{nm}.bias"
        out[k] = (rng.standard_normal(np.asarray(sd[k]).shape) * ALIGNER_BIAS_STD).astype(np.float32)
    return out


def _t(x):
    return torch.as_tensor(np.asarray(x, np.float32))


def log_p_attn(sd, x_proj, mel):
    """alignment.py:27-55 for B = 1.  x_proj (N, H) the embed_projection1 output, mel (n_mels, T).  Returns (T, N) fp32 numpy."""
    from scipy.stats import betabinom
    w = lambda n: _t(sd[f"am.alignment_module.{n}.weight"])      # noqa: E731
    b = lambda n: _t(sd[f"am.alignment_module.{n}.bias"])        # noqa: E731
    with torch.no_grad():
        text = _t(x_proj).t().unsqueeze(0)
        text = F.conv1d(F.relu(F.conv1d(text, w("t_conv1"), b("t_conv1"), padding=1)), w("t_conv2"), b("t_conv2")).squeeze(0).t()
        f = _t(mel).unsqueeze(0)
        f = F.relu(F.conv1d(f, w("f_conv1"), b("f_conv1"), padding=1))
        f = F.relu(F.conv1d(f, w("f_conv2"), b("f_conv2"), padding=1))
        f = F.conv1d(f, w("f_conv3"), b("f_conv3")).squeeze(0).t()
        score = -torch.norm(f.unsqueeze(1) - text.unsqueeze(0), p=2, dim=2)
        lp = F.log_softmax(score, dim=-1)
    T, N = lp.shape
    alpha = np.arange(1, T + 1, dtype=float)
    prior = betabinom.logpmf(np.arange(N)[:, None], N, alpha, T - alpha + 1)       # (N, T)
    return (lp + torch.from_numpy(prior).t().to(torch.float32)).numpy()


def mas(lp):
    """alignment.py:93-122 with Q in fp64 and row 0 summed sequentially in fp64.  lp (T, N).  Returns A (T,) int64."""
    lp = np.asarray(lp, np.float32)
    T, N = lp.shape
    Q = np.full((N, T), -np.inf)
    lpt = lp.T.astype(np.float64)
    acc = 0.0
    for j in range(T):
        acc = acc + lpt[0, j]
        Q[0, j] = acc
    for j in range(1, T):
        for i in range(1, min(j + 1, N)):
            Q[i, j] = max(Q[i - 1, j - 1], Q[i, j - 1]) + lpt[i, j]
    A = np.full(T, N - 1, np.int64)
    for j in range(T - 2, -1, -1):
        ia, ib = A[j + 1] - 1, A[j + 1]
        if ib == 0:
            A[j] = 0
        elif Q[ia, j] >= Q[ib, j]:
            A[j] = ia
        else:
            A[j] = ib
    return A


def mas_fast(lp):
    """mas() vectorised over tokens (the same fp64 operations per cell, so the same path): for the large seeded batches."""
    lp = np.asarray(lp, np.float32)
    T, N = lp.shape
    lpt = lp.astype(np.float64)
    q = np.full(N, -np.inf)
    q[0] = lpt[0, 0]
    up = np.zeros((T, N), bool)
    for j in range(1, T):
        left = np.concatenate([[-np.inf], q[:-1]])
        u = left >= q
        up[j] = u
        nq = np.where(u, left, q) + lpt[j]
        nq[0] = q[0] + lpt[j, 0]
        nq[min(j + 1, N):] = -np.inf
        q = nq
    A = np.full(T, N - 1, np.int64)
    for j in range(T - 2, -1, -1):
        ib = A[j + 1]
        A[j] = ib - 1 if ib > 0 and up[j + 1, ib] else ib
    return A


def margins(lp, A):
    """|Q[i-1, j] - Q[i, j]| at every decision the backtrack makes on the path A (fp64): small values are near ties."""
    lp = np.asarray(lp, np.float32)
    T, N = lp.shape
    lpt = lp.T.astype(np.float64)
    Q = np.full((N, T), -np.inf)
    Q[0] = np.cumsum(lpt[0])
    for j in range(1, T):
        for i in range(1, min(j + 1, N)):
            Q[i, j] = max(Q[i - 1, j - 1], Q[i, j - 1]) + lpt[i, j]
    out = []
    for j in range(T - 2, -1, -1):
        ib = A[j + 1]
        if ib > 0 and np.isfinite(Q[ib, j]):
            out.append(abs(Q[ib - 1, j] - Q[ib, j]))
    return np.array(out)


def durations(A, N):
    return np.bincount(np.asarray(A), minlength=N).astype(np.int64)


def average_by_duration(d, xs):
    """alignment.py:145-162 for one utterance, as ev_align computes it: fp64 sum over the token's frames, one rounding to fp32."""
    d = np.asarray(d, np.int64)
    xs = np.asarray(xs, np.float32).astype(np.float64)
    ends = np.cumsum(d)
    out = np.zeros(d.size, np.float32)
    for n, (a, e) in enumerate(zip(ends - d, ends)):
        out[n] = np.float32(xs[a:e].sum() / (e - a)) if e > a else 0.0
    return out


def path_score(lp, A):
    """mean_t lp[t, A[t]] (= -bin_loss), fp64 sum."""
    lp = np.asarray(lp, np.float32)
    return np.float32(lp[np.arange(lp.shape[0]), A].astype(np.float64).sum() / lp.shape[0])
