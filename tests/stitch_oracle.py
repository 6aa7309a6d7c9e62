"""numpy oracle of ev_stitch's specification (include/evhip.h): the cut, the int64 plan, the ramp and the mix with explicit float32 products and
sums in the specified order, and the clamped int16 conversion.  The ramp table is an argument, so a bit-exact comparison uses the table the device
holds."""
import numpy as np

MAX_FADE = 4096


def ramp_table(F):
    """tab[i] = (float)(0.5 - 0.5 cos(pi (i + 0.5) / F)) in float64, rounded once."""
    i = np.arange(F, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / max(F, 1))).astype(np.float32)


def scan(x, trim_frac, trim_abs):
    """(peak float32, first, last): max |x| and the first / last index with |x| > max(peak * trim_frac as one float32 product, trim_abs);
    -1, -1 where there is none."""
    ax = np.abs(np.asarray(x, np.float32))
    peak = np.float32(ax.max())
    thr = max(np.float32(peak * np.float32(trim_frac)), np.float32(trim_abs))
    hit = np.nonzero(ax > thr)[0]
    if hit.size == 0:
        return peak, -1, -1
    return peak, int(hit[0]), int(hit[-1])


def cut(x, trim_frac, trim_abs, keep):
    """(a, b, peak): the kept range x[a .. b); no trim at all (both thresholds zero): the whole segment and peak 0, as no scan runs."""
    L = len(x)
    if trim_frac == 0 and trim_abs == 0:
        return 0, L, np.float32(0.0)
    peak, first, last = scan(x, trim_frac, trim_abs)
    if first < 0:
        return 0, 0, peak
    return max(0, first - keep), min(L, last + 1 + keep), peak


def plan(n, seg_doc, pause_after, F, lead=0, tail=0):
    """int64 plan of the cut lengths n: (pos, fl, fr, doc_lens)."""
    n = [int(v) for v in n]
    S = len(n)
    F = int(F)
    D = int(seg_doc[-1]) + 1
    pos, fl, fr, doc_lens = [0] * S, [0] * S, [0] * S, [0] * D
    for s in range(S):
        if s == 0 or seg_doc[s] != seg_doc[s - 1]:
            pos[s] = int(lead)
            fl[s] = min(F, n[s] // 2)
        if s == S - 1 or seg_doc[s + 1] != seg_doc[s]:
            fr[s] = min(F, n[s] // 2)
            doc_lens[int(seg_doc[s])] = pos[s] + n[s] + int(tail)
            continue
        p = int(pause_after[s])
        ov = 0
        if p < 0 and n[s] > 0 and n[s + 1] > 0:
            ov = min(-p, F, n[s] // 2, n[s + 1] // 2)
        gap = max(p, 0) if ov == 0 else 0
        pos[s + 1] = pos[s] + n[s] + gap - ov
        fr[s] = ov if ov > 0 else min(F, n[s] // 2)
        fl[s + 1] = ov if ov > 0 else min(F, n[s + 1] // 2)
    return (np.array(pos, np.int64), np.array(fl, np.int32), np.array(fr, np.int32), np.array(doc_lens, np.int64))


def ramp(i, L, tab):
    """r(i, L) for an int64 index array i: tab[((2 i + 1) F) / (2 L)] where i < L, 1.0f elsewhere or when L = 0."""
    i = np.asarray(i, np.int64)
    out = np.ones(i.shape, np.float32)
    if L > 0:
        F = len(tab)
        m = i < L
        out[m] = np.asarray(tab, np.float32)[((2 * i[m] + 1) * F) // (2 * L)]
    return out


def contribution(x, fl, fr, tab):
    """c[i] = x[i] * (r(i, fl) * r(n - 1 - i, fr)): two rounded float32 products."""
    x = np.asarray(x, np.float32)
    i = np.arange(x.size, dtype=np.int64)
    g = (ramp(i, int(fl), tab) * ramp(x.size - 1 - i, int(fr), tab)).astype(np.float32)
    return (x * g).astype(np.float32)


def mix(cuts, seg_doc, pos, fl, fr, doc_lens, tab):
    """cuts: the cut segments (float32 arrays, possibly empty) -> (documents, cover): per document the float32 samples and how many segments cover
    each sample.  A second contribution is added to the first in one rounded float32 sum; uncovered samples are +0.0."""
    docs = [np.zeros(int(L), np.float32) for L in doc_lens]
    cover = [np.zeros(int(L), np.int32) for L in doc_lens]
    for s, x in enumerate(cuts):
        d = int(seg_doc[s])
        c = contribution(x, fl[s], fr[s], tab)
        lo, hi = int(pos[s]), int(pos[s]) + c.size
        first = cover[d][lo:hi] == 0
        seg = docs[d][lo:hi]
        docs[d][lo:hi] = np.where(first, c, (seg + c).astype(np.float32))
        cover[d][lo:hi] += 1
    return docs, cover


def to_i16(x):
    """(int)(x * 32768.0f) truncated toward zero, then clamped to [-32768, 32767]."""
    v = (np.asarray(x, np.float32) * np.float32(32768.0)).astype(np.float32)
    return np.clip(np.trunc(v.astype(np.float64)), -32768, 32767).astype(np.int16)


def stitch(wavs, seg_doc, pause_after, tab, trim_frac=0.0, trim_abs=0.0, keep=0, lead=0, tail=0):
    """The whole specification on host segments; F = len(tab).  Returns dict(docs, cover, pos, start, end, peak, fl, fr, doc_lens)."""
    abp = [cut(w, trim_frac, trim_abs, keep) for w in wavs]
    a = np.array([v[0] for v in abp], np.int64)
    b = np.array([v[1] for v in abp], np.int64)
    peak = np.array([v[2] for v in abp], np.float32)
    pos, fl, fr, doc_lens = plan(b - a, seg_doc, pause_after, len(tab), lead, tail)
    cuts = [np.asarray(w, np.float32)[a[s]:b[s]] for s, w in enumerate(wavs)]
    docs, cover = mix(cuts, seg_doc, pos, fl, fr, doc_lens, tab)
    return dict(docs=docs, cover=cover, pos=pos, start=a, end=b, peak=peak, fl=fl, fr=fr, doc_lens=doc_lens)
