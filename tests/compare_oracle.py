"""numpy float64 restatement of ev_compare (include/evhip.h), the summation order included: a chunk of 4096 terms is laid out as (16, 256) with
zero padding, row r holding the elements r * 256 + t; the rows are added one after the other (thread t's ascending sum), the 256 thread sums meet
in the halving tree, and a segment's chunk sums are added in ascending order.  Padding with +0.0 changes no bit: an accumulator that starts at
+0.0 never becomes -0.0 under round-to-nearest."""
import numpy as np

CHUNK = 4096
FLOOR = 1e-60


def chunk_sum(terms):
    """terms: (<= CHUNK,) float64 -> the chunk's sum in the device's order."""
    v = np.zeros(CHUNK, np.float64)
    v[:terms.size] = terms
    rows = v.reshape(CHUNK // 256, 256)
    s = np.zeros(256, np.float64)
    for r in range(rows.shape[0]):
        s = s + rows[r]
    o = 128
    while o >= 1:
        s[:o] = s[:o] + s[o:2 * o]
        o //= 2
    return s[0]


def ordered_sum(terms):
    """(chunk sums, the segment's sum): the chunks added sequentially from +0.0."""
    cs = np.array([chunk_sum(terms[i:i + CHUNK]) for i in range(0, terms.size, CHUNK)], np.float64)
    tot = np.float64(0.0)
    for c in cs:
        tot = tot + c
    return cs, tot


def terms(a, b):
    """d, y (float64) and the non-finite mask of one segment."""
    a32, b32 = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    bad = ~(np.isfinite(a32) & np.isfinite(b32))
    x, y = a32.astype(np.float64), b32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.where(bad, 0.0, x - y)
    y = np.where(bad, 0.0, y)
    return d, y, bad


def ratios(sum_d2, sum_y, sum_y2, n):
    sum_d2, sum_y, sum_y2 = np.float64(sum_d2), np.float64(sum_y), np.float64(sum_y2)
    num = np.sqrt(sum_d2)
    rel = num / np.sqrt(np.maximum(sum_y2, np.float64(FLOOR)))
    var = sum_y2 - (sum_y * sum_y) / np.float64(n)
    return rel, num / np.sqrt(np.maximum(var, np.float64(FLOOR)))


def compare_segment(a, b):
    d, y, bad = terms(a, b)
    out = {}
    _, out["sum_d"] = ordered_sum(d)
    out["chunk_d2"], out["sum_d2"] = ordered_sum(d * d)
    _, out["sum_y"] = ordered_sum(y)
    out["chunk_y2"], out["sum_y2"] = ordered_sum(y * y)
    out["rel_l2"], out["rel_l2_ac"] = ratios(out["sum_d2"], out["sum_y"], out["sum_y2"], d.size)
    ad = np.abs(d)
    with np.errstate(over="ignore"):
        out["max_abs_d"] = np.float32(ad.max())
    out["argmax_d"] = np.int64(np.argmax(ad))          # numpy's argmax returns the first maximum
    out["peak_y"] = np.float32(np.abs(y).max())        # |y| of a float32 value: exact
    out["nonfinite"] = np.int64(bad.sum())
    return out


PER_SEGMENT = ("sum_d", "sum_d2", "sum_y", "sum_y2", "rel_l2", "rel_l2_ac", "max_abs_d", "argmax_d", "peak_y", "nonfinite")


def compare(a_list, b_list):
    """The arrays EVEngine.compare returns."""
    segs = [compare_segment(a, b) for a, b in zip(a_list, b_list)]
    out = {k: np.array([s[k] for s in segs]) for k in PER_SEGMENT}
    out["chunk_d2"] = np.concatenate([s["chunk_d2"] for s in segs])
    out["chunk_y2"] = np.concatenate([s["chunk_y2"] for s in segs])
    out["chunk_offsets"] = np.concatenate([[0], np.cumsum([s["chunk_d2"].size for s in segs])]).astype(np.int64)
    return out
