"""numpy / Python-integer restatement of ev_score (include/evhip.h, steps 1-6): the basis (taken from ev_score_design, so libm's cos is not a
source of mismatch), the integer cepstra with their fp64 summation order, the integer local distance, the DTW recurrence with its tie rule, the
backtrack, the sums along the path and the host ratios.  Everything but the two F0 sums is exact; the test files compare it bit for bit.

The DP runs over anti-diagonals in int64 (values stay below 2^44); ``dtw_plain`` in tests/test_score.py is the independent statement on Python ints."""
import ctypes as C
import math

import numpy as np

Q, CLAMP, MAX_FRAMES, MAX_CEPS = 65536, 1 << 27, 4096, 32
INF = np.int64(1) << np.int64(62)
INT_KEYS = ("path_len", "n_diag", "n_a", "n_b", "n_vv", "n_vu", "n_uv", "n_uu", "nonfinite_a", "nonfinite_b", "lens_a", "lens_b")
EXACT_KEYS = ("sum_dist",) + INT_KEYS
TIE_ROW = 13
TIE_RULES = ("spec", "a_before_diag", "b_before_a")      # the specification's order and the two wrong ones the tie case tells apart


def design(n_mels: int, n_ceps: int) -> np.ndarray:
    """The (n_ceps, n_mels) fp32 table of ev_score_design."""
    from emotivoice_amd import _ffi
    basis = np.zeros((n_ceps, n_mels), np.float32)
    if _ffi.lib().ev_score_design(n_mels, n_ceps, basis.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError(_ffi.lib().ev_last_error(None).decode())
    return basis


def design_numpy(n_mels: int, n_ceps: int) -> np.ndarray:
    """Step 1 in numpy: what ev_score_design computes up to libm's cos (the CPU test holds the two within 1 ulp)."""
    d = np.arange(1, n_ceps + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return (np.sqrt(2.0 / n_mels) * np.cos(np.pi * d * (m + 0.5) / n_mels)).astype(np.float32)


def cepstra(mel: np.ndarray, basis: np.ndarray):
    """Step 2 for one signal: mel (n_mels, T) fp32 -> (cq (T, D) int32, the number of frames that hold a non-finite mel value)."""
    mel = np.asarray(mel, np.float32)
    m64, b64 = mel.astype(np.float64), basis.astype(np.float64)
    x = np.zeros((mel.shape[1], basis.shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(mel.shape[0]):          # m ascending: one exact product and one rounded addition per term
            x = x + m64[m][:, None] * b64[:, m][None, :]
        y = np.clip(x * float(Q), -float(CLAMP), float(CLAMP))
    cq = np.where(np.isfinite(x), np.rint(np.where(np.isfinite(x), y, 0.0)), 0.0).astype(np.int32)
    return cq, int((~np.isfinite(mel)).any(axis=0).sum())


def isqrt(s: np.ndarray) -> np.ndarray:
    """The largest r with r * r <= s, elementwise on int64 (s < 2^61)."""
    s = np.asarray(s, np.int64)
    r = np.floor(np.sqrt(s.astype(np.float64))).astype(np.int64)
    for _ in range(4):
        r = r - (r * r > s)
    for _ in range(4):
        r = r + ((r + 1) * (r + 1) <= s)
    assert ((r * r <= s) & ((r + 1) * (r + 1) > s)).all()
    return r


def dist_matrix(cqa: np.ndarray, cqb: np.ndarray) -> np.ndarray:
    """Step 3: (Ta, Tb) int64."""
    a, b = cqa.astype(np.int64), cqb.astype(np.int64)
    s = np.zeros((a.shape[0], b.shape[0]), np.int64)
    for d in range(a.shape[1]):
        e = a[:, d][:, None] - b[:, d][None, :]
        s += e * e
    return isqrt(s)


def dtw(dist: np.ndarray, tie: str = "spec"):
    """Step 4: (A[Ta-1][Tb-1], the path as a (K, 2) int32 array, ascending).  ``tie``: TIE_RULES."""
    Ta, Tb = dist.shape
    A = np.full((Ta + 1, Tb + 1), INF, np.int64)          # A[i + 1][j + 1] holds cell (i, j); row 0 and column 0 are the infinite border
    code = np.zeros((Ta, Tb), np.uint8)                   # 0 diagonal, 1 a-step (i-1, j), 2 b-step (i, j-1)
    A[1, 1] = dist[0, 0]
    for k in range(1, Ta + Tb - 1):
        i = np.arange(max(0, k - Tb + 1), min(Ta - 1, k) + 1)
        j = k - i
        dg, up, left = A[i, j], A[i, j + 1], A[i + 1, j]
        if tie == "spec":
            c = np.where((dg <= up) & (dg <= left), 0, np.where(up <= left, 1, 2))
        elif tie == "a_before_diag":
            c = np.where((up <= dg) & (up <= left), 1, np.where(dg <= left, 0, 2))
        elif tie == "b_before_a":
            c = np.where((dg <= up) & (dg <= left), 0, np.where(left <= up, 2, 1))
        else:
            raise ValueError(tie)
        A[i + 1, j + 1] = dist[i, j] + np.where(c == 0, dg, np.where(c == 1, up, left))
        code[i, j] = c
    i, j = Ta - 1, Tb - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        c = code[i, j]
        if c != 2:
            i -= 1
        if c != 1:
            j -= 1
        path.append((i, j))
    return int(A[Ta, Tb]), np.array(path[::-1], np.int32).reshape(-1, 2)


def ratios(sum_dist: int, K: int, n_a: int, n_b: int, n_vv: int, n_vu: int, n_uv: int, sum_c: float, sum_c2: float):
    """Step 6, in the order the header writes it."""
    mcd = (10.0 / math.log(10.0)) * math.sqrt(2.0) * (float(sum_dist) / 65536.0) / float(K)
    rmse = math.sqrt(sum_c2 / float(n_vv)) if n_vv else math.nan
    bias = sum_c / float(n_vv) if n_vv else math.nan
    return dict(mcd_db=mcd, f0_rmse_cents=rmse, f0_bias_cents=bias, vuv_error=float(n_vu + n_uv) / float(K), warp=float(n_a + n_b) / float(K))


def score_pair(cqa, cqb, f0a=None, f0b=None, linear=False, tie="spec"):
    """Steps 3-6 of one pair from its integer cepstra."""
    Ta, Tb = cqa.shape[0], cqb.shape[0]
    if linear:
        K = min(Ta, Tb)
        path = np.stack([np.arange(K, dtype=np.int32)] * 2, 1)
        e = cqa[:K].astype(np.int64) - cqb[:K].astype(np.int64)
        sum_dist = int(isqrt((e * e).sum(axis=1)).sum())
    else:
        dm = dist_matrix(cqa, cqb)
        sum_dist, path = dtw(dm, tie)
        assert sum_dist == int(dm[path[:, 0], path[:, 1]].sum())
    K = path.shape[0]
    step = np.diff(path, axis=0)
    n_diag = int(((step[:, 0] == 1) & (step[:, 1] == 1)).sum())
    n_a = int(((step[:, 0] == 1) & (step[:, 1] == 0)).sum())
    n_b = int(((step[:, 0] == 0) & (step[:, 1] == 1)).sum())
    assert K == 1 + n_diag + n_a + n_b
    out = dict(sum_dist=sum_dist, path_len=K, n_diag=n_diag, n_a=n_a, n_b=n_b, n_vv=0, n_vu=0, n_uv=0, n_uu=0, sum_c=0.0, sum_c2=0.0, sum_abs_c=0.0,
               path=path)
    if f0a is not None and f0b is not None:
        fa, fb = np.asarray(f0a, np.float32)[path[:, 0]], np.asarray(f0b, np.float32)[path[:, 1]]
        with np.errstate(invalid="ignore"):
            va, vb = np.isfinite(fa) & (fa > 0), np.isfinite(fb) & (fb > 0)
        out.update(n_vv=int((va & vb).sum()), n_vu=int((va & ~vb).sum()), n_uv=int((~va & vb).sum()), n_uu=int((~va & ~vb).sum()))
        vv = va & vb
        c = 1200.0 * np.log2(fa[vv].astype(np.float64) / fb[vv].astype(np.float64))
        sc = sc2 = 0.0
        for v in c.tolist():          # ascending path order
            sc += v
            sc2 += v * v
        out.update(sum_c=sc, sum_c2=sc2, sum_abs_c=float(np.abs(c).sum()))
    out.update(ratios(sum_dist, K, n_a, n_b, out["n_vv"], out["n_vu"], out["n_uv"], out["sum_c"], out["sum_c2"]))
    return out


def score(feats_a, feats_b, f0_a=None, f0_b=None, linear=False, n_ceps=13, basis=None):
    """The batch: per-pair numpy arrays under the keys of EVAudio.score_to_numpy, path_list, cq_a_list / cq_b_list, and sum_abs_c (the scale of
    sum_c's tolerance)."""
    n_mels = np.asarray(feats_a[0]).shape[0]
    basis = design(n_mels, n_ceps) if basis is None else basis
    ca, cb = [cepstra(m, basis) for m in feats_a], [cepstra(m, basis) for m in feats_b]
    pairs = [score_pair(x[0], y[0], None if f0_a is None else f0_a[b], None if f0_b is None else f0_b[b], linear)
             for b, (x, y) in enumerate(zip(ca, cb))]
    out = {k: np.array([p[k] for p in pairs], np.int64 if k == "sum_dist" else np.int32) for k in ("sum_dist",) + INT_KEYS[:8]}
    for k in ("sum_c", "sum_c2", "sum_abs_c", "mcd_db", "f0_rmse_cents", "f0_bias_cents", "vuv_error", "warp"):
        out[k] = np.array([p[k] for p in pairs], np.float64)
    out["nonfinite_a"], out["nonfinite_b"] = np.array([x[1] for x in ca], np.int32), np.array([y[1] for y in cb], np.int32)
    out["lens_a"], out["lens_b"] = np.array([x[0].shape[0] for x in ca], np.int32), np.array([y[0].shape[0] for y in cb], np.int32)
    out["path_list"] = [p["path"] for p in pairs]
    out["path_offsets"] = np.concatenate([[0], np.cumsum(out["path_len"])]).astype(np.int64)
    out["cq_a_list"], out["cq_b_list"] = [x[0] for x in ca], [y[0] for y in cb]
    return out


def tie_case():
    """The named input that pins the tie rule: mel values from {0, 0.5, 1}, a with a run of ten identical frames, b built from a's frames with
    repeats.  That alone gives predecessors of equal cost between the diagonal and a step, which tells "a-step before diagonal" apart.  It cannot
    tell "b-step before a-step" apart: on a zero-cost path A[i-1][j] = A[i][j-1] = 0 forces a[i-1] = a[i] = b[j-1] = b[j], so the diagonal is 0 too
    and wins under either order.  So frames 19 .. 21 of a are X, Y, X with X = 0.5 everywhere (its cepstra are 0: rows 1 .. D of the DCT are
    orthogonal to a constant) and Y = X + 0.5 on mel row TIE_ROW, and b holds X, Y', X there with Y' = X - 0.5 on that row: cq(Y') = -cq(Y), so
    dist(Y, X) = dist(X, Y') = g exactly, and dist(Y, Y') = isqrt(4 s) > 2 isqrt(s) = 2 g because sqrt(s) has a fraction above 1/2 at this row.
    The cell after the gadget then has the a-step and the b-step at 2 g and the diagonal above them.  Returns (mel_a (80, 24), mel_b (80, Tb))."""
    rng = np.random.default_rng(1000)
    a = rng.integers(0, 3, (80, 24)).astype(np.float32) * 0.5
    a[:, 8:18] = a[:, 8:9]
    a[:, 19:22] = 0.5
    a[TIE_ROW, 20] = 1.0
    rep = rng.integers(1, 4, 24)
    rep[19:22] = 1
    b = np.repeat(a, rep, axis=1)
    b[TIE_ROW, int(rep[:20].sum())] = 0.0
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def assert_exact(got, want, name=""):
    """Every exact quantity of a device result (EVAudio.score_to_numpy with paths and cq) against the oracle's, with no tolerance."""
    for k in EXACT_KEYS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (name, k, got[k], want[k])
    assert np.array_equal(got["path_offsets"], want["path_offsets"]), (name, "path_offsets")
    for b, (g, w) in enumerate(zip(got["path_list"], want["path_list"])):
        assert g.shape == w.shape and np.array_equal(g, w), (name, "path", b)
    for side in ("a", "b"):
        if "cq_%s_list" % side in got:
            for b, (g, w) in enumerate(zip(got["cq_%s_list" % side], want["cq_%s_list" % side])):
                assert g.shape == w.shape and np.array_equal(g, w), (name, "cq_" + side, b)
    for k in ("mcd_db", "vuv_error", "warp"):          # host ratios of exact integers: the same C double operations
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (name, k, got[k], want[k])


def assert_f0_sums(got, want, name=""):
    """sum_c2 within 1e-9 relative and sum_c within 1e-9 * sum |c| absolute: at most 8191 terms with a few ulp of fp64 log2 error each is about
    4e-12; the margin covers the difference between libm's log2 and the device's."""
    for b in range(len(want["sum_c"])):
        assert abs(got["sum_c2"][b] - want["sum_c2"][b]) <= 1e-9 * abs(want["sum_c2"][b]), (name, b, got["sum_c2"][b], want["sum_c2"][b])
        assert abs(got["sum_c"][b] - want["sum_c"][b]) <= 1e-9 * want["sum_abs_c"][b], (name, b, got["sum_c"][b], want["sum_c"][b])
        for k in ("f0_rmse_cents", "f0_bias_cents"):
            if want["n_vv"][b] == 0:
                assert np.isnan(got[k][b]), (name, k, b)
            else:
                assert abs(got[k][b] - want[k][b]) <= 1e-9 * max(abs(want[k][b]), want["sum_abs_c"][b] / want["n_vv"][b]), (name, k, b)
