"""CPU checks of ev_score (include/evhip.h): the design table against scipy, the oracle (tests/score_oracle.py) against an independent plain DTW on
Python integers and against known answers, the tie case that pins the predecessor rule, the host ratios, every rejection that needs no device, and
the boundary (header, binding, struct layout, the host side of emotivoice_amd/scoring.py)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import score_oracle as so
from conftest import ROOT
from emotivoice_amd import _ffi
from emotivoice_amd.scoring import ScoreConfig, corpus_means

LIB = _ffi.lib()


def _mel(T, seed, n_mels=80):
    return (np.random.default_rng(seed).standard_normal((n_mels, T)) * 1.5 - 4.0).astype(np.float32)


def dtw_plain(dist):
    """The independent statement of step 4: a triple loop (rows, columns, the three predecessors in the rule's order) on Python ints."""
    Ta, Tb = len(dist), len(dist[0])
    A = [[None] * Tb for _ in range(Ta)]
    back = [[None] * Tb for _ in range(Ta)]
    for i in range(Ta):
        for j in range(Tb):
            if i == 0 and j == 0:
                A[0][0] = int(dist[0][0])
                continue
            best = None
            for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):          # diagonal, a-step, b-step: the first of the cheapest wins
                if pi < 0 or pj < 0:
                    continue
                if best is None or A[pi][pj] < best[0]:
                    best = (A[pi][pj], pi, pj)
            A[i][j] = int(dist[i][j]) + best[0]
            back[i][j] = (best[1], best[2])
    path, cell = [], (Ta - 1, Tb - 1)
    while cell is not None:
        path.append(cell)
        cell = back[cell[0]][cell[1]]
    return A[Ta - 1][Tb - 1], path[::-1]


def test_design_table_against_scipy_within_one_ulp():
    """1 fp32 ulp of scipy's value everywhere the DCT is not exactly zero.  Where it is -- d (2 m + 1) an odd multiple of M, told by integer
    arithmetic -- scipy's own value is fp64 rounding noise (1e-17, or 0.0) and an ulp of it means nothing; there both tables are held to the error of
    an fp64 evaluation instead: the argument pi d (m + 0.5) / M is rounded three times, |d cos| <= 1, so |entry| <= sqrt(2 / M) * pi * d * 2^-51."""
    from scipy.fft import dct
    for M, D in ((80, 13), (80, 32), (128, 32), (2, 1), (33, 32)):
        got = so.design(M, D)
        full = dct(np.eye(M, dtype=np.float64), type=2, norm="ortho", axis=0)          # full[d] = row d of the orthonormal DCT-II
        want = full[1:D + 1]
        d, m = np.arange(1, D + 1)[:, None], np.arange(M)[None, :]
        zero = (d * (2 * m + 1)) % (2 * M) == M
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert got.shape == (D, M) and got.dtype == np.float32
        for table in (got.astype(np.float64), so.design_numpy(M, D).astype(np.float64)):
            assert (np.abs(table - want) <= ulp)[~zero].all(), (M, D, np.abs(table - want)[~zero].max())
            noise = np.sqrt(2.0 / M) * np.pi * d * 2.0 ** -51 * np.ones_like(want)
            assert (np.abs(table) <= noise)[zero].all() and (np.abs(want) <= noise)[zero].all(), (M, D)
    assert np.abs(so.design(80, 13).astype(np.float64).sum(axis=1)).max() < 1e-6          # rows 1 .. D are orthogonal to a constant: c0 is left out


def test_isqrt_is_the_floor_square_root_at_its_edges():
    s = np.array([0, 1, 2, 3, 4, 8, 9, (1 << 52) - 1, (1 << 53) + 1, (3037000499 ** 2) % (1 << 61), (1 << 61) - 1, 1 << 61, 2 ** 60 - 1, 2 ** 60, 2 ** 60 + 1,
                  (2 ** 30 + 1) ** 2 - 1, (2 ** 30 + 1) ** 2], np.int64)
    assert [int(r) for r in so.isqrt(s)] == [math.isqrt(int(v)) for v in s]


def test_oracle_dp_against_the_plain_triple_loop():
    rng = np.random.default_rng(5)
    basis = so.design(80, 13)
    for ta, tb, levels in ((1, 1, 0), (1, 9, 0), (9, 1, 0), (17, 23, 0), (40, 31, 3), (25, 25, 2)):
        if levels:          # few distinct frames: many equal distances, so the tie rule decides often
            a = rng.integers(0, levels, (80, ta)).astype(np.float32) * 0.5
            b = rng.integers(0, levels, (80, tb)).astype(np.float32) * 0.5
            a[1:], b[1:] = a[:1], b[:1]
        else:
            a, b = _mel(ta, ta * 7 + tb), _mel(tb, tb * 11 + ta)
        dm = so.dist_matrix(so.cepstra(a, basis)[0], so.cepstra(b, basis)[0])
        total, path = so.dtw(dm)
        want_total, want_path = dtw_plain(dm.tolist())
        assert total == want_total and [tuple(c) for c in path.tolist()] == want_path, (ta, tb)


def test_cepstra_follow_the_stated_order_and_rounding():
    basis = so.design(80, 13)
    mel = _mel(9, 3)
    cq, nonf = so.cepstra(mel, basis)
    for t in (0, 8):
        for d in (0, 12):
            x = 0.0
            for m in range(80):
                x = x + float(mel[m, t]) * float(basis[d, m])          # Python floats: one exact product, one rounded addition
            assert cq[t, d] == int(np.rint(x * 65536.0)), (t, d)
    assert nonf == 0 and cq.dtype == np.int32
    # ties to even on the integer grid, and the clamp: a one-mel, one-coefficient "basis" of 1 makes x the mel value itself
    one = np.ones((1, 1), np.float32)
    vals = np.array([[0.5 / 65536, 1.5 / 65536, 2.5 / 65536, -0.5 / 65536, -1.5 / 65536, 3000.0, -3000.0, 2048.0, np.nan, np.inf]], np.float32)
    cq, nonf = so.cepstra(vals, one)
    assert cq[:, 0].tolist() == [0, 2, 2, 0, -2, 1 << 27, -(1 << 27), 1 << 27, 0, 0] and nonf == 2


def test_known_answers():
    a = _mel(40, 1)
    basis = so.design(80, 13)
    shifted = (a + np.float32(0.25) * basis[2][:, None]).astype(np.float32)          # 0.25 of basis row 3 added to every frame
    res = so.score([a, a, a], [a, np.repeat(a, 2, axis=1), shifted])
    assert res["sum_dist"][0] == 0 and res["path_len"][0] == 40 and res["n_diag"][0] == 39 and res["n_a"][0] == 0 and res["n_b"][0] == 0
    assert res["sum_dist"][1] == 0 and res["path_len"][1] == 80 and (res["n_diag"][1], res["n_a"][1], res["n_b"][1]) == (39, 0, 40)
    assert np.array_equal(res["path_list"][1][:, 0], np.arange(80) // 2) and np.array_equal(res["path_list"][1][:, 1], np.arange(80))
    assert (res["n_diag"][2], res["n_a"][2], res["n_b"][2]) == (39, 0, 0)
    exact = (10.0 / math.log(10.0)) * math.sqrt(2.0) * 0.25          # 1.53546...
    # every coefficient is within 2^-16 nat (two roundings to the 1 / 65536 grid and the fp32 rounding of the shifted mel) of its exact value
    assert abs(exact - 1.53546) < 1e-5 and abs(res["mcd_db"][2] - exact) <= (10.0 / math.log(10.0)) * math.sqrt(2.0) * math.sqrt(13.0) * 2.0 ** -16
    assert res["mcd_db"][0] == 0.0 and res["warp"][1] == 0.5 and res["warp"][2] == 0.0


def test_the_tie_case_pins_the_predecessor_rule():
    a, b = so.tie_case()
    assert set(np.unique(a)) <= {0.0, 0.5, 1.0} and set(np.unique(b)) <= {0.0, 0.5, 1.0}
    assert (a[:, 8:18] == a[:, 8:9]).all() and b.shape[1] > a.shape[1]
    basis = so.design(80, 13)
    cqa, cqb = so.cepstra(a, basis)[0], so.cepstra(b, basis)[0]
    dm = so.dist_matrix(cqa, cqb)
    total, path = so.dtw(dm)
    assert (total, [tuple(c) for c in path.tolist()]) == dtw_plain(dm.tolist())
    paths = {tie: so.dtw(dm, tie) for tie in so.TIE_RULES}
    for tie in so.TIE_RULES[1:]:
        assert paths[tie][0] == total, tie          # the same cost: only the choice among equal predecessors differs
        assert paths[tie][1].shape != path.shape or not np.array_equal(paths[tie][1], path), tie
    assert not cqa[19].any() and np.array_equal(cqa[20], -cqb[int(np.where((cqb == -cqa[20]).all(axis=1))[0][0])])          # X is 0, Y' mirrors Y
    g = int(so.isqrt(np.array([(cqa[20].astype(np.int64) ** 2).sum()]))[0])
    assert total == 2 * g and int(so.isqrt(np.array([4 * (cqa[20].astype(np.int64) ** 2).sum()]))[0]) > 2 * g


def test_f0_sums_and_host_ratios():
    a, b = _mel(30, 1), _mel(30, 2)
    f0a = np.full(30, 220.0, np.float32)
    f0b = np.full(30, 110.0, np.float32)
    f0a[:5], f0b[3:8], f0a[20], f0b[21] = 0.0, 0.0, np.nan, -5.0
    res = so.score([a], [b], [f0a], [f0b], linear=True)
    assert (res["n_vv"][0], res["n_vu"][0], res["n_uv"][0], res["n_uu"][0]) == (20, 4, 4, 2)
    assert res["sum_c"][0] == 20 * 1200.0 and res["sum_c2"][0] == 20 * 1200.0 ** 2
    assert res["f0_rmse_cents"][0] == 1200.0 and res["f0_bias_cents"][0] == 1200.0 and res["vuv_error"][0] == 8 / 30
    r = so.ratios(sum_dist=65536 * 30, K=30, n_a=3, n_b=6, n_vv=0, n_vu=1, n_uv=2, sum_c=0.0, sum_c2=0.0)
    assert math.isnan(r["f0_rmse_cents"]) and math.isnan(r["f0_bias_cents"])          # the NaN rule for n_vv = 0
    assert r["mcd_db"] == (10.0 / math.log(10.0)) * math.sqrt(2.0) * (float(65536 * 30) / 65536.0) / 30.0 and abs(r["mcd_db"] - 6.1418514637) < 1e-9
    assert r["vuv_error"] == 0.1 and r["warp"] == 0.3
    none = so.score([a], [b], None, [f0b])
    assert none["n_vv"][0] == 0 and none["sum_c"][0] == 0.0 and math.isnan(none["f0_rmse_cents"][0])
    cm = corpus_means(so.score([a, a], [b, a], [f0a, f0a], [f0b, f0a], linear=True))
    assert cm["path_len"] == 60 and cm["pairs"] == 2 and cm["n_vv"] == 20 + 24 and cm["f0_bias_cents"] == 20 * 1200.0 / 44


def test_rejections_that_need_no_device():
    def err():
        return LIB.ev_last_error(None).decode()
    basis = np.zeros((32, 128), np.float32)
    for (M, D), needle in (((0, 1), "n_mels = 0"), ((129, 13), "n_mels = 129"), ((80, 0), "n_ceps = 0"), ((80, 33), "n_ceps = 33"),
                           ((13, 13), "n_ceps = 13"), ((1, 1), "n_ceps = 1")):
        assert LIB.ev_score_design(M, D, basis.ctypes.data_as(C.c_void_p)) != 0 and "ev_score_design" in err() and needle in err(), (M, D, err())
    assert LIB.ev_score_design(80, 13, None) != 0 and "basis is NULL" in err()
    assert LIB.ev_score_design(128, 32, basis.ctypes.data_as(C.c_void_p)) == 0 and LIB.ev_score_design(2, 1, basis.ctypes.data_as(C.c_void_p)) == 0
    mel = np.zeros(80 * 8, np.float32)
    lens = np.array([3, 5], np.int32)

    def load(side=0, B=2, M=80, D=13, mel_p=mel.ctypes.data, lens_a=lens):
        return LIB.ev_score_load(None, side, B, M, D, C.c_void_p(mel_p), lens_a.ctypes.data_as(C.c_void_p) if lens_a is not None else None, None, 0)
    for kw, needle in ((dict(mel_p=0), "mel is NULL"), (dict(lens_a=None), "lens is NULL"), (dict(side=2), "side = 2"), (dict(side=-1), "side = -1"),
                       (dict(B=0), "B = 0"), (dict(B=65536), "B = 65536"), (dict(M=0), "n_mels = 0"), (dict(M=129), "n_mels = 129"),
                       (dict(D=0), "n_ceps = 0"), (dict(D=33), "n_ceps = 33"), (dict(M=8, D=8), "n_ceps = 8"),
                       (dict(lens_a=np.array([3, 0], np.int32)), "lens[1] = 0"), (dict(lens_a=np.array([4097, 5], np.int32)), "lens[0] = 4097"),
                       (dict(), "h is NULL")):
        assert load(**kw) != 0 and "ev_score_load" in err() and needle in err(), (kw, err())
    res = _ffi.ev_score_result()
    assert LIB.ev_score(None, 0, None) != 0 and "out is NULL" in err()
    res.struct_size = 8
    assert LIB.ev_score(None, 0, C.byref(res)) != 0 and "struct_size" in err()
    res.struct_size = C.sizeof(_ffi.ev_score_result)
    assert LIB.ev_score(None, 0, C.byref(res)) != 0 and "h is NULL" in err()


def _plan(la, lb):
    la, lb = np.ascontiguousarray(la, np.int32), np.ascontiguousarray(lb, np.int32)
    pass_of, pass_bytes = np.full(la.size, -1, np.int32), np.zeros(la.size, np.int64)
    n = LIB.ev_score_plan(la.size, la.ctypes.data_as(C.c_void_p), lb.ctypes.data_as(C.c_void_p), pass_of.ctypes.data_as(C.c_void_p),
                          pass_bytes.ctypes.data_as(C.c_void_p))
    return n, pass_of, pass_bytes[:max(n, 0)]


def test_the_planned_workspace_stays_within_one_gib():
    """ev_score_plan is the layout ev_score uses; its workspace for distances and decisions is one buffer of the largest pass.  A pass of long
    pairs (a run of 64: decisions 1 / 16 of the distances) followed by passes of pairs with a short a (a run of 1: decisions as large as the
    distances) is the batch whose two kinds of words peak in different passes."""
    def need(ta, tb):
        rm = 1
        while rm * 64 < ta:
            rm *= 2
        return (tb + 63) * 64 * 4 * (rm + max(rm // 16, 1))
    GIB = _ffi.EV_SCORE_WORKSPACE
    assert GIB == 1 << 30 and need(4096, 4096) == 4159 * 4096 * 4 + 4159 * 64 * 16
    la, lb = [4096] * 14 + [64] * 510, [4096] * 524
    n, pass_of, pass_bytes = _plan(la, lb)
    assert n == 2 and (pass_bytes <= GIB).all() and pass_bytes.min() > GIB * 0.9          # 14 long and 28 short pairs, then 482 short ones
    assert (np.diff(pass_of) >= 0).all() and pass_of[0] == 0 and pass_of[-1] == n - 1          # whole consecutive pairs
    for q in range(n):
        assert pass_bytes[q] == sum(need(x, y) for x, y, k in zip(la, lb, pass_of) if k == q)
        if q + 1 < n:          # greedy: the next pair did not fit
            first = int(np.argmax(pass_of == q + 1))
            assert pass_bytes[q] + need(la[first], lb[first]) > GIB
    rng = np.random.default_rng(3)
    la, lb = rng.integers(1, 4097, 3000), rng.integers(1, 4097, 3000)
    n, pass_of, pass_bytes = _plan(la, lb)
    assert n > 10 and (pass_bytes <= GIB).all() and pass_bytes.sum() == sum(need(x, y) for x, y in zip(la, lb))
    assert _plan([1], [1])[0] == 1 and _plan([4096], [4096])[2][0] == need(4096, 4096) < GIB // 14

    def err():
        return LIB.ev_last_error(None).decode()
    assert _plan([0], [5])[0] == -1 and "lens_a[0] = 0" in err()
    assert _plan([5, 5], [5, 4097])[0] == -1 and "lens_b[1] = 4097" in err()
    assert LIB.ev_score_plan(1, None, None, None, None) == -1 and "NULL" in err()
    one = np.ones(1, np.int32)
    assert LIB.ev_score_plan(0, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p),
                             np.zeros(1, np.int64).ctypes.data_as(C.c_void_p)) == -1 and "B = 0" in err()


def test_header_binding_and_struct_layout(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "evhip.h")).read()
    for name, val in (("EV_SCORE_MAX_FRAMES", "4096"), ("EV_SCORE_MAX_CEPS", "32"), ("EV_SCORE_Q", "65536"), ("EV_SCORE_CLAMP", "(1 << 27)"),
                      ("EV_SCORE_LINEAR", "0x1u")):
        assert "#define %s" % name in hdr and val in hdr.split("#define %s" % name)[1].split("\n")[0], name
    assert (_ffi.EV_SCORE_MAX_FRAMES, _ffi.EV_SCORE_MAX_CEPS, _ffi.EV_SCORE_Q, _ffi.EV_SCORE_CLAMP, _ffi.EV_SCORE_LINEAR) == (4096, 32, 65536, 1 << 27, 1)
    assert "not SPTK" in hdr.replace("NOT", "not") and "EV_ABI_VERSION 7" in hdr
    for name, nargs in (("ev_score_design", 3), ("ev_score_load", 9), ("ev_score", 3), ("ev_score_plan", 5)):
        assert len(_ffi.SIGNATURES[name][1]) == nargs and hasattr(LIB, name), name
    if shutil.which("gcc") is None:
        pytest.skip("gcc not installed")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evhip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(ev_score_result), '
                   'offsetof(ev_score_result, sum_dist), offsetof(ev_score_result, sum_c), offsetof(ev_score_result, path_offsets), '
                   'offsetof(ev_score_result, cq_b));return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = _ffi.ev_score_result
    assert sizes == [C.sizeof(R), R.sum_dist.offset, R.sum_c.offset, R.path_offsets.offset, R.cq_b.offset]


def test_score_config_and_tools_parse():
    assert ScoreConfig().validate().n_ceps == 13 and not ScoreConfig().linear
    for bad in (0, 33):
        with pytest.raises(ValueError):
            ScoreConfig(n_ceps=bad).validate()
    with pytest.raises(ValueError):
        ScoreConfig(n_ceps=13).validate(n_mels=13)
    import importlib.util
    for tool in ("score_corpus", "bench_score"):
        spec = importlib.util.spec_from_file_location(tool, os.path.join(ROOT, "tools", tool + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert callable(mod.main)
