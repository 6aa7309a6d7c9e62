"""CPU checks of ev_compare's oracle (tests/compare_oracle.py), of the precision ladder (emotivoice_amd/precision_guard.py) through measure= fakes,
and of the new ABI surface."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import compare_oracle as co
from conftest import ROOT

from emotivoice_amd import _ffi


def _signals(seed, n, dc=0.05, noise=1e-3):
    rng = np.random.default_rng(seed)
    b = (0.3 * rng.standard_normal(n) + dc).astype(np.float32)
    a = (b + noise * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    return a, b


@pytest.mark.parametrize("n", [1, 255, 257, 4096, 4097, 3 * 4096 + 5, 50001])
def test_oracle_sums_agree_with_fsum(n):
    """The ordered sum of n terms carries at most (n - 1) roundings of at most 2^-53 * (the running sum <= sum |term|) each, to first order; the
    bound 4 n 2^-53 sum |term| leaves the second-order terms room."""
    a, b = _signals(n, n)
    d, y, bad = co.terms(a, b)
    assert not bad.any()
    seg = co.compare_segment(a, b)
    for key, t in (("sum_d", d), ("sum_d2", d * d), ("sum_y", y), ("sum_y2", y * y)):
        exact = math.fsum(t.tolist())
        assert abs(float(seg[key]) - exact) <= 4 * n * 2.0 ** -53 * math.fsum(np.abs(t).tolist()), key


@pytest.mark.parametrize("n,dc", [(257, 0.0), (4097, 0.02), (3 * 4096 + 5, -0.02), (50001, 0.01)])
def test_oracle_rel_l2_ac_is_the_two_pass_measure(n, dc):
    """One-pass variance against the two-pass rel_l2_ac the parity tests use; |mean| <= 0.1 rms, so the cancellation loses nothing."""
    from test_gpu_parity import rel_l2_ac
    a, b = _signals(100 + n, n, dc=dc)
    b64 = b.astype(np.float64)
    assert abs(b64.mean()) <= 0.1 * np.sqrt(np.mean(b64 * b64))
    seg = co.compare_segment(a, b)
    want = rel_l2_ac(a, b)
    assert abs(float(seg["rel_l2_ac"]) - want) <= 1e-9 * want
    want_l2 = float(np.linalg.norm(a.astype(np.float64) - b64) / np.linalg.norm(b64))
    assert abs(float(seg["rel_l2"]) - want_l2) <= 1e-9 * want_l2


def test_oracle_nonfinite_floor_and_argmax():
    a, b = _signals(3, 5000)
    a[4095], a[4096], b[4097] = np.nan, np.inf, np.nan
    b[17], a[17] = 0.25, 0.75
    b[4500], a[4500] = 0.25, -0.25          # the same |d| later: the first index wins
    seg = co.compare_segment(a, b)
    assert int(seg["nonfinite"]) == 3 and int(seg["argmax_d"]) == 17 and float(seg["max_abs_d"]) == 0.5
    assert all(np.isfinite(float(seg[k])) for k in ("sum_d", "sum_d2", "sum_y", "sum_y2", "rel_l2", "rel_l2_ac"))
    z = co.compare_segment(np.ones(300, np.float32), np.zeros(300, np.float32))      # an all-zero yardstick: the floor
    assert float(z["rel_l2"]) == float(z["rel_l2_ac"]) == math.sqrt(300.0) / math.sqrt(co.FLOOR)
    same = co.compare_segment(b, b)
    assert float(same["sum_d2"]) == 0.0 and float(same["rel_l2_ac"]) == 0.0 and int(same["argmax_d"]) == 0 and int(same["nonfinite"]) == 1


# ----------------------------------------------------------------------------------------------------------------- the ladder
def _fake(levels, nonfinite=None, yard_nonfinite=0):
    """measure= stand-in: levels maps a rung's (name, sorted kwargs) to its per-utterance rel_l2_ac; records the rungs asked for."""
    calls = []

    def measure(rung):
        calls.append(rung)
        if rung is None:
            return dict(rel_l2_ac=[0.0], max_abs_d=[0.0], mel_rel_l2=[0.0], nonfinite=yard_nonfinite, worst_chunk=dict(utterance=0, offset=0, ratio=0.0),
                        duration_mismatch=0)
        key = (rung[0], tuple(sorted(rung[1].items())))
        vals = levels[key]
        return dict(rel_l2_ac=list(vals), max_abs_d=[1e-4] * len(vals), mel_rel_l2=[1e-6] * len(vals), nonfinite=(nonfinite or {}).get(key, 0),
                    worst_chunk=dict(utterance=int(np.argmax(vals)), offset=4096, ratio=2 * max(vals)), duration_mismatch=1)
    measure.calls = calls
    return measure


MX, MX32 = ("mx", ()), ("mx", (("mx_residual", "fp32"),))


def _choose(measure, **kw):
    from emotivoice_amd.precision_guard import choose_precision
    return choose_precision(None, b"", measure=measure, **kw)


def test_ladder_first_rung_under_the_bar():
    from emotivoice_amd.precision_guard import LADDER
    assert LADDER == [("mx", {}), ("mx", {"mx_residual": "fp32"}), ("strict", {})]
    m = _fake({MX: [4e-4, 9.9e-4, 2e-4]})
    rep = _choose(m)
    assert (rep.chosen, rep.chosen_kwargs, rep.chosen_index, rep.escalated) == ("mx", {}, 0, False)
    assert m.calls == [None, ("mx", {})] and len(rep.rungs) == 1      # nothing beyond the winner is built
    r = rep.rungs[0]
    assert r["accepted"] and r["worst_rel_l2_ac"] == 9.9e-4 and r["worst_chunk"]["utterance"] == 1 and r["duration_mismatch"] == 1
    d = json.loads(json.dumps(rep.as_dict()))
    assert d["chosen"] == "mx" and d["rungs"][0]["rel_l2_ac"] == [4e-4, 9.9e-4, 2e-4] and "mx" in rep.line()


def test_ladder_second_rung_and_fall_through_to_strict():
    rep = _choose(_fake({MX: [4e-4, 1.2e-3], MX32: [7e-4, 8e-4]}))
    assert (rep.chosen, rep.chosen_kwargs, rep.chosen_index, rep.escalated) == ("mx", {"mx_residual": "fp32"}, 1, True)
    assert [r["accepted"] for r in rep.rungs] == [False, True]
    m = _fake({MX: [4e-4, 1.2e-3], MX32: [1.01e-3, 8e-4]})
    rep = _choose(m)
    assert (rep.chosen, rep.chosen_kwargs, rep.chosen_index) == ("strict", {}, 2)
    assert [r["accepted"] for r in rep.rungs] == [False, False, True] and rep.rungs[2]["measured"] is False
    assert m.calls == [None, ("mx", {}), ("mx", {"mx_residual": "fp32"})]      # strict is accepted by construction, never measured


def test_ladder_bar_is_inclusive_and_guard_scales_it():
    assert _choose(_fake({MX: [1e-3]})).chosen_index == 0                      # <= bar
    levels = {MX: [8.4e-4], MX32: [6e-4]}
    assert _choose(_fake(levels), guard=1.0).chosen_index == 0
    rep = _choose(_fake(levels), guard=0.8)                                    # 8.4e-4 > 8e-4
    assert rep.chosen_index == 1 and rep.limit == pytest.approx(8e-4)
    assert _choose(_fake(levels), bar=5e-4, guard=1.0).chosen == "strict"
    assert _choose(_fake(levels), bar=5e-4, guard=2.0).chosen_index == 0


def test_ladder_skips_a_nonfinite_rung_and_a_nan_ratio():
    rep = _choose(_fake({MX: [1e-5], MX32: [6e-4]}, nonfinite={MX: 2}))
    assert rep.chosen_index == 1 and rep.rungs[0]["nonfinite"] == 2 and not rep.rungs[0]["accepted"]
    assert _choose(_fake({MX: [float("nan")], MX32: [6e-4]})).chosen_index == 1


def test_nonfinite_yardstick_raises():
    from emotivoice_amd.engine import EVError
    m = _fake({MX: [1e-5]}, yard_nonfinite=3)
    with pytest.raises(EVError, match="yardstick"):
        _choose(m)
    assert m.calls == [None]


def test_ladder_arguments_are_checked():
    with pytest.raises(ValueError, match="strict"):
        _choose(_fake({MX: [1e-5]}), ladder=[("mx", {})])
    with pytest.raises(ValueError):
        _choose(_fake({MX: [1e-5]}), bar=0.0)
    rep = _choose(_fake({("fast", ()): [3e-3], MX: [5e-4]}), ladder=[("fast", {}), ("mx", {}), ("strict", {})])
    assert (rep.chosen, rep.chosen_index) == ("mx", 1)


def test_worst_chunk_names_utterance_and_offset():
    from emotivoice_amd.precision_guard import worst_chunk
    cmp = dict(chunk_d2=np.array([1e-8, 1e-8, 4e-6, 1e-8]), chunk_y2=np.array([1.0, 1.0, 1.0, 0.5]), chunk_offsets=np.array([0, 1, 4]))
    assert worst_chunk(cmp) == dict(utterance=1, offset=4096, ratio=pytest.approx(2e-3))


# ----------------------------------------------------------------------------------------------------------------- the verified load
def _generator(monkeypatch, calls, chosen=("mx", {}), index=0, **kw):
    from emotivoice_amd import generator, precision_guard

    def fake_choose(shapes, blob, **kwargs):
        calls.append(kwargs)
        rep = precision_guard.PrecisionReport(bar=kwargs.get("bar", 1e-3), guard=kwargs.get("guard", 1.0))
        rep.chosen, rep.chosen_kwargs, rep.chosen_index = chosen[0], dict(chosen[1]), index
        return rep
    monkeypatch.setattr(generator, "pack_state_dict", lambda sd, shapes, pe_len: (b"blob", None))
    monkeypatch.setattr(precision_guard, "choose_precision", fake_choose)
    return generator.JETSGeneratorHIP(**kw)


def test_verify_none_never_calls_the_guard(monkeypatch, recwarn):
    calls = []
    gen = _generator(monkeypatch, calls)
    assert gen.load_state_dict({"am.x": 0}) is gen and gen.load_state_dict({"am.x": 0}, strict=True, verify=None) is gen
    assert calls == [] and gen.precision_report is None and gen._engine_kwargs == {} and gen._precision == "mx" and len(recwarn) == 0


def test_verify_runs_the_guard_and_moves_the_object(monkeypatch):
    calls = []
    gen = _generator(monkeypatch, calls)
    gen.load_state_dict({"am.x": 0}, verify=dict(bar=2e-3))
    assert calls == [dict(bar=2e-3, device=0)] and gen.precision_report.chosen == "mx" and gen._engine_kwargs == {} and gen._precision == "mx"
    calls.clear()
    gen = _generator(monkeypatch, calls, chosen=("mx", {"mx_residual": "fp32"}), index=1)
    with pytest.warns(RuntimeWarning, match="precision bar") as w:
        gen.load_state_dict({"am.x": 0}, verify=True)
    assert len(w) == 1 and (gen._precision, gen._engine_kwargs) == ("mx", {"mx_residual": "fp32"}) and gen._engine is None
    gen.load_state_dict({"am.x": 0}, verify=True)          # the next verified load judges the requested mode again
    assert len(calls) == 2


def test_unverified_load_returns_to_the_requested_precision(monkeypatch):
    """The rung and the report belong to the weights they were measured on."""
    calls = []
    gen = _generator(monkeypatch, calls, chosen=("strict", {}), index=2)
    with pytest.warns(RuntimeWarning):
        gen.load_state_dict({"am.x": 0}, verify=True)
    assert (gen._precision, gen._engine_kwargs) == ("strict", {}) and gen.precision_report is not None
    gen.load_state_dict({"am.x": 0})
    assert (gen._precision, gen._dec_prec, gen._voc_prec, gen._engine_kwargs) == ("mx", None, None, {}) and gen.precision_report is None
    gen = _generator(monkeypatch, calls, chosen=("mx", {"mx_residual": "fp32"}), index=1)
    with pytest.warns(RuntimeWarning):
        gen.load_state_dict({"am.x": 0}, verify=True)
    gen.load_packed(b"blob")
    assert (gen._precision, gen._engine_kwargs) == ("mx", {}) and gen.precision_report is None


def test_verify_leaves_explicit_modes_alone(monkeypatch):
    for kw in (dict(precision="fast"), dict(precision="strict"), dict(vocoder_precision="x3")):
        calls = []
        gen = _generator(monkeypatch, calls, chosen=("strict", {}), index=2, **kw)
        gen.load_state_dict({"am.x": 0}, verify=True)
        assert calls == [] and gen.precision_report is None and gen._engine_kwargs == {}


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_ev_compare_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "evhip.h")).read()
    assert re.search(r"\bint\s+ev_compare\s*\(\s*ev_handle\s*\*", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert re.search(r"#define EV_COMPARE_CHUNK\s+4096\b", hdr) and re.search(r"#define EV_COMPARE_FLOOR\s+1e-60\b", hdr)
    assert (_ffi.EV_COMPARE_CHUNK, _ffi.EV_COMPARE_FLOOR, co.CHUNK, co.FLOOR) == (4096, 1e-60, 4096, 1e-60)
    assert "ev_compare" in _ffi.SIGNATURES and hasattr(_ffi.lib(), "ev_compare")
    assert _ffi.lib().ev_compare(None, 1, None, None, None, 0, None) < 0          # a NULL handle is refused before anything is touched


def test_ev_compare_result_layout_matches_the_header(tmp_path):
    fields = [f[0] for f in _ffi.ev_compare_result._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evhip.h"\nint main(){printf("%zu", sizeof(ev_compare_result));\n'
                   + "".join('printf(" %%zu", offsetof(ev_compare_result, %s));\n' % f for f in fields) + "return 0;}")
    exe = tmp_path / "sz"
    if shutil.which("gcc") is None:
        pytest.skip("gcc not installed")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_ffi.ev_compare_result)] + [getattr(_ffi.ev_compare_result, f).offset for f in fields]
