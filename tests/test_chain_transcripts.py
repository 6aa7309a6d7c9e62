"""The output chain against tests/golden/chain/transcripts.json, which tests/golden/make_golden_chain.py recorded from the commit before the chain
became emotivoice_amd/output_chain.py: for the cross product of the stage arguments of synthesize and synthesize_long, and for four sequences
of calls on one engine, the code under test asks the stand-in library (tests/fake_evhip.py) for the same calls with the same arguments, copies
the same bytes to the host, returns the same dict and rejects the same calls with the same words before any library call.  The file is never
written here: a mismatch is diffed by hand with the recorder's ``--full`` on both commits."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN_DIR

FIXTURE = os.path.join(GOLDEN_DIR, "chain", "transcripts.json")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("make_golden_chain", os.path.join(GOLDEN_DIR, "make_golden_chain.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixture_is_the_product_the_issue_lists(recorded):
    runs = recorded["product"]
    assert len(runs) == 480 and sum(k.startswith("synthesize ") for k in runs) == 288 and sum(k.startswith("synthesize_long ") for k in runs) == 192
    rejected = {k: v for k, v in runs.items() if "error" in v}
    assert len(rejected) == 72 and all("delivery=ulaw24000" in k and "flac=none" not in k for k in rejected)
    assert all(v["error"] == ["ValueError", "flac needs delivery's encoding 's16', not 'ulaw'"] and v["names"] == "" for v in rejected.values())
    assert len(recorded["recorded_from"]) == 40 and os.path.getsize(FIXTURE) < 200_000
    seq = recorded["sequences"]
    assert seq["1 delivery setups"]["counts"]["ev_deliver_setup"] == 3
    assert seq["2 denoise setups and the measured bias"]["counts"] == dict(ev_deliver_setup=0, ev_denoise_setup=3, ev_denoise_bias=1)
    assert [s["error"][1] for s in seq["4 vocoder=False"]["steps"]] == ["%s needs the vocoder's waveform" % k for k in ("flac", "limiter", "loudness", "delivery", "denoise")]
    assert all(s["names"] == "" for s in seq["4 vocoder=False"]["steps"])


def test_the_product_is_the_recorded_one(recorded, recorder):
    got = recorder.product()
    assert list(got) == list(recorded["product"])
    wrong = [k for k in got if got[k] != recorded["product"][k]]
    assert not wrong, "%d of %d runs differ, the first: %s\n got %s\nwant %s" % (len(wrong), len(got), wrong[0], got[wrong[0]], recorded["product"][wrong[0]])


def test_the_sequences_are_the_recorded_ones(recorded, recorder):
    got = recorder.sequences()
    assert list(got) == list(recorded["sequences"])
    for title, want in recorded["sequences"].items():
        assert got[title]["counts"] == want["counts"], title
        for g, w in zip(got[title]["steps"], want["steps"]):
            assert g == w, "%s: %s" % (title, w["call"])
        assert len(got[title]["steps"]) == len(want["steps"])
