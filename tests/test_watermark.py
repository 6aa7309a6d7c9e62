"""The watermark scheme on the CPU, with tests/watermark_oracle.py alone: the pattern (also against the library's host function), embed -> detect
on the two 4 s fixtures, wrong key, unmarked input, a front cut, 1000 random keys, survival through the project's own chain as its oracles state
it (loudness gain -> limiter -> 8 kHz mu-law -> G.711 decode -> back to 16 kHz), an 8-bit payload, and negative controls.  z must reach 1.25 x
the threshold wherever the mark is claimed present."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import deliver_oracle as dl
import denoise_oracle as do
import limit_oracle as lim
import loudness_oracle as lo
import resample_oracle as ro
import watermark_oracle as wo
from conftest import GOLDEN_DIR

SR, KEY = 16000, 0x5EED1234
MARGIN = 1.25 * wo.THRESHOLD
FIXTURES = {"speech_like": lambda n: wo.speech_like(3, n), "harmonic_rich": lambda n: wo.harmonic_rich(3, n)}
_CACHE = {}


def _plain(name, seconds=4):
    if (name, seconds) not in _CACHE:
        _CACHE[name, seconds] = FIXTURES[name](seconds * SR)
    return _CACHE[name, seconds]


def _marked(name, seconds=4, nbits=0, payload=0):
    k = (name, seconds, nbits, payload, "marked")
    if k not in _CACHE:
        _CACHE[k] = wo.embed64(_plain(name, seconds), KEY, nbits, payload, 1.0).astype(np.float32)
    return _CACHE[k]


def test_pattern_balance_roles_and_payload_flips():
    signs, roles = wo.pattern(KEY)
    assert signs.shape == roles.shape == (768,) and set(np.unique(signs)) == {-1, 1} and np.all(roles == wo.PILOT)
    for key in (0, 1, KEY, 0xFFFFFFFF):
        s, _ = wo.pattern(key)
        assert abs(int(s.sum())) <= 111      # 4 sigma of 768 fair signs
    assert not np.array_equal(wo.pattern(1)[0], wo.pattern(2)[0])
    base, roles = wo.pattern(KEY, 8, 0)
    assert np.array_equal(base, signs)       # payload 0 flips nothing; the roles do not touch the signs
    carried = roles != wo.PILOT
    assert set(np.unique(roles[carried])) == set(range(8)) and 300 <= carried.sum() <= 468      # half of 768, 4.5 sigma
    assert all(18 <= (roles == b).sum() <= 78 for b in range(8))      # 768 / 16 = 48 each, sigma 6.7: 4.5 sigma
    flipped, roles2 = wo.pattern(KEY, 8, 0b10100101)
    assert np.array_equal(roles, roles2)
    want = np.isin(roles, [0, 2, 5, 7])
    assert np.array_equal(flipped != base, want) and np.array_equal(flipped[~want], base[~want])
    _, r16 = wo.pattern(KEY, 16, 0)
    assert set(np.unique(r16[r16 != wo.PILOT])) == set(range(16))


def test_pattern_is_the_library_s():
    from emotivoice_amd import _ffi
    lib = _ffi.lib()
    for key, nbits, payload in ((KEY, 0, 0), (7, 8, 0xA5), (0xFFFFFFFF, 16, 0xBEEF), (0, 1, 1)):
        got = np.zeros(768, np.int8)
        assert lib.ev_watermark_pattern(C.c_uint32(key), nbits, C.c_uint32(payload), got.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(got, wo.pattern(key, nbits, payload)[0]), (key, nbits, payload)
    got = np.zeros(768, np.int8)
    for bad in ((1, 17, 0), (1, -1, 0), (1, 4, 16), (1, 0, 1)):
        assert lib.ev_watermark_pattern(C.c_uint32(bad[0]), bad[1], C.c_uint32(bad[2]), got.ctypes.data_as(C.c_void_p)) == -1
    assert lib.ev_watermark_pattern(C.c_uint32(1), 0, C.c_uint32(0), None) == -1


def test_strength_zero_is_denoise_at_strength_zero():
    w = _plain("speech_like")[:8192]
    assert np.array_equal(wo.embed64(w, KEY, strength_db=0.0), do.denoise64(w, np.ones(513, np.float32), 0.0))


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_embed_then_detect_on_the_four_second_fixtures(name):
    y = _marked(name)
    d = wo.detect(y, KEY)
    print(name, "z %.2f offset %d n %d" % (d["z"], d["offset"], d["n"]))
    assert d["present"] and d["z"] >= MARGIN and d["offset"] == 0
    wrong = wo.detect(y, KEY ^ 0x1111)
    plain = wo.detect(_plain(name), KEY)
    print(name, "wrong key z %.2f, unmarked z %.2f" % (wrong["z"], plain["z"]))
    assert not wrong["present"] and not plain["present"]
    x = _plain(name)[:y.size].astype(np.float64)
    snr = 10 * np.log10((x ** 2).sum() / ((y - x) ** 2).sum())
    print(name, "SNR %.1f dB" % snr)
    assert 20.0 < snr < 40.0      # a 1 dB mark on a third of the band: neither inaudibly small by construction nor a different signal


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_offset_after_a_front_cut(name):
    """1000 samples are 4 frames less 24 samples: the pattern's tile 0 then starts 4 frames before the recording does, at offset 124 of 128."""
    d = wo.detect(_marked(name)[1000:], KEY)
    print(name, "z %.2f offset %d" % (d["z"], d["offset"]))
    assert d["present"] and d["z"] >= MARGIN and d["offset"] == 124


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_a_thousand_random_keys_on_the_unmarked_fixture(name):
    folded = wo.fold(wo.band_q(_plain(name))[0])
    keys = np.random.default_rng(11).integers(0, 2 ** 32, 1000, dtype=np.uint64)
    z = np.array([wo.correlate(folded, int(k))["z"] for k in keys])
    print(name, "largest z over 1000 keys %.2f" % z.max())
    assert z.max() < wo.THRESHOLD


def _through_the_chain(y):
    """loudness to -16 LUFS as a pre-gain -> limiter -> 8 kHz mu-law -> G.711 decode -> 16 kHz, each by the stage's own oracle."""
    from emotivoice_amd.limiter import pre_gain
    from emotivoice_amd.loudness import LoudnessConfig
    g, _ = pre_gain(lo.measure(y, SR)["loudness"], LoudnessConfig(target_lufs=-16.0).validate())
    limited = lim.limit(y, gain_in=g)["wav"]
    law = dl.deliver(limited, SR, 8000, dl.ULAW)["data"]
    back = wo.ulaw_decode(law)
    h, up, down, _ = ro.design(8000, SR)
    return ro.resample32(back, h, up, down)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_mark_survives_the_project_s_own_chain(name):
    z = _through_the_chain(_marked(name))
    d = wo.detect(z, KEY)
    print(name, "after the chain: z %.2f offset %d" % (d["z"], d["offset"]))
    assert d["present"] and d["z"] >= MARGIN and d["offset"] == 0
    assert not wo.detect(_through_the_chain(_plain(name)), KEY)["present"]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_an_eight_bit_payload_from_sixteen_seconds(name):
    payload = 0xA5
    d = wo.detect(_marked(name, 16, 8, payload), KEY, 8)
    print(name, "z %.2f payload %#x bit_C %s" % (d["z"], d["payload"], d["bit_C"][:8].tolist()))
    assert d["present"] and d["z"] >= MARGIN and d["payload"] == payload and d["offset"] == 0
    assert np.all(d["bit_C"][8:] == 0) and np.all(d["bit_n"][8:] == 0)


def _embed_bar():
    """The whole-call bar of tests/test_gpu_denoise.py, 4 x the reference's own float32 error recorded in tests/golden, times the largest gain."""
    errs = [float(np.load(p)["ref_err"]) for p in glob.glob(os.path.join(GOLDEN_DIR, "denoise", "dn_[a-h]_*.npz"))]
    assert len(errs) == 8
    return 4 * max(errs) * float(wo.gains_f32(1.0)[0])


@pytest.mark.parametrize("wrong", (dict(invert_band=17), dict(tile_shift=1)))
def test_negative_controls_fail_the_embed_bar(wrong):
    """An embed with one band's chips inverted, or with u off by one tile, is further from the right one than the bar the device is held to:
    that bar sees either mistake.  The tile shift also moves the reported offset by a tile."""
    w = _plain("speech_like")
    e = do.peak_error(wo.embed64(w, KEY, **wrong), _marked("speech_like").astype(np.float64))
    print(wrong, "E %.3e bar %.3e" % (e, _embed_bar()))
    assert e > 100 * _embed_bar()
    if "tile_shift" in wrong:
        # tile 0 of the shifted pattern starts at frame -8: offset 120, give or take the one frame by which neighbouring offsets, which share
        # seven of a tile's eight frames, can tie
        assert abs(wo.detect(wo.embed64(w, KEY, **wrong).astype(np.float32), KEY)["offset"] - 120) <= 1


def test_negative_control_a_detector_with_the_wrong_tile_loses_the_mark():
    """A detector whose chips sit one band off (v + 1 for v) or that reads the tiles of another key's pattern sees nothing."""
    folded = wo.fold(wo.band_q(_marked("speech_like"))[0])
    shifted = dict(folded, F=np.roll(folded["F"], 1, axis=2), A=np.roll(folded["A"], 1, axis=2))
    assert wo.correlate(folded, KEY)["present"] and not wo.correlate(shifted, KEY)["present"]


def test_config_and_report():
    from emotivoice_amd.watermark import WatermarkConfig, detect_report, parse_flag, watermark_config
    assert watermark_config(None) is None and watermark_config(7).key == 7
    c = parse_flag("0x10:5:8")
    assert (c.key, c.payload, c.nbits) == (16, 5, 8) and watermark_config("9").nbits == 0
    p, n, s = WatermarkConfig(key=1, payload=[1, 0, 3], nbits=[1, 0, 2], strength_db=[0.5, 1.0, 2.0]).validate().per_segment(3)
    assert p.tolist() == [1, 0, 3] and n.tolist() == [1, 0, 2] and s.dtype == np.float32
    for bad in (dict(key=-1), dict(key=1, nbits=17), dict(key=1, nbits=2, payload=4), dict(key=1, strength_db=7.0), dict(key=1, strength_db=float("nan")),
                dict(key=2 ** 32), dict(key=1, payload=[0, 0], nbits=[0, 0, 0])):
        with pytest.raises(ValueError):
            WatermarkConfig(**bad).validate()
    with pytest.raises(ValueError):
        parse_flag("1:2")
    with pytest.raises(ValueError):
        WatermarkConfig(key=1, nbits=[0, 0]).validate().per_segment(3)
    d = wo.detect(_marked("speech_like"), KEY)
    rep = detect_report(dict(C=[d["C"], 0], n=[d["n"], 0], offset=[d["offset"], 0], bit_C=np.zeros((2, 16), np.int32), bit_n=np.zeros((2, 16), np.int32)))
    assert rep[0]["present"] and abs(rep[0]["z"] - d["z"]) < 1e-12 and rep[1] == dict(z=0.0, present=False, offset=0, bits=[], payload=0, bit_z=[])
