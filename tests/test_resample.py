"""ev_resample's host side: the oracle of the specification against scipy, the library's filter design against the Python one, what the filter
does to tones, ResampleConfig's rejections, lengths and the time offset.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import resample_oracle as ro

PAIRS = [(48000, 16000), (44100, 16000), (22050, 16000), (24000, 16000), (8000, 16000), (16000, 24000)]


def test_oracle_equals_scipy_resample_poly():
    """The direct float64 sum is scipy.signal.resample_poly(x, up, down, window=h / up) to 1e-12, with equal lengths."""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(0)
    for sr_in, sr_out in PAIRS:
        h, up, down, half = ro.design(sr_in, sr_out)
        x = rng.uniform(-1.0, 1.0, 3001).astype(np.float32)
        y = ro.resample64(x, h, up, down)
        want = signal.resample_poly(x.astype(np.float64), up, down, window=h.astype(np.float64) / up)
        assert y.size == want.size == ro.output_len(x.size, up, down), (sr_in, sr_out)
        err = np.abs(y - want).max()
        print(sr_in, sr_out, "up %d down %d half %d  max |oracle - scipy| %.2e" % (up, down, half, err))
        assert err <= 1e-12, (sr_in, sr_out, err)


def test_float32_oracle_stays_within_the_accumulation_bound():
    rng = np.random.default_rng(1)
    for sr_in, sr_out in ((44100, 16000), (8000, 16000)):
        h, up, down, half = ro.design(sr_in, sr_out)
        x = rng.uniform(-1.0, 1.0, 2000).astype(np.float32)
        bound = ro.accumulation_bound(h, up, ro.taps_per_output(h, up), np.abs(x).max())
        err = np.abs(ro.resample32(x, h, up, down).astype(np.float64) - ro.resample64(x, h, up, down)).max()
        print(sr_in, sr_out, "E(f32) %.2e bound %.2e" % (err, bound))
        assert err <= bound


def test_library_design_equals_the_python_design():
    """ev_resample_design touches no device: half_len exactly, every tap within one float32 ulp, and the negative size for a small cap."""
    from emotivoice_amd import _ffi
    from emotivoice_amd.resample import ResampleConfig
    lib = _ffi.lib()
    for sr_in, sr_out in ((44100, 16000), (48000, 16000), (8000, 16000)):
        cfg = ResampleConfig(sr_in=sr_in, sr_out=sr_out)
        want = cfg.design()
        assert np.array_equal(want, ro.design(sr_in, sr_out)[0])
        n = want.size
        assert lib.ev_resample_design(sr_in, sr_out, 16, 0.945, 9.0, None, 0) == -n
        small = np.zeros(n - 1, np.float32)
        assert lib.ev_resample_design(sr_in, sr_out, 16, 0.945, 9.0, small.ctypes.data_as(C.c_void_p), n - 1) == -n and not small.any()
        got = np.zeros(n, np.float32)
        assert lib.ev_resample_design(sr_in, sr_out, 16, 0.945, 9.0, got.ctypes.data_as(C.c_void_p), n) == cfg.half_len() == (n - 1) // 2
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
        worst = (np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp).max()
        print(sr_in, sr_out, "taps %d worst %.2f ulp, equal %d" % (n, worst, int((got == want).sum())))
        assert worst <= 1.0
        assert abs(float(got.astype(np.float64).sum()) - cfg.ratio()[0]) <= 1e-4          # unit gain at DC
    other = ResampleConfig(sr_in=22050, sr_out=16000, zeros=8, rolloff=0.9, beta=6.0)
    got = np.zeros(2 * other.half_len() + 1, np.float32)
    assert lib.ev_resample_design(22050, 16000, 8, 0.9, 6.0, got.ctypes.data_as(C.c_void_p), got.size) == 8 * 441
    assert (np.abs(got.astype(np.float64) - other.design()) <= np.spacing(np.maximum(np.abs(got), np.abs(other.design())))).all()
    for bad in ((0, 16000, 16, 0.945, 9.0), (16000, 16001, 16, 0.945, 9.0), (44100, 16000, 0, 0.945, 9.0), (44100, 16000, 16, 0.0, 9.0),
                (44100, 16000, 16, 0.945, float("nan"))):
        assert lib.ev_resample_design(*bad, None, 0) == 0, bad


def test_tones_pass_and_aliases_are_suppressed():
    """0.5 s tones at unit amplitude, RMS over the middle half of the output: 1 kHz keeps its RMS within 1e-4 relative, 8960 Hz (which would
    alias to 7040 Hz) comes out at <= 2e-4 of the input's."""
    for sr_in in (48000, 44100):
        h, up, down, half = ro.design(sr_in, 16000)
        rms = {}
        for f in (1000.0, 8960.0):
            x = ro.tone(f, sr_in, 0.5)
            y = ro.resample64(x, h, up, down)
            mid = y[y.size // 4:y.size - y.size // 4]
            xin = x.astype(np.float64)[x.size // 4:x.size - x.size // 4]
            rms[f] = (np.sqrt((mid ** 2).mean()), np.sqrt((xin ** 2).mean()))
        print(sr_in, "1 kHz RMS %.6f (in %.6f), 8960 Hz RMS %.3e" % (rms[1000.0][0], rms[1000.0][1], rms[8960.0][0]))
        assert abs(rms[1000.0][0] - rms[1000.0][1]) <= 1e-4 * rms[1000.0][1]
        assert rms[8960.0][0] <= 2e-4 * rms[8960.0][1]


def test_validate_names_the_rejected_field():
    from emotivoice_amd.resample import ResampleConfig
    nan = float("nan")
    for kw, needle in ((dict(sr_in=0), "sr_in"), (dict(sr_in=44100, sr_out=0), "sr_out"), (dict(sr_in=16001), "EV_RESAMPLE_MAX_RATIO"),
                       (dict(sr_in=44100, sr_out=44099), "EV_RESAMPLE_MAX_RATIO"), (dict(taps=np.zeros(1, np.float32)), "taps"),
                       (dict(taps=np.zeros(4, np.float32)), "taps"), (dict(taps=np.zeros(32771, np.float32)), "EV_RESAMPLE_MAX_TAPS"),
                       (dict(taps=np.array([0.0, nan, 0.0], np.float32)), "taps"), (dict(sr_in=48000, sr_out=1000, zeros=512), "EV_RESAMPLE_MAX_TAPS"),
                       (dict(zeros=0), "zeros"), (dict(rolloff=0.0), "rolloff"), (dict(rolloff=1.5), "rolloff"), (dict(beta=-1.0), "beta"),
                       (dict(beta=nan), "beta"), (dict(trim=True, trim_frac=0.0), "trim_frac"), (dict(trim=True, trim_frac=1.0), "trim_frac"),
                       (dict(trim=True, trim_frac=nan), "trim_frac"), (dict(trim=True, trim_pad=-1), "trim_pad")):
        with pytest.raises(ValueError) as e:
            ResampleConfig(**kw).validate()
        assert needle in str(e.value), (kw, str(e.value))
    ok = ResampleConfig(sr_in=44100, trim=True).validate()
    assert ok.ratio() == (160, 441) and ok.pad() == 800 and ok.half_len() == 16 * 441 and ok.is_default_design()
    assert ResampleConfig(sr_in=44100, trim_frac=nan).validate() is not None          # without trim the trim fields are not looked at
    assert ResampleConfig(sr_in=44100).key() != ResampleConfig(sr_in=44100, trim=True).key()
    assert ResampleConfig(sr_in=8000, taps=np.ones(5, np.float32)).key() == ResampleConfig(sr_in=8000, taps=np.ones(5)).key()


def test_output_len_and_packing():
    from emotivoice_amd.resample import MAX_OUT, ResampleConfig, pack_wavs
    for sr_in, sr_out in PAIRS + [(11025, 16000)]:
        cfg = ResampleConfig(sr_in=sr_in, sr_out=sr_out)
        up, down = cfg.ratio()
        for L in (1, 2, 3, down, down + 1, 4409, 100003):
            assert cfg.output_len(L) == ro.output_len(L, up, down) == int(np.ceil(L * up / down - 1e-9)), (sr_in, L)
    assert ResampleConfig(sr_in=48000).output_len(3) == 1 and ResampleConfig(sr_in=48000).output_len(4) == 2
    assert ResampleConfig(sr_in=8000).output_len(1) == 2
    flat, is16, lens = pack_wavs([np.zeros(1, np.float64), np.ones(3, np.float32)])
    assert flat.dtype == np.float32 and not is16 and lens.tolist() == [1, 3] and flat.tolist() == [0.0, 1.0, 1.0, 1.0]
    flat, is16, lens = pack_wavs([np.ones(2, np.int16)])
    assert flat.dtype == np.int16 and is16
    for wavs, needle in (([], "no utterances"), ([np.zeros(0, np.float32)], "wavs[0]"), ([np.zeros(2, np.float32), np.zeros(2, np.int16)], "wavs[1]"),
                         ([np.zeros(2, np.int32)], "int16 or floating")):
        with pytest.raises(ValueError) as e:
            pack_wavs(wavs)
        assert needle in str(e.value)
    big = np.broadcast_to(np.float32(0.0), (MAX_OUT * 3 + 1,))
    with pytest.raises(ValueError) as e:
        pack_wavs([big], ResampleConfig(sr_in=48000))
    assert "EV_ALIGN_MAX_FRAMES" in str(e.value)


def test_phase_table_rows_are_the_taps_in_the_order_k_ascends():
    from emotivoice_amd.resample import phase_table
    for up, half in ((1, 4), (3, 7), (4, 8), (5, 2), (160, 7056)):
        h = np.arange(1, 2 * half + 2, dtype=np.float32)            # h[i] = i + half + 1: every tap its own value
        tab = phase_table(h, up)
        assert tab.shape == (up, ((2 * half) // up + 1) | 1)
        seen = []
        for p in range(up):
            i = [int(v) - half - 1 for v in tab[p] if v != 0]
            assert i and all(ii % up == p for ii in i) and i == sorted(i, reverse=True) and i[0] + up > half and i[-1] - up < -half
            seen += i
        assert sorted(seen) == list(range(-half, half + 1))


def test_time_offset_arithmetic():
    """Output sample j of a trimmed utterance is resampled sample trim_start - trim_pad + j."""
    from emotivoice_amd.alignment import timestamps
    from emotivoice_amd.resample import time_offset_s
    assert time_offset_s(4800, 800, 16000) == 0.25
    assert time_offset_s(0, 800, 16000) == -0.05
    assert time_offset_s(123, 0, 16000) == 123 / 16000
    y = np.zeros(16000, np.float32)
    y[4800:9000] = 0.5
    out, start, end = ro.trim(y, 0.005, 800)
    assert (start, end) == (4800, 8999) and out.size == end - start + 1600
    off = time_offset_s(start, 800, 16000)
    j = 800                                                        # the first kept sample on the trimmed clock
    assert abs((j / 16000 + off) - 4800 / 16000) < 1e-12
    (a, b), = timestamps([10])
    assert abs((a + off) - (start - 800) / 16000) < 1e-12 and abs((b + off) - (start - 800 + 2560) / 16000) < 1e-12
