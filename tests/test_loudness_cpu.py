"""No GPU: the host side of the loudness stage (multilingual_kws_amd/loudness.py, include/mkws.h "Loudness and true peak").  The
K-weighting coefficients against the table of ITU-R BS.1770-4 and against the oracle (tests/util_loudness.py), every refusal of
mkws_loudness_create and of the wrapper before a device is looked for, and the oracle itself against the conformance signals of EBU
Tech 3341 (mono, at 16 kHz)."""
import ctypes

import numpy as np
import pytest

from multilingual_kws_amd import _lib, loudness, resample
from tests import util_loudness as ul

INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -3


def test_coeffs_match_bs1770_and_the_oracle():
    got = loudness.coeffs(48000)
    assert got.shape == (2, 5) and got.dtype == np.float64
    assert np.abs(got - ul.BS1770_48K).max() <= 1e-12
    assert np.abs(ul.k_coeffs(48000) - ul.BS1770_48K).max() <= 1e-12
    for rate in (16000, 8000, 44100):
        assert np.abs(loudness.coeffs(rate) - ul.k_coeffs(rate)).max() <= 1e-14, rate


def test_geometry_and_defaults():
    cfg = loudness.make_cfg(16000)
    assert (cfg.rate, cfg.mode, cfg.target_lufs, cfg.true_peak_db, cfg.headroom_db) == (16000, 0, -16.0, -1.5, 0.1)
    assert (cfg.zero_crossings, cfg.kaiser_beta, round(cfg.rolloff, 6)) == (32, 9.0, 0.95)
    for rate, chunk in ((16000, 32), (8000, 32), (48000, 32), (44100, 30), (10090, 1)):
        g = loudness.geometry(loudness.make_cfg(rate))
        assert g == dict(hop=rate // 10, block=4 * (rate // 10), chunk=chunk, tile=256 * chunk), (rate, g)
        assert g["hop"] % g["chunk"] == 0
    with pytest.raises(TypeError):
        loudness.make_cfg(16000, not_an_option=1)
    with pytest.raises(ValueError):
        loudness.make_cfg(16000, mode="rms")


def test_true_peak_taps_are_the_resamplers():
    """The oracle's restatement of the filter against the library's host table (L = 4, M = 1): equal to a float32 rounding."""
    tab = resample.host_taps(resample.make_cfg(1, 4))
    mine = ul.true_peak_taps()
    assert tab.shape == mine.shape == (65, 4)
    assert np.abs(tab.astype(np.float64) - mine.astype(np.float64)).max() <= 2.0 ** -24
    tab = resample.host_taps(resample.make_cfg(1, 4, zero_crossings=8, kaiser_beta=5.0, rolloff=0.9))
    assert np.abs(tab.astype(np.float64) - ul.true_peak_taps(8, 5.0, 0.9).astype(np.float64)).max() <= 2.0 ** -24


def _create(cfg, max_rows=4, max_samples=16000):
    h = ctypes.c_void_p()
    rc = _lib.lib().mkws_loudness_create(ctypes.byref(cfg), max_rows, max_samples, ctypes.byref(h))
    if h:
        _lib.lib().mkws_loudness_destroy(h)
    return rc


def test_create_refuses_before_it_looks_for_a_device():
    import torch
    L = _lib.lib()
    bad = [
        (dict(rate=0), INVALID), (dict(rate=-16000), INVALID), (dict(rate=16001), UNSUPPORTED), (dict(rate=44101), UNSUPPORTED),
        (dict(rate=3000), UNSUPPORTED), (dict(mode=2), INVALID), (dict(mode=-1), INVALID),
        (dict(target_lufs=float("nan")), INVALID), (dict(target_lufs=float("inf")), INVALID), (dict(true_peak_db=float("-inf")), INVALID),
        (dict(true_peak_db=float("nan")), INVALID), (dict(headroom_db=float("nan")), INVALID),
        (dict(zero_crossings=0), INVALID), (dict(zero_crossings=4096), UNSUPPORTED), (dict(rolloff=0.0), INVALID), (dict(rolloff=1.5), INVALID),
        (dict(kaiser_beta=-1.0), INVALID), (dict(kaiser_beta=float("nan")), INVALID),
    ]
    for over, code in bad:
        cfg = loudness.make_cfg(16000)
        for k, v in over.items():
            setattr(cfg, k, v)
        assert _create(cfg) == code, (over, L.mkws_last_error())
        out10, out4 = (ctypes.c_double * 10)(), (ctypes.c_int32 * 4)()
        assert L.mkws_loudness_coeffs(ctypes.byref(cfg), out10) == code and L.mkws_loudness_geometry(ctypes.byref(cfg), out4) == code, over
    cfg = loudness.make_cfg(16000)
    for rows, samples, code in ((0, 16000, INVALID), (-1, 16000, INVALID), (4, 0, INVALID), (4, -5, INVALID),
                                (1024, 1 << 33, UNSUPPORTED), (1 << 30, 1 << 20, UNSUPPORTED), (1, 1 << 45, UNSUPPORTED)):
        assert _create(cfg, rows, samples) == code, (rows, samples, L.mkws_last_error())
    h = ctypes.c_void_p()
    assert L.mkws_loudness_create(None, 4, 16000, ctypes.byref(h)) == INVALID and L.mkws_loudness_create(ctypes.byref(cfg), 4, 16000, None) == INVALID
    assert L.mkws_loudness_coeffs(ctypes.byref(cfg), None) == INVALID and L.mkws_loudness_geometry(ctypes.byref(cfg), None) == INVALID
    if not torch.cuda.is_available():          # what is left is a good configuration: only the device is missing
        assert _create(cfg) == NO_DEVICE
        assert _create(cfg, 1024, 16000) == NO_DEVICE and _create(cfg, 1, 16000 * 600) == NO_DEVICE


class _NoDevice:
    """Stands where the library stands in a meter: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} before it had accepted its arguments")


def _meter_without_device(max_rows=4, max_samples=1000):
    m = loudness.LoudnessMeter.__new__(loudness.LoudnessMeter)
    m.L, m.h, m.max_rows, m.max_samples = _NoDevice(), None, max_rows, max_samples
    return m


def test_wrapper_refuses_before_any_device_call():
    import torch
    m = _meter_without_device()
    good = np.zeros((2, 100), np.float32)
    for call in (m.measure, m.gains, m.normalize):
        with pytest.raises(TypeError):
            call(good.astype(np.float64))
        with pytest.raises(TypeError):
            call(good.astype(np.int32))
        with pytest.raises(ValueError):
            call(np.zeros((2, 3, 4), np.float32))
        with pytest.raises(ValueError):
            call(np.zeros((5, 100), np.float32))          # more rows than the workspace
        with pytest.raises(ValueError):
            call(np.zeros((2, 1001), np.float32))         # longer rows than the workspace
        for lengths in ([100], [100, 101], [-1, 5], [[1, 2]], np.array([1.0, 2.0]), torch.tensor([1, 2, 3])):
            with pytest.raises(ValueError):
                call(good, lengths=lengths)
    for out in (np.zeros((2, 100), np.float32), torch.zeros((2, 100)), torch.zeros((2, 100), dtype=torch.float64), torch.zeros((2, 100), device="meta")):
        with pytest.raises(ValueError):
            m.normalize(good, out=out)
    with pytest.raises(ValueError):
        loudness.LoudnessMeter(16000, mode="rms")
    with pytest.raises(TypeError):
        loudness.LoudnessMeter(16000, window=3)
    for kw in (dict(rate=16001), dict(target_lufs=float("nan")), dict(max_rows=0), dict(max_samples=0), dict(max_rows=1024, max_samples=1 << 33)):
        with pytest.raises(_lib.MkwsError) as e:
            loudness.LoudnessMeter(**kw)
        assert e.value.code in (INVALID, UNSUPPORTED), kw


def test_input_data_surface():
    import inspect
    from multilingual_kws.embedding import input_data as alias
    from multilingual_kws_amd.embedding import input_data
    assert alias is input_data
    assert list(inspect.signature(input_data.measure_loudness).parameters) == ["audio", "sample_rate", "lengths"]
    sig = inspect.signature(input_data.normalize_loudness)
    assert list(sig.parameters) == ["audio", "sample_rate", "target_lufs", "true_peak_db", "mode", "lengths"]
    assert [sig.parameters[k].default for k in ("sample_rate", "target_lufs", "true_peak_db", "mode", "lengths")] == [16000, -16.0, -1.5, "loudness", None]
    assert inspect.signature(input_data.read_clips).parameters["normalize"].default is None
    with pytest.raises(ValueError):
        input_data.read_clips([], normalize={"loudness": -16})
    with pytest.raises(ValueError):
        input_data.read_clips([], normalize="loudness")


@pytest.mark.parametrize("name", ["tech3341_case3", "tech3341_case4", "tech3341_case5", "sine_997_0dbfs"])
def test_oracle_reads_the_conformance_signals(name):
    """EBU Tech 3341 at 16 kHz, one channel: the stereo reading less 3.01 LU, within +-0.1 LU."""
    x, want = ul.conformance_signals(16000)[name]
    m = ul.measure(x, 16000, peaks=False)
    assert abs(m["loudness"] - want) <= 0.1, (name, m)
    if name == "tech3341_case4":
        assert m["absolute"] < m["blocks"] and m["relative"] < m["absolute"]      # the -72 dBFS parts fall to the absolute gate, the -36 ones to the relative


def test_oracle_sine_at_48k_and_true_peaks():
    x = ul.steps(48000, 997.0, [(0.0, 5.0)])
    m = ul.measure(x, 48000)
    assert abs(m["loudness"] - (-3.01)) <= 0.01 and m["blocks"] == 47 == m["absolute"] == m["relative"]
    for amp, div, phase, want in ul.TRUE_PEAK_CASES:
        tp, bound = ul.true_peak(ul.true_peak_signal(amp, div, phase), ul.true_peak_taps())
        db = 20.0 * np.log10(tp)
        assert want - 0.4 <= db <= want + 0.2 and bound < 1e-5, (amp, div, phase, db)


def test_oracle_gain_rules():
    m = dict(loudness=-30.0, true_peak=0.1, sample_peak=0.09)
    g, flags = ul.gain_of(m)
    assert flags == 0 and g == np.float32(10.0 ** (14.0 / 20.0))
    g, flags = ul.gain_of(dict(m, true_peak=0.5))
    assert flags == ul.FLAG_PEAK_LIMITED and g == np.float32(10.0 ** (-1.5 / 20.0) / 0.5)
    assert ul.gain_of(dict(m, loudness=-np.inf)) == (np.float32(1.0), ul.FLAG_UNMEASURED)
    assert ul.gain_of(m, mode="peak") == (np.float32(10.0 ** (-0.1 / 20.0) / 0.09), 0)
    assert ul.gain_of(dict(m, sample_peak=0.0), mode="peak") == (np.float32(1.0), ul.FLAG_UNMEASURED)
    short = ul.measure(ul.ramp_noise(6399, 16000, 1), 16000)
    assert short["blocks"] == 0 and short["loudness"] == -np.inf
    both = ul.measure(ul.ramp_noise(80000, 16000, 2), 16000)
    assert both["blocks"] == 47 and both["absolute"] < both["blocks"] and 0 < both["relative"] < both["absolute"]
