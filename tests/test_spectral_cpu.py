"""The mfcc / average feature modes without a GPU: the float64 reference of tests/spectral_cases.py against TensorFlow's own known answers,
the library's host tables against that reference, every refusal, the wrappers' pure checks, the dispatcher, and the measured tolerances
the GPU tests hold the device to."""
import ctypes

import numpy as np
import pytest

from multilingual_kws_amd import _lib, spectral
from multilingual_kws_amd.embedding import input_data, live
from tests import spectral_cases as sc

torch = pytest.importorskip("torch")


# ---- the reference against TensorFlow's known answers -------------------------------------------------------------------------------
def test_reference_mfcc_known_answer():
    """TF mfcc_test.cc: 513 bins, power[i] = i + 1, 22050 Hz, 40 channels over 20-4000 Hz, 13 coefficients."""
    want = [29.13970072, -6.41568601, -0.61903012, -0.96778652, -0.26819878, -0.40907028, -0.15614748, -0.23203119, -0.10481487, -0.1543029,
            -0.0769791, -0.10806114, -0.06047613]
    got = sc.ref_mfcc(np.arange(1, 514, dtype=np.float64), 22050, 13)
    assert np.abs(got - want).max() < 5e-9, got


def test_reference_spectrogram_known_answer():
    """TF spectrogram_op_test.cc: window 8, stride 1; a symmetric Hann window does not give these integers."""
    got = sc.ref_power(np.asarray([[1, 0, -1, 0, 1, 0, -1, 0]], dtype=np.float64), 8, 1)
    assert got.shape == (1, 1, 5) and np.abs(got[0, 0] - [0, 1, 4, 1, 0]).max() < 1e-12
    assert np.abs(np.sqrt(got[0, 0]) - [0, 1, 2, 1, 0]).max() < 1e-12


def test_reference_silence_is_the_features_minimum():
    got = sc.ref_mfcc(np.zeros(257), 16000, 40)
    assert abs(got[0] - np.sqrt(2 / 40) * 40 * np.log(1e-12)) < 1e-9 and abs(got[0] + 247.139) < 1e-3 and np.abs(got[1:]).max() < 1e-9
    assert input_data.get_features_range(dict(preprocess="mfcc"))[0] == -247.0


def test_average_settings_give_43_outputs_the_last_of_five_bins():
    ms = input_data.prepare_model_settings(3, 16000, 1000, 30, 20, 40, "average")
    assert ms["average_window_width"] == 6 and ms["fingerprint_width"] == 43
    power = np.random.default_rng(0).uniform(0, 1, (2, 257))
    got = sc.ref_average(power, 6)
    assert got.shape == (2, 43) and np.allclose(got[:, 42], power[:, 252:257].mean(axis=1)) and np.allclose(got[:, 0], power[:, :6].mean(axis=1))
    assert spectral.geometry(spectral.make_cfg(mode="average", average_window_width=6, num_features=43)) == (512, 257, 43)


# ---- host side -----------------------------------------------------------------------------------------------------------------------
def _one_rounding(got, want):
    """got (float32) is within one float rounding of the float64 value"""
    return bool(np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)))


@pytest.mark.parametrize("mode", ["mfcc40", "mfcc13", "mfcc1"])
@pytest.mark.parametrize("geometry", list(sc.GEOMETRIES))
def test_host_tables_match_the_reference(geometry, mode):
    over = sc.cfg_of(geometry, mode)
    cfg = spectral.make_cfg(**over)
    sr, window, stride = sc.GEOMETRIES[geometry]
    fft, bins, width = spectral.geometry(cfg)
    assert (fft, bins, width) == (sc.next_pow2(window), sc.next_pow2(window) // 2 + 1, over["num_features"])
    weights, band, start, end = sc.mel_tables(bins, sr, 40, 20.0, 4000.0)
    assert spectral.host_scalars(cfg) == dict(window=window, stride=stride, fft_size=fft, bins=bins, width=width, channels=40, start_index=start, end_index=end)
    assert _one_rounding(spectral.host_table(cfg, "window"), sc.hann_periodic(window))
    assert _one_rounding(spectral.host_table(cfg, "mel_weights"), weights)
    assert np.array_equal(spectral.host_table(cfg, "band_mapper"), band)
    assert _one_rounding(spectral.host_table(cfg, "dct").reshape(width, 40), sc.dct_matrix(width, 40))


@pytest.mark.parametrize("geometry", list(sc.GEOMETRIES))
def test_host_tables_average_mode(geometry):
    for mode in ("avg6", "avg1", "avgall"):
        over = sc.cfg_of(geometry, mode)
        cfg = spectral.make_cfg(**over)
        fft, bins, width = spectral.geometry(cfg)
        assert width == over["num_features"] == -(-bins // over["average_window_width"])
        assert _one_rounding(spectral.host_table(cfg, "window"), sc.hann_periodic(over["window_size_samples"]))
        for name in ("mel_weights", "band_mapper", "dct"):
            with pytest.raises(_lib.MkwsError, match="mfcc mode only"):
                spectral.host_table(cfg, name)


def test_num_frames():
    cfg = spectral.make_cfg()
    assert [spectral.num_frames(cfg, n) for n in (0, 479, 480, 799, 800, 16000, 16001)] == [0, 0, 1, 1, 2, 49, 49]
    cfg = spectral.make_cfg(window_size_samples=129, window_stride_samples=64)
    assert [spectral.num_frames(cfg, n) for n in (128, 129, 192, 193)] == [0, 1, 1, 2]


REFUSALS = [
    (dict(sample_rate=0), -1, "sample_rate"),
    (dict(window_size_samples=0), -1, "window_size_samples"),
    (dict(window_size_samples=128), -2, "window_size_samples"),
    (dict(window_size_samples=1025), -2, "window_size_samples"),
    (dict(window_stride_samples=0), -1, "window_stride_samples"),
    (dict(mode=2), -1, "mode"),
    (dict(num_features=0), -1, "num_features"),
    (dict(num_features=41), -1, "num_features"),
    (dict(filterbank_channels=0, num_features=0), -1, "filterbank_channels"),
    (dict(filterbank_channels=65, num_features=65), -2, "filterbank_channels"),
    (dict(lower_frequency_limit=-1.0), -1, "lower_frequency_limit"),
    (dict(lower_frequency_limit=float("nan")), -1, "lower_frequency_limit"),
    (dict(lower_frequency_limit=4000.0), -1, "upper_frequency_limit"),
    (dict(upper_frequency_limit=8000.5), -1, "upper_frequency_limit"),
    (dict(mode="average", average_window_width=0, num_features=257), -1, "average_window_width"),
    (dict(mode="average", average_window_width=6, num_features=42), -1, "num_features"),
]


@pytest.mark.parametrize("over,code,field", REFUSALS)
def test_every_refusal_names_its_field(over, code, field):
    cfg = spectral.make_cfg(**over)
    L = _lib.lib()
    h = ctypes.c_void_p()
    for call in (lambda: L.mkws_spectral_geometry(ctypes.byref(cfg), None, None, None),
                 lambda: L.mkws_spectral_host_table(ctypes.byref(cfg), 0, None, 0),
                 lambda: L.mkws_spectral_create(ctypes.byref(cfg), 16000, ctypes.byref(h))):      # decided on the host, before a device is looked for
        assert call() == code
        assert field in L.mkws_last_error().decode(), L.mkws_last_error()
    assert h.value is None


def test_accepted_edges_of_the_geometry():
    for over in (dict(window_size_samples=129), dict(window_size_samples=1024), dict(num_features=1), dict(filterbank_channels=64, num_features=64),
                 dict(lower_frequency_limit=0.0), dict(upper_frequency_limit=8000.0), dict(mode="average", average_window_width=300, num_features=1)):
        spectral.geometry(spectral.make_cfg(**over))
    with pytest.raises(TypeError):
        spectral.make_cfg(not_an_option=1)
    with pytest.raises(ValueError):
        spectral.make_cfg(mode="micro")


def test_create_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib.lib()
    h = ctypes.c_void_p()
    cfg = spectral.make_cfg()
    assert L.mkws_spectral_create(ctypes.byref(cfg), 16000, ctypes.byref(h)) == -3       # MKWS_ERR_NO_DEVICE
    assert b"no HIP device" in L.mkws_last_error() and h.value is None
    with pytest.raises(_lib.MkwsError):
        spectral.SpectralFrontend()


# ---- the wrappers' pure checks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_check_forward(device):
    dev = torch.device(device)
    cfg = spectral.make_cfg()
    mk = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    assert spectral.check_forward(cfg, dev, mk(3, 16000)) == (3, 16000, 49)
    assert spectral.check_forward(cfg, dev, mk(16001, dtype=torch.int16), max_samples=16001) == (1, 16001, 49)
    assert spectral.check_forward(cfg, dev, mk(0, 16000)) == (0, 16000, 49)
    assert spectral.check_forward(cfg, dev, mk(2, 479)) == (2, 479, 0)
    assert spectral.check_forward(cfg, dev, mk(3, 32000)[:, ::2]) == (3, 16000, 49)              # a strided view is made contiguous by the wrapper
    assert spectral.check_forward(cfg, dev, mk(3, 16000), out=mk(5, 49, 40)) == (3, 16000, 49)  # rows to spare
    with pytest.raises(ValueError, match="audio"):
        spectral.check_forward(cfg, dev, mk(1, 3, 16000))
    with pytest.raises(ValueError, match="audio"):
        spectral.check_forward(cfg, torch.device("cuda", 0), mk(3, 16000))
    with pytest.raises(ValueError, match="audio"):
        spectral.check_forward(cfg, dev, np.zeros((3, 16000), np.float32))
    with pytest.raises(TypeError, match="audio"):
        spectral.check_forward(cfg, dev, mk(3, 16000, dtype=torch.float64))
    with pytest.raises(ValueError, match="audio.*max_samples"):
        spectral.check_forward(cfg, dev, mk(3, 16001), max_samples=16000)
    for bad in (mk(2, 49, 40), mk(3, 49, 41), mk(3, 48, 40), mk(3, 49, 40, dtype=torch.float64), mk(3, 49, 80)[:, :, ::2], mk(3, 49 * 40)):
        with pytest.raises(ValueError, match="out"):
            spectral.check_forward(cfg, dev, mk(3, 16000), out=bad)
    with pytest.raises(ValueError, match="out"):
        spectral.check_forward(cfg, dev, mk(3, 16000), out=torch.empty((3, 49, 40), device="meta" if device == "cpu" else "cpu"))


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_check_stream(device):
    dev = torch.device(device)
    cfg = spectral.make_cfg()
    mk = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    assert spectral.check_stream(cfg, dev, mk(48000), 16000, 320) == (48000, 49, 101)
    assert spectral.check_stream(cfg, dev, mk(48000), 16000, 640) == (48000, 49, 51)
    assert spectral.check_stream(cfg, dev, mk(15999), 16000, 320) == (15999, 49, 0)
    assert spectral.check_stream(cfg, dev, mk(96000)[::2], 16000, 320) == (48000, 49, 101)
    for bad in (mk(1, 48000), mk(48000, dtype=torch.int16), np.zeros(48000, np.float32)):
        with pytest.raises(ValueError, match="audio"):
            spectral.check_stream(cfg, dev, bad, 16000, 320)
    with pytest.raises(ValueError, match="audio"):
        spectral.check_stream(cfg, torch.device("cuda", 0), mk(48000), 16000, 320)
    with pytest.raises(ValueError, match="audio.*max_samples"):
        spectral.check_stream(cfg, dev, mk(48000), 16000, 320, max_samples=47999)
    with pytest.raises(ValueError, match="window_samples"):
        spectral.check_stream(cfg, dev, mk(48000), 0, 320)
    for hop in (0, -320, 321, 160):
        with pytest.raises(ValueError, match="hop_samples"):
            spectral.check_stream(cfg, dev, mk(48000), 16000, hop)


# ---- the dispatcher ------------------------------------------------------------------------------------------------------------------
def test_to_features_micro_is_to_micro_spectrogram(monkeypatch):
    calls = []
    marker = object()
    monkeypatch.setattr(input_data, "to_micro_spectrogram", lambda *a, **k: (calls.append((a, k)), marker)[1])
    ms = input_data.standard_microspeech_model_settings(3)
    audio = np.zeros(16000, np.float32)
    assert input_data.to_features(ms, audio) is marker
    assert len(calls) == 1 and calls[0][0][0] is ms and calls[0][0][1] is audio and calls[0][1] == {}
    with pytest.raises(ValueError, match="preprocess"):
        input_data.to_features(dict(ms, preprocess="fft"), audio)
    assert calls == calls[:1]


def test_get_features_range():
    rng = lambda mode: input_data.get_features_range(input_data.prepare_model_settings(3, 16000, 1000, 30, 20, 40, mode))
    assert rng("average") == (0.0, 127.5) and rng("mfcc") == (-247.0, 30.0) and rng("micro") == (0.0, 26.0)
    with pytest.raises(ValueError):
        input_data.get_features_range(dict(preprocess="fft"))


def test_live_chain_is_micro_only():
    micro = input_data.standard_microspeech_model_settings(3)
    assert live._require_micro(micro, "LiveSession") is micro
    for mode in ("mfcc", "average"):
        with pytest.raises(ValueError, match="micro-only"):
            live._require_micro(input_data.prepare_model_settings(3, 16000, 1000, 30, 20, 40, mode), "LiveSession")


# ---- the tolerances ------------------------------------------------------------------------------------------------------------------
def test_tolerances_are_the_twins_measured_error_times_the_margin():
    e_power, e_mel, e_feat = sc.twin_errors()
    print(f"twin against float64 over {len(sc.ACCURACY_CASES)} configurations x {len(sc.INPUTS)} inputs: power {e_power:.3e}, mel {e_mel:.3e} of the frame "
          f"maximum, features {e_feat:.3e} absolute")
    assert sc.MARGIN == 4
    assert (sc.T_POWER, sc.T_MEL, sc.T_FEAT) == (sc.round_up_2(4 * e_power), sc.round_up_2(4 * e_mel), sc.round_up_2(4 * e_feat))


@pytest.mark.parametrize("geometry", list(sc.GEOMETRIES))
def test_floor_inputs_are_well_conditioned(geometry):
    """Every channel a bin feeds is at least MIN_CHANNEL_RATIO of its frame's maximum on the inputs the feature layer is compared on."""
    assert sc.MIN_CHANNEL_RATIO == 1e-4
    cfg = sc.cfg_of(geometry, "mfcc40")
    fed = sc.fed_channels(cfg)
    assert fed.sum() >= 30
    mel = sc.reference_of(geometry, "mfcc40")["mel"]
    assert not mel[:, :, ~fed].any()
    for name in sc.FLOOR_INPUTS:
        m = mel[sc.INPUTS.index(name)][:, fed]
        ratio = float((m.min(axis=-1) / m.max(axis=-1)).min())
        print(geometry, name, f"smallest channel / frame maximum = {ratio:.2e}")
        assert ratio >= sc.MIN_CHANNEL_RATIO, (geometry, name, ratio)
