"""The mfcc / average feature modes: a float64 reference written from the arithmetic include/mkws.h states (TensorFlow's spectrogram.cc,
mfcc_mel_filterbank.cc, mfcc_dct.cc and mfcc.cc restated), a float32 numpy twin of it whose own error against float64 sets the
tolerances, and the case tables of tests/test_spectral_cpu.py and tests/test_spectral_gpu.py.

Tolerances are measured, not chosen: twin_errors() is the twin's worst error against float64 over ACCURACY_CASES at three layers (power and
mel tap: abs err / frame max; features: abs err) and T_POWER, T_MEL, T_FEAT are MARGIN times those, rounded up to two digits
(test_spectral_cpu.py asserts that).  MARGIN = 4: the device's butterfly order, its unfused multiplies and adds and the hardware sqrt / log
roundings each differ from the twin's by about the twin's own error, while a wrong twiddle, window coefficient, band edge or DCT row
shows at 1e-4 of the frame maximum or worse.

Conditioning: the log amplifies the relative error of a channel by frame max / channel value, so the feature layer is compared only on the
inputs with a noise floor (FLOOR_INPUTS), on which every channel that is fed by a bin is at least MIN_CHANNEL_RATIO of its frame's maximum
(test_spectral_cpu.py asserts it for every such case).  A bare tone and a square wave are held at the power and mel taps only, silence at the
features (coefficient 0 = sqrt(2 / C) * C * ln(1e-12), the others 0)."""
import functools
import math

import numpy as np

from multilingual_kws_amd import synth

MARGIN = 4
T_POWER = 1.5e-6      # measured: the twin is 3.545e-07 of the frame maximum off float64
T_MEL = 3.8e-6        # measured: 9.494e-07 of the frame maximum (the chirp: sqrt of a small bin beside a large one)
T_FEAT = 2.8e-4       # measured: 6.853e-05 absolute (silence: forty float32 terms of -6.18 summed to -247.139)
MIN_CHANNEL_RATIO = 1e-4

GEOMETRIES = {            # name: (sample_rate, window, stride) -> fft
    "w480": (16000, 480, 320),      # 512, the standard
    "w640": (16000, 640, 320),      # 1024
    "w400": (16000, 400, 160),      # 512
    "w256": (8000, 256, 128),       # 256: the window equals the fft size, no zero padding
    "w129": (16000, 129, 64),       # 256: the shortest window the fft range admits
}
MODES = ("mfcc40", "mfcc13", "mfcc1", "avg6", "avg1", "avgall")
BATCHES = (1, 3, 65)
FLOOR_INPUTS = ("synth0", "synth1", "synth2", "quiet", "chirp")
TAP_ONLY_INPUTS = ("tone", "square")
INPUTS = FLOOR_INPUTS + TAP_ONLY_INPUTS + ("silence",)
CHIRP_AMPLITUDE, CHIRP_FLOOR = 0.15, 0.03      # (at 0.5 over 0.03 the chirp's smallest channel falls below MIN_CHANNEL_RATIO at 8 kHz)


def next_pow2(x):
    return 1 if x <= 1 else 2 ** (int(x) - 1).bit_length()


def cfg_of(geometry, mode):
    """-> the keyword arguments of spectral.make_cfg / SpectralFrontend."""
    sr, window, stride = GEOMETRIES[geometry]
    bins = next_pow2(window) // 2 + 1
    base = dict(sample_rate=sr, window_size_samples=window, window_stride_samples=stride)
    if mode.startswith("mfcc"):
        return dict(base, mode="mfcc", num_features=int(mode[4:]), filterbank_channels=40, lower_frequency_limit=20.0, upper_frequency_limit=4000.0)
    w = bins if mode == "avgall" else int(mode[3:])
    return dict(base, mode="average", average_window_width=w, num_features=-(-bins // w))


def shape_samples(geometry):
    """no frames, one frame, tail ignored, the standard clip, odd rows (clips 1.. are not 16-byte aligned)"""
    _, window, stride = GEOMETRIES[geometry]
    return (window - 1, window, window + stride - 1, 16000, 16001)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
@functools.lru_cache(maxsize=None)
def signals(sample_rate, n):
    """name -> float32 [n]"""
    t = np.arange(n, dtype=np.float64) / sample_rate
    rng = np.random.default_rng(0x5BEC)
    noise = rng.uniform(-1.0, 1.0, (2, n))
    clips = synth.clips_float32(3, n)
    f0, f1, dur = 100.0, 0.45 * sample_rate, max(n, 1) / sample_rate
    chirp = CHIRP_AMPLITUDE * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / dur * t * t)) + CHIRP_FLOOR * noise[1]
    out = dict(synth0=clips[0], synth1=clips[1], synth2=clips[2], quiet=1e-3 * noise[0], chirp=chirp, tone=0.5 * np.sin(2 * np.pi * 1000.0 * t),
               square=np.where(np.sin(2 * np.pi * 250.0 * t + 0.1) >= 0, 1.0, -1.0), silence=np.zeros(n))
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def input_batch(geometry, n=16000, names=INPUTS):
    return np.stack([signals(GEOMETRIES[geometry][0], n)[k] for k in names])


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference
def hann_periodic(window):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(window) / window)


def mel(f):
    return 1127.0 * np.log1p(np.asarray(f, dtype=np.float64) / 700.0)


def mel_tables(bins, sample_rate, channels, lower, upper):
    """-> (weights float64 [bins], band int [bins] (-2 outside), start, end)"""
    centre = mel(lower) + (np.arange(channels + 1) + 1) * (mel(upper) - mel(lower)) / (channels + 1)
    hz_per_bin = 0.5 * sample_rate / (bins - 1)
    start, end = int(1.5 + lower / hz_per_bin), int(upper / hz_per_bin)
    weights, band = np.zeros(bins), np.full(bins, -2, dtype=np.int64)
    for i in range(start, end + 1):
        m = float(mel(i * hz_per_bin))
        b = int(np.sum(centre[:channels] < m)) - 1
        band[i] = b
        weights[i] = (centre[b + 1] - m) / (centre[b + 1] - centre[b]) if b >= 0 else (centre[0] - m) / (centre[0] - float(mel(lower)))
    return weights, band, start, end


def dct_matrix(num_features, channels):
    k, j = np.arange(num_features)[:, None], np.arange(channels)[None, :]
    return math.sqrt(2.0 / channels) * np.cos(k * (math.pi / channels) * (j + 0.5))


def frames_of(audio, window, stride):
    """[B, n] -> [B, frames, window]"""
    B, n = audio.shape
    F = 0 if n < window else 1 + (n - window) // stride
    idx = np.arange(window)[None, :] + stride * np.arange(F)[:, None]
    return audio[:, idx.reshape(-1)].reshape(B, F, window)


def ref_power(audio, window, stride):
    """audio_spectrogram(magnitude_squared=True): [B, n] -> float64 [B, frames, bins]"""
    fr = frames_of(np.asarray(audio, dtype=np.float64), window, stride) * hann_periodic(window)
    z = np.fft.rfft(fr, n=next_pow2(window), axis=-1)
    return z.real ** 2 + z.imag ** 2


def ref_mel(power, sample_rate, channels=40, lower=20.0, upper=4000.0):
    """the filterbank outputs before the log: [..., bins] -> float64 [..., channels]"""
    weights, band, start, end = mel_tables(power.shape[-1], sample_rate, channels, lower, upper)
    out = np.zeros(power.shape[:-1] + (channels,))
    for i in range(start, end + 1):
        v, b = np.sqrt(power[..., i]), band[i]
        if b >= 0:
            out[..., b] += v * weights[i]
        if b + 1 < channels:
            out[..., b + 1] += v * (1.0 - weights[i])
    return out


def ref_mfcc_of_mel(mel_out, num_features):
    return np.log(np.maximum(mel_out, 1e-12)) @ dct_matrix(num_features, mel_out.shape[-1]).T


def ref_mfcc(power, sample_rate, num_features, channels=40, lower=20.0, upper=4000.0):
    return ref_mfcc_of_mel(ref_mel(power, sample_rate, channels, lower, upper), num_features)


def ref_average(power, w):
    """tf.nn.pool(AVG, SAME) over w bins: pads on the right only, divides by the number of real bins"""
    bins = power.shape[-1]
    return np.stack([power[..., o * w:min((o + 1) * w, bins)].mean(axis=-1) for o in range(-(-bins // w))], axis=-1)


def reference(cfg, audio):
    """cfg: cfg_of(...) -> dict(power=, mel= (mfcc only), feat=), float64"""
    power = ref_power(audio, cfg["window_size_samples"], cfg["window_stride_samples"])
    if cfg["mode"] == "mfcc":
        m = ref_mel(power, cfg["sample_rate"], cfg["filterbank_channels"], cfg["lower_frequency_limit"], cfg["upper_frequency_limit"])
        return dict(power=power, mel=m, feat=ref_mfcc_of_mel(m, cfg["num_features"]))
    return dict(power=power, feat=ref_average(power, cfg["average_window_width"]))


def fed_channels(cfg):
    """The channels some bin adds to: the others are 0 by construction, on every implementation."""
    bins = next_pow2(cfg["window_size_samples"]) // 2 + 1
    _, band, start, end = mel_tables(bins, cfg["sample_rate"], cfg["filterbank_channels"], cfg["lower_frequency_limit"], cfg["upper_frequency_limit"])
    C = cfg["filterbank_channels"]
    fed = np.zeros(C, dtype=bool)
    for i in range(start, end + 1):
        if band[i] >= 0:
            fed[band[i]] = True
        if band[i] + 1 < C:
            fed[band[i] + 1] = True
    return fed


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 twin: the same arithmetic in float32 with the tables rounded to float and scipy's float32 FFT
def twin(cfg, audio):
    import scipy.fft
    f32 = np.float32
    window, stride = cfg["window_size_samples"], cfg["window_stride_samples"]
    fr = frames_of(np.asarray(audio, dtype=f32), window, stride) * hann_periodic(window).astype(f32)
    z = scipy.fft.rfft(fr, n=next_pow2(window), axis=-1)
    assert z.dtype == np.complex64
    power = z.real * z.real + z.imag * z.imag
    if cfg["mode"] != "mfcc":
        w, bins = cfg["average_window_width"], power.shape[-1]
        outs = []
        for o in range(-(-bins // w)):
            acc = np.zeros(power.shape[:-1], dtype=f32)
            for i in range(o * w, min((o + 1) * w, bins)):
                acc = acc + power[..., i]
            outs.append(acc / f32(min((o + 1) * w, bins) - o * w))
        return dict(power=power, feat=np.stack(outs, axis=-1))
    C, F = cfg["filterbank_channels"], cfg["num_features"]
    weights, band, start, end = mel_tables(power.shape[-1], cfg["sample_rate"], C, cfg["lower_frequency_limit"], cfg["upper_frequency_limit"])
    weights = weights.astype(f32)
    mag = np.sqrt(power)
    m = np.zeros(power.shape[:-1] + (C,), dtype=f32)
    for i in range(start, end + 1):
        b = band[i]
        if b >= 0:
            m[..., b] += mag[..., i] * weights[i]
        if b + 1 < C:
            m[..., b + 1] += mag[..., i] * (f32(1.0) - weights[i])
    lg = np.log(np.maximum(m, f32(1e-12)))
    dct = dct_matrix(F, C).astype(f32)
    feat = np.zeros(power.shape[:-1] + (F,), dtype=f32)
    for j in range(C):
        feat = feat + lg[..., j:j + 1] * dct[:, j]
    assert power.dtype == f32 and m.dtype == f32 and feat.dtype == f32
    return dict(power=power, mel=m, feat=feat)


# ---------------------------------------------------------------------------------------------------------------------------------
# error measures
def frame_rel_err(got, want):
    """max over everything of abs err / the frame's maximum of `want` (a frame of zeros: the absolute error)"""
    if want.size == 0:
        return 0.0
    top = np.max(np.abs(want), axis=-1, keepdims=True)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.where(top > 0, top, 1.0)))


def abs_err(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want))) if want.size else 0.0


def rows_of(names):
    return [INPUTS.index(k) for k in names]


FEATURE_ROWS = rows_of(FLOOR_INPUTS + ("silence",))
ACCURACY_CASES = [(g, m) for g in GEOMETRIES for m in MODES]


def layer_errors(cfg, got, want):
    """The three measures of one INPUTS batch: (power, mel, features).  Average mode holds its features as abs err / the power's frame
    maximum, under the power layer."""
    e_power = frame_rel_err(got["power"], want["power"])
    if cfg["mode"] != "mfcc":
        top = np.max(want["power"], axis=-1, keepdims=True)
        e_avg = float(np.max(np.abs(np.asarray(got["feat"], dtype=np.float64) - want["feat"]) / np.where(top > 0, top, 1.0)))
        return max(e_power, e_avg), 0.0, 0.0
    return e_power, frame_rel_err(got["mel"], want["mel"]), abs_err(np.asarray(got["feat"])[FEATURE_ROWS], want["feat"][FEATURE_ROWS])


@functools.lru_cache(maxsize=None)
def reference_of(geometry, mode):
    return reference(cfg_of(geometry, mode), input_batch(geometry))


@functools.lru_cache(maxsize=None)
def twin_errors():
    """-> the twin's worst (power, mel, features) errors against float64 over ACCURACY_CASES"""
    worst = np.zeros(3)
    for g, m in ACCURACY_CASES:
        cfg = cfg_of(g, m)
        worst = np.maximum(worst, layer_errors(cfg, twin(cfg, input_batch(g)), reference_of(g, m)))
    return tuple(worst.tolist())


def round_up_2(x):
    """x rounded up to two significant digits"""
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return float(f"{math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e:.1e}")
