"""Shared by the loudness tests: the float64 numpy / scipy restatement of DESIGN.md section 40 (ITU-R BS.1770-4 integrated loudness, the
4x oversampled true peak, the gain rules) and the test signals.  This file is the oracle; nothing here calls the library."""
import numpy as np
from scipy.signal import lfilter

from tests.util_resample import splitmix

SHELF = dict(f0=1681.974450955533, G=3.999843853973347, Q=0.7071752369554196)
HIGH = dict(f0=38.13547087602444, Q=0.5003270373238773)
FLAG_UNMEASURED, FLAG_PEAK_LIMITED = 1, 2
# ITU-R BS.1770-4, table 1 and table 2 (48 kHz)
BS1770_48K = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                       [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]])


def k_coeffs(rate):
    """float64 [2, 5]: rows shelf and high-pass, columns b0, b1, b2, a1, a2 (a0 = 1), by the bilinear form libebur128 uses."""
    fs = float(rate)
    K = np.tan(np.pi * SHELF["f0"] / fs)
    Vh = 10.0 ** (SHELF["G"] / 20.0)
    Vb = Vh ** 0.4996667741545416
    Q = SHELF["Q"]
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K = np.tan(np.pi * HIGH["f0"] / fs)
    Q = HIGH["Q"]
    a0 = 1.0 + K / Q + K * K
    high = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, high], dtype=np.float64)


def k_weight(x, rate):
    """The row through both biquads from zero state, float64."""
    c = k_coeffs(rate)
    y = np.asarray(x, dtype=np.float64)
    for b0, b1, b2, a1, a2 in c:
        y = lfilter([b0, b1, b2], [1.0, a1, a2], y)
    return y


def true_peak_taps(zero_crossings=32, kaiser_beta=9.0, rolloff=0.95):
    """float32 [T, 4]: the project's Kaiser-windowed sinc (the resampler's design) with L = 4, M = 1: tab[j, p] = (float) h[p + 4 j]."""
    L = 4
    half = zero_crossings * L
    T = (2 * half + 1 + L - 1) // L
    fc = rolloff / L
    i = np.arange(-half, half + 1, dtype=np.float64)
    h = L * fc * np.sinc(fc * i) * np.i0(kaiser_beta * np.sqrt(np.maximum(0.0, 1.0 - (i / half) ** 2))) / np.i0(kaiser_beta)
    tab = np.zeros(T * L, np.float32)
    tab[:2 * half + 1] = h.astype(np.float32)
    return tab.reshape(T, L)


def as_f32(x):
    x = np.asarray(x)
    return x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x.astype(np.float32)


def true_peak(x, tab):
    """max |y| over the 4 len oversampled samples in float64 on the float32 taps `tab`, centred, zeros outside the row -> (the peak,
    the rounding bound of a float32 evaluation: (T + 1) 2^-24 max_j sum |h x|)."""
    x = as_f32(x).astype(np.float64)
    n = len(x)
    if n == 0:
        return 0.0, 0.0
    T, L = tab.shape
    zc = (T - 1) // 2                                    # half / L: output L i + p is sum_j tab[j, p] x[i + zc - j]
    peak = mag = 0.0
    for p in range(L):
        h = tab[:, p].astype(np.float64)
        peak = max(peak, float(np.abs(np.convolve(x, h)[zc:zc + n]).max()))
        mag = max(mag, float(np.convolve(np.abs(x), np.abs(h))[zc:zc + n].max()))
    return peak, (T + 1) * 2.0 ** -24 * mag


def measure(x, rate, tab=None, peaks=True):
    """One row (float32, or int16 taken as v / 32768), all of it -> dict of the statistics row and the block counts (peaks = False
    leaves the oversampling out: true_peak and tp_bound are None)."""
    x = as_f32(x)
    n = len(x)
    if rate % 10:
        raise ValueError("the rate must be a multiple of 10")
    hop = rate // 10
    block = 4 * hop
    y = k_weight(x, rate)
    nb = (n - block) // hop + 1 if n >= block else 0
    z = np.array([np.mean(y[j * hop:j * hop + block] ** 2) for j in range(nb)], dtype=np.float64)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    absolute = l > -70.0
    L, relative = -np.inf, np.zeros(nb, bool)
    if absolute.any():
        gamma = -0.691 + 10.0 * np.log10(np.cumsum(z[absolute])[-1] / absolute.sum()) - 10.0
        relative = absolute & (l > gamma)
        if relative.any():
            L = -0.691 + 10.0 * np.log10(np.cumsum(z[relative])[-1] / relative.sum())
    tp, bound = true_peak(x, true_peak_taps() if tab is None else tab) if peaks else (None, None)
    x64 = x.astype(np.float64)
    return dict(loudness=float(L), true_peak=tp, tp_bound=bound, sample_peak=float(np.abs(x64).max()) if n else 0.0,
                mean_square=float(np.mean(x64 * x64)) if n else 0.0, blocks=int(nb), absolute=int(absolute.sum()), relative=int(relative.sum()))


def gain_of(m, target_lufs=-16.0, true_peak_db=-1.5, mode="loudness", headroom_db=0.1):
    """-> (float32 gain, flags) from measure()'s dict."""
    if mode == "peak":
        if m["sample_peak"] > 0.0:
            return np.float32(10.0 ** (-headroom_db / 20.0) / m["sample_peak"]), 0
        return np.float32(1.0), FLAG_UNMEASURED
    if m["loudness"] == -np.inf:
        return np.float32(1.0), FLAG_UNMEASURED
    g_db, flags = target_lufs - m["loudness"], 0
    tp_db = 20.0 * np.log10(m["true_peak"]) if m["true_peak"] > 0.0 else -np.inf
    if tp_db + g_db > true_peak_db:
        g_db, flags = true_peak_db - tp_db, FLAG_PEAK_LIMITED
    return np.float32(10.0 ** (g_db / 20.0)), flags


# -- signals ---------------------------------------------------------------------------------------------------------------------------

def sine(rate, freq, dbfs, seconds, phase_deg=0.0, start=0):
    t = (np.arange(int(round(seconds * rate)), dtype=np.float64) + start) / rate
    return 10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * freq * t + np.deg2rad(phase_deg))


def steps(rate, freq, parts):
    """A phase-continuous sine through parts = [(dBFS, seconds), ...] (EBU Tech 3341's level steps), float32."""
    out, at = [], 0
    for dbfs, seconds in parts:
        out.append(sine(rate, freq, dbfs, seconds, start=at))
        at += len(out[-1])
    return np.concatenate(out).astype(np.float32)


def conformance_signals(rate=16000):
    """name -> (mono float32 signal, the expected reading: the stereo figure of Tech 3341 less 3.01 LU for the one channel)."""
    return {
        "tech3341_case3": (steps(rate, 1000.0, [(-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0)]), -26.01),
        "tech3341_case4": (steps(rate, 1000.0, [(-72.0, 10.0), (-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0), (-72.0, 10.0)]), -26.01),
        "tech3341_case5": (steps(rate, 1000.0, [(-26.0, 20.0), (-20.0, 20.1), (-26.0, 20.0)]), -26.01),
        "sine_997_0dbfs": (steps(rate, 997.0, [(0.0, 20.0)]), -3.01),
    }


# EBU Tech 3341 true-peak cases at 48 kHz: (amplitude, fs / divisor, phase in degrees, expected dBTP); the window is +0.2 / -0.4
TRUE_PEAK_CASES = [(0.5, 4, 0.0, -6.0), (0.5, 4, 45.0, -6.0), (0.5, 6, 60.0, -6.0), (0.5, 8, 67.5, -6.0), (1.41, 4, 45.0, 3.0)]


def true_peak_signal(amplitude, divisor, phase_deg, rate=48000, seconds=0.5, fade_ms=50):
    """The sine at fs / divisor under 50 ms raised-cosine fades, so that no edge transient enters; float32."""
    n = int(seconds * rate)
    x = amplitude * np.sin(2.0 * np.pi * np.arange(n) / divisor + np.deg2rad(phase_deg))
    f = int(rate * fade_ms / 1000)
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(f) + 0.5) / f)
    x[:f] *= ramp
    x[n - f:] *= ramp[::-1]
    return x.astype(np.float32)


def ramp_noise(n, rate, seed, dtype=np.float32, lo_db=-80.0, hi_db=-6.0, dc=0.05):
    """Seeded noise in [-1, 1] with a DC offset under a level ramp from lo_db to hi_db dBFS across the row: early blocks fall to the
    absolute gate, the middle ones to the relative gate.  int16: the same, rounded to the 16-bit grid."""
    u = (splitmix(n, seed) >> np.uint64(40)).astype(np.float64) / 2.0 ** 23 - 1.0
    level = 10.0 ** ((lo_db + (hi_db - lo_db) * (np.arange(n, dtype=np.float64) + 0.5) / max(n, 1)) / 20.0)
    x = (u * (1.0 - dc) + dc) * level
    if np.dtype(dtype) == np.int16:
        return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)
