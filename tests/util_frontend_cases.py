"""The configuration matrix, the signal set and the plan restatement behind the frontend's bit-exact claim.

Shared by tests/test_frontend_cases_cpu.py (what the matrix is for: which branch of mkws_frontend.hip each configuration reaches)
and tests/test_frontend_configs_gpu.py (the kernels against the oracle on every configuration).  Nothing here touches a device.
"""
import functools
import math

import numpy as np

# name -> (overrides of the default configuration, clip length n).  Every one has a 512-point FFT and at most 64 channels, and
# frames x channels <= 3960 so that the one-workgroup-per-clip kernel fits its LDS.
CASES = {
    "default": ({}, 16000),
    "c64_nopcan": (dict(num_channels=64, enable_pcan=0), 16000),
    "c63": (dict(num_channels=63), 16000),
    "c33": (dict(num_channels=33), 16000),
    "c6": (dict(num_channels=6), 16000),
    "c1": (dict(num_channels=1), 16000),
    "sr22050_nolog": (dict(sample_rate=22050, window_size_ms=20, window_step_ms=10, upper_band_limit=10000, enable_log=0), 22050),
    "sr11025": (dict(sample_rate=11025, window_size_ms=30, window_step_ms=15, upper_band_limit=5000), 11025),
    "sr44100": (dict(sample_rate=44100, window_size_ms=11, window_step_ms=5, upper_band_limit=20000), 22050),
    "w512": (dict(window_size_ms=32, window_step_ms=10), 16000),
    "w272": (dict(window_size_ms=17, window_step_ms=3), 4800),
    "sr12345": (dict(sample_rate=12345, window_size_ms=30, window_step_ms=7, upper_band_limit=6000), 6001),
}
DEFAULTS = dict(sample_rate=16000, window_size_ms=30, window_step_ms=20, num_channels=40, upper_band_limit=7500.0, lower_band_limit=125.0,
                enable_pcan=1, enable_log=1)
SEED = 20


def full_cfg(name):
    """The configuration with the defaults the plan depends on filled in."""
    return dict(DEFAULTS, **CASES[name][0])


# ------------------------------------------------------------------------------------------------------------------------- signals

SIGNAL_NAMES = ("noise_full", "noise_amp3", "burst", "const_min", "const_max", "nyquist", "impulses", "chirp", "quiet_loud", "zeros")


def signals(n, sample_rate, seed):
    """int16 [10, n], the rows named by SIGNAL_NAMES: clips that move every stage of the frontend, not only the FFT."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    out = {}
    out["noise_full"] = rng.integers(-32768, 32768, size=n)
    out["noise_amp3"] = rng.integers(-3, 4, size=n)
    burst = np.zeros(n, dtype=np.int64)                          # noise-estimate decay, the min_signal_remaining floor, log inputs <= 1
    lo, hi = (5 * n) // 12, (7 * n) // 12
    burst[lo:hi] = rng.integers(-32768, 32768, size=hi - lo)
    out["burst"] = burst
    out["const_min"] = np.full(n, -32768)
    out["const_max"] = np.full(n, 32767)
    out["nyquist"] = np.where(i % 2 == 0, 32767, -32768)
    imp = np.zeros(n, dtype=np.int64)
    imp[::97] = 32767
    imp[::131] = -32768
    out["impulses"] = imp
    t = i / float(sample_rate)                                   # 0 .. Nyquist over the clip
    out["chirp"] = np.round(30000.0 * np.sin(2.0 * np.pi * 0.5 * (0.5 * sample_rate) / (n / float(sample_rate)) * t * t))
    sign = np.asarray([1, 1, -1, 1, -1, -1, 1])[i % 7]
    out["quiet_loud"] = sign * np.where(i < n // 2, 1, 20000)
    out["zeros"] = np.zeros(n, dtype=np.int64)
    pcm = np.stack([np.asarray(out[k]) for k in SIGNAL_NAMES])
    assert pcm.min() >= -32768 and pcm.max() <= 32767
    return pcm.astype(np.int16)


@functools.lru_cache(maxsize=None)
def case_signals(name, n=None):
    """The ten clips of a configuration (read-only), at its own length or at n samples."""
    over, n0 = CASES[name]
    pcm = signals(n0 if n is None else n, full_cfg(name)["sample_rate"], SEED)
    pcm.setflags(write=False)
    return pcm


@functools.lru_cache(maxsize=None)
def case_expected(name, n=None, cut=0):
    """The oracle's raw uint16 [10, frames, channels] on case_signals(name, n)[:, :len - cut], computed once (read-only)."""
    from oracle.frontend_oracle import FrontendOracle
    fo = FrontendOracle(**CASES[name][0])
    pcm = case_signals(name, n)
    exp = np.stack([fo.run_i16(c[:c.shape[0] - cut]) for c in pcm])
    exp.setflags(write=False)
    return exp


def stream_geometry(name):
    """(window_samples, hop_samples, total samples) of the stream / live cases: 21 frames per window, a hop of two steps, 41 windows."""
    p = plan(name)
    window_samples, hop_samples = p["window_size"] + 20 * p["window_step"], 2 * p["window_step"]
    return window_samples, hop_samples, window_samples + 40 * hop_samples


@functools.lru_cache(maxsize=None)
def stream_recording(name):
    """int16 [total]: burst, chirp, quiet-then-loud and full-scale noise one after the other, each a quarter of the recording."""
    total = stream_geometry(name)[2]
    pcm = case_signals(name, -(-total // 4))
    rec = np.concatenate([pcm[SIGNAL_NAMES.index(k)] for k in ("burst", "chirp", "quiet_loud", "noise_full")])[:total].copy()
    rec.setflags(write=False)
    return rec


# ----------------------------------------------------------------------------------------------------------------- plan restatement

_F = np.float32


def _mel(hz):
    """mkws_frontend_tables.cpp mel_of: float in, double log1p, rounded back to float."""
    return _F(1127.0 * math.log1p(float(_F(hz)) / 700.0))


@functools.lru_cache(maxsize=None)
def plan(name):
    """What mkws_frontend_create decides for a configuration, restated on numpy float32: the table scalars, the per-output tap lists
    (bin widths in the float32 mel arithmetic of mkws_frontend_tables.cpp), the helper split (longest lists first, stop at a list
    shorter than 2 or when the 64 lanes run out), the padded lane length nm, the weight sums and fast48."""
    c = full_cfg(name)
    sr, C = c["sample_rate"], c["num_channels"]
    C1 = C + 1
    window_size, window_step = c["window_size_ms"] * sr // 1000, c["window_step_ms"] * sr // 1000
    fft_size = 1
    while fft_size < window_size:
        fft_size *= 2
    spectrum = fft_size // 2 + 1
    mel_lo, mel_hi = _mel(c["lower_band_limit"]), _mel(c["upper_band_limit"])
    spacing = _F(_F(mel_hi - mel_lo) / _F(C1))
    center = [_F(mel_lo + _F(spacing * _F(i + 1))) for i in range(C1)]
    hz_per_bin = _F(0.5 * sr / (float(_F(spectrum)) - 1))
    start_index = int(1.5 + float(_F(_F(c["lower_band_limit"]) / hz_per_bin)))
    bin_mel = [_mel(_F(_F(f) * hz_per_bin)) for f in range(2 * spectrum + 1)]
    astart, awidth, freq_starts, weight_starts, widths = [], [], [0] * C1, [0] * C1, [0] * C1
    cur, running, zeros_inserted = start_index, 0, False
    for ch in range(C1):
        f = cur
        while f < 2 * spectrum and bin_mel[f] <= center[ch]:
            f += 1
        astart.append(cur)
        awidth.append(f - cur)
        if f == cur:
            widths[ch] = 4
            if not zeros_inserted:
                zeros_inserted = True
                for j in range(ch):
                    weight_starts[j] += 4
                running += 4
        else:
            aligned = cur // 2 * 2
            padded = ((cur - aligned + f - cur - 1) // 4 + 1) * 4
            freq_starts[ch], weight_starts[ch], widths[ch] = aligned, running, padded
            running += padded
        cur = f
    num_weights = running
    weights, unweights = np.zeros(num_weights, np.int16), np.zeros(num_weights, np.int16)
    W, U, end_index = {}, {}, 0
    for ch in range(C1):
        denom = mel_lo if ch == 0 else center[ch - 1]
        for j in range(awidth[ch]):
            b = astart[ch] + j
            w = _F(_F(center[ch] - bin_mel[b]) / _F(center[ch] - denom))
            W[b] = int(math.floor(float(_F(w * _F(4096))) + 0.5))
            U[b] = int(math.floor((1.0 - float(w)) * 4096 + 0.5))
            idx = weight_starts[ch] + astart[ch] - freq_starts[ch] + j
            weights[idx], unweights[idx] = W[b], U[b]
        if awidth[ch] > 0:
            end_index = max(end_index, astart[ch] + awidth[ch])
    out_len = [awidth[o] + awidth[o + 1] for o in range(C)]
    out_coef = [[U[astart[o] + j] for j in range(awidth[o])] + [W[astart[o + 1] + j] for j in range(awidth[o + 1])] for o in range(C)]
    # the helper split of mkws_frontend_create
    lane_len = out_len + [0] * (64 - C)
    order = sorted(range(C), key=lambda o: -out_len[o])          # (sorted is stable, like std::stable_sort)
    helped = []
    for k, lane in zip(range(C), range(C, 64)):
        o = order[k]
        if out_len[o] < 2:
            break
        first = (out_len[o] + 1) // 2
        lane_len[o], lane_len[lane] = first, out_len[o] - first
        helped.append(o)
    nm = max([4] + [(x + 3) & ~3 for x in lane_len])
    sums = [sum(l) for l in out_coef]
    nonneg = all(w >= 0 for l in out_coef for w in l)
    return dict(window_size=window_size, window_step=window_step, fft_size=fft_size, start_index=start_index, end_index=end_index,
                num_weights=num_weights, weights=weights, unweights=unweights, chan_freq_starts=freq_starts,
                chan_weight_starts=weight_starts, chan_widths=widths, out_len=out_len, helped=helped, lane_len=lane_len, nm=nm,
                sums=sums, sum_ok=nonneg and max(sums) <= 65536, fast48=nonneg and max(sums) <= 65536 and nm <= 32)
