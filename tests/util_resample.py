"""Shared by the resampler tests: a numpy restatement of the specification in include/mkws.h ("Sample-rate conversion") with the dtype
as a parameter -- float32 gives the emulator the device must equal bit for bit, float64 the oracle -- and the test signals."""
import numpy as np

RATES = (48000, 44100, 32000, 22050, 11025, 8000)


def polyphase(x, tab, M, off, dtype, ns=None, want_abs=False):
    """y[n] = sum_j tab[j, p] * x[q - j] for m = n * M + off, q = m div L, p = m mod L, accumulated from +0 in `dtype`, one multiply and one
    add per tap, j ascending; x outside the row is 0.  tab: float32 [T, L]; ns: the outputs to evaluate (default: all ceil(n * L / M)).
    want_abs: also sum_j |tab * x| in float64, the scale of the rounding bound."""
    T, L = tab.shape
    x, tabd = np.asarray(x).astype(dtype), tab.astype(dtype)
    ns = np.arange(-(-len(x) * L // M), dtype=np.int64) if ns is None else np.asarray(ns, dtype=np.int64)
    m = ns * M + off
    q, p = m // L, m % L
    acc, mag = np.zeros(len(ns), dtype), np.zeros(len(ns), np.float64)
    for j in range(T):
        i = q - j
        xs = np.where((i >= 0) & (i < len(x)), x[np.clip(i, 0, len(x) - 1)], dtype(0))
        prod = tabd[j, p] * xs
        acc = acc + prod
        if want_abs:
            mag += np.abs(prod.astype(np.float64))
    return (acc, mag) if want_abs else acc


def _around_tile(rs, n_out):
    """Input lengths whose outputs end one each side of n_out samples and on it (an upsampler's lengths step by more than one)."""
    g = rs.geometry
    first, last = (n_out - 1) * g["M"] // g["L"] + 1, n_out * g["M"] // g["L"]          # the smallest and largest n_in that give n_out
    assert rs.out_samples(first) == rs.out_samples(last) == n_out and rs.out_samples(first - 1) < n_out < rs.out_samples(last + 1)
    return sorted({first - 1, first, last, last + 1})


def _check(rs, x_rows, got_rows, centred, tab=None):
    """Every row of a device result against the emulator on the handle's own taps (tab: rs.taps(), when the caller keeps it): bit-equal
    to the float32 form and within (T + 1) * 2^-24 * sum_j |tab * x| of the float64 form."""
    g, tab = rs.geometry, rs.taps() if tab is None else tab
    off = g["half"] if centred else 0
    for x, got in zip(x_rows, got_rows):
        xf = x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x
        want = polyphase(xf, tab, g["M"], off, np.float32)
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rs.rate_in, len(x), centred, int((got != want).sum()))
        exact, mag = polyphase(xf, tab, g["M"], off, np.float64, want_abs=True)
        assert np.all(np.abs(got - exact) <= (g["T"] + 1) * 2.0 ** -24 * mag)


def splitmix(n, seed):
    """uint64 [n] of splitmix64 from `seed`."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise_f32(n, seed):
    """float32 noise in [-1, 1] with exact zeros, +1.0 and -1.0 sprinkled in."""
    x = ((splitmix(n, seed) >> np.uint64(40)).astype(np.float64) / 2.0 ** 23 - 1.0).astype(np.float32)
    x[5::97], x[7::101], x[11::103] = 0.0, 1.0, -1.0
    return x


def noise_i16(n, seed):
    """int16 noise over the whole range with zeros and both extremes sprinkled in."""
    x = (splitmix(n, seed) >> np.uint64(48)).astype(np.uint16).view(np.int16).copy()
    x[5::97], x[7::101], x[11::103] = 0, 32767, -32768
    return x
