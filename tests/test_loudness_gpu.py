"""mkws_loudness_* and its wrappers against the float64 oracle (tests/util_loudness.py).

Parity: the integrated loudness within 1e-6 LU where it is finite (a float32 gain resolves 5e-7 dB), -inf and the three block counts
exactly, the sample peak exactly, the mean square within 1e-12 relative, the true peak within (T + 1) 2^-24 max_j sum |h x| of the
float64 evaluation of the same float32 taps.  Every input sits between canary bands (NaN for float32, -32768 for int16) with row strides
longer than the rows, and every output in a canary-filled allocation whose bands and gaps must keep the canary.

The gain: within 1 float32 ulp of the oracle's own gain, also where the true-peak limit binds and the gain is limit / true_peak (the
device sums the oversampled row in float64, so its true peak carries no float32 rounding into the gain)."""
import ctypes
import io
import wave

import numpy as np
import pytest

from multilingual_kws_amd import _lib, loudness, resample
from tests import util_loudness as ul
from util_fenced import PAD, FencedBuffer, holds_canary

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATES = (16000, 8000, 48000, 44100)
GAP = 37                                     # elements between the rows of a strided batch

_meters, _oracle = {}, {}


def _meter(rate, **kw):
    key = (rate, tuple(sorted(kw.items())))
    if key not in _meters:
        _meters[key] = loudness.LoudnessMeter(rate, max_rows=3, max_samples=5 * rate, **kw)
    return _meters[key]


@pytest.fixture(scope="module", autouse=True)
def _close_meters():
    yield
    import torch
    torch.cuda.synchronize()
    for m in _meters.values():
        m.close()
    _meters.clear()
    _oracle.clear()


def _taps():
    if "taps" not in _oracle:
        _oracle["taps"] = resample.host_taps(resample.make_cfg(1, 4))
    return _oracle["taps"]


def _row(rate, n, seed, dtype):
    """(the row, the oracle's reading of it), computed once."""
    key = (rate, n, seed, np.dtype(dtype).name)
    if key not in _oracle:
        x = ul.ramp_noise(n, rate, seed, dtype)
        _oracle[key] = (x, ul.measure(x, rate, _taps()))
    return _oracle[key]


class _Input:
    """Rows [B, n] at `stride` elements between canary bands: NaN around float32 rows, -32768 around int16 rows."""

    def __init__(self, rows, stride):
        import torch
        B, n = rows.shape
        span = (B - 1) * stride + n
        if rows.dtype == np.float32:
            self.buf = FencedBuffer(span, "float32", device=DEV)
            self.whole, mid = self.buf.whole, self.buf.mid
        else:
            assert rows.dtype == np.int16
            self.whole = torch.full((2 * PAD + span + 2 * PAD,), -32768, dtype=torch.int16, device=DEV)
            mid = self.whole[2 * PAD:2 * PAD + span]
        self.view = mid.as_strided((B, n), (stride, 1))
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
        self.snap = self.whole.clone()

    def unchanged(self):
        import torch
        return torch.equal(self.whole, self.snap)


def _call(meter, rows, lengths=None, stride=None):
    """mkws_loudness_measure and mkws_loudness_apply on fenced buffers -> (stats [B, 4], counts [B, 4], gain [B], out [B, n])."""
    import torch
    L = _lib.lib()
    B, n = rows.shape
    stride = n + GAP if stride is None else stride
    inp = _Input(rows, stride)
    stats, counts, gain = FencedBuffer(B * 4, "float64", device=DEV), FencedBuffer(B * 4, "int32", device=DEV), FencedBuffer(B, "float32", device=DEV)
    ostride = n + GAP + 3
    out = FencedBuffer((B - 1) * ostride + n, "float32", device=DEV)
    d_len = torch.tensor(lengths, dtype=torch.int64, device=DEV) if lengths is not None else None
    p_len = ctypes.c_void_p(d_len.data_ptr()) if d_len is not None else None
    i16, st = int(rows.dtype == np.int16), _lib.current_stream_ptr()
    _lib.check(L.mkws_loudness_measure(meter.h, ctypes.c_void_p(inp.view.data_ptr()), i16, B, n, stride, p_len, ctypes.c_void_p(stats.ptr()),
                                       ctypes.c_void_p(counts.ptr()), ctypes.c_void_p(gain.ptr()), st))
    _lib.check(L.mkws_loudness_apply(meter.h, ctypes.c_void_p(inp.view.data_ptr()), i16, B, n, stride, p_len, ctypes.c_void_p(gain.ptr()),
                                     ctypes.c_void_p(out.ptr()), ostride, st))
    torch.cuda.synchronize()
    assert inp.unchanged(), "the input or its bands were written"
    for name, buf in (("stats", stats), ("counts", counts), ("gain", gain), ("out", out)):
        assert buf.pads_intact(), f"a band of {name} was written"
        if name != "out":
            assert not buf.canary_mask().any(), f"an element of {name} was not written"
    h = out.host()
    inside = np.zeros(h.size, bool)
    for b in range(B):
        inside[b * ostride:b * ostride + n] = True
    assert holds_canary(h[~inside]).all(), "the output was written between its rows"
    assert not holds_canary(h[inside]).any(), "an output sample was not written"
    return (stats.host().reshape(B, 4), counts.host().reshape(B, 4), gain.host(),
            np.stack([h[b * ostride:b * ostride + n] for b in range(B)]))


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def _check_row(tag, x, m, stats, counts, gain, out, n, opts=None):
    """One row of a device result against the oracle's reading `m` of x (its own samples); n: the width of the batch it sat in."""
    opts = opts or {}
    L, tp, sp, ms = (float(v) for v in stats)
    print(f"{tag}: L {L!r} vs {m['loudness']!r}; tp err {abs(tp - m['true_peak']):.3e} of {m['tp_bound']:.3e}; "
          f"ms rel {abs(ms - m['mean_square']) / max(m['mean_square'], 1e-300):.3e}; counts {counts.tolist()}")
    if np.isfinite(m["loudness"]):
        assert abs(L - m["loudness"]) <= 1e-6, tag
    else:
        assert L == m["loudness"], tag
    assert counts[:3].tolist() == [m["blocks"], m["absolute"], m["relative"]], tag
    assert sp == m["sample_peak"], tag
    assert abs(ms - m["mean_square"]) <= 1e-12 * m["mean_square"], tag
    assert abs(tp - m["true_peak"]) <= m["tp_bound"], tag
    want, flags = ul.gain_of(m, **opts)
    print(f"{tag}: gain {_ulps(gain, want)} ulp from the oracle's{' (peak-limited)' if flags & ul.FLAG_PEAK_LIMITED else ''}")
    assert _ulps(gain, want) <= 1 and int(counts[3]) == flags, (tag, gain, want, counts[3], flags)
    xf = ul.as_f32(x)
    assert np.array_equal((xf * np.float32(gain)).view(np.uint32), out[:len(x)].view(np.uint32)), tag
    assert not out[len(x):n].view(np.uint32).any(), tag
    if flags & ul.FLAG_UNMEASURED:
        assert gain == np.float32(1.0) and np.array_equal(out[:len(x)].view(np.uint32), xf.view(np.uint32)), tag


def _lengths(rate):
    g = loudness.geometry(loudness.make_cfg(rate))
    hop, block, chunk, tile = g["hop"], g["block"], g["chunk"], g["tile"]
    k = block // chunk + 5                       # chunk multiples past one block, off the hop grid
    assert (k * chunk) % hop and (2 * k * chunk) % hop
    return g, sorted({1, block - 1, block, block + hop - 1, block + hop, chunk - 1, chunk + 1, 2 * chunk - 1, 2 * chunk + 1,
                      k * chunk - 1, k * chunk + 1, 2 * k * chunk - 1, 2 * k * chunk + 1, tile - 1, tile, tile + 1, 5 * rate} - {0})


@pytest.mark.parametrize("rate", RATES)
def test_parity_with_the_oracle(rate):
    g, lengths = _lengths(rate)
    meter = _meter(rate)
    removed = [0, 0]
    for i, n in enumerate(lengths):
        for dtype in ((np.float32, np.int16) if n in (g["block"] + g["hop"], g["tile"] + 1, 5 * rate) else ((np.float32, np.int16)[i % 2],)):
            x, m = _row(rate, n, 100 + i, dtype)
            stats, counts, gain, out = _call(meter, x[None])
            _check_row(f"{rate} n={n} {np.dtype(dtype).name}", x, m, stats[0], counts[0], gain[0], out[0], n)
            removed[0] += m["blocks"] - m["absolute"]
            removed[1] += m["absolute"] - m["relative"]
    assert removed[0] > 0 and removed[1] > 0, "the content must lose blocks to each gate"
    # B = 3, rows of one length at a stride longer than the rows
    for n, dtype in ((g["block"] + g["hop"], np.float32), (g["tile"] + 1, np.int16)):
        rows = [_row(rate, n, 200 + b, dtype) for b in range(3)]
        stats, counts, gain, out = _call(meter, np.stack([x for x, _ in rows]))
        for b, (x, m) in enumerate(rows):
            _check_row(f"{rate} B=3 n={n} row {b}", x, m, stats[b], counts[b], gain[b], out[b], n)
    # ragged: every row's own samples, then poison up to the batch's width
    own = [g["block"] - 1, g["block"] + g["hop"], g["tile"] + 1]
    for dtype, poison in ((np.float32, np.float32(np.nan)), (np.int16, np.int16(-32768))):
        n = max(own) + 5
        rows = [_row(rate, k, 300 + b, dtype) for b, k in enumerate(own)]
        batch = np.full((3, n), poison, dtype)
        for b, (x, _) in enumerate(rows):
            batch[b, :len(x)] = x
        stats, counts, gain, out = _call(meter, batch, lengths=own)
        for b, (x, m) in enumerate(rows):
            _check_row(f"{rate} ragged {np.dtype(dtype).name} row {b}", x, m, stats[b], counts[b], gain[b], out[b], n)


def test_conformance_loudness_on_the_device():
    """EBU Tech 3341 cases 3, 4, 5 and the 997 Hz sine, one channel at 16 kHz: within +-0.1 LU."""
    import torch
    signals = ul.conformance_signals(16000)
    meter = loudness.LoudnessMeter(16000, max_rows=1, max_samples=max(len(x) for x, _ in signals.values()))
    try:
        for name, (x, want) in signals.items():
            stats, counts = meter.measure(torch.from_numpy(x).to(DEV))
            got = float(stats[0])
            print(name, got, counts.tolist())
            assert abs(got - want) <= 0.1, (name, got)
    finally:
        meter.close()


def test_conformance_true_peak_on_the_device():
    """EBU Tech 3341's true-peak cases at 48 kHz under 50 ms fades: -6.0 (+3.0 for the 1.41 FS case) +0.2 / -0.4 dBTP."""
    meter = _meter(48000)
    for amp, div, phase, want in ul.TRUE_PEAK_CASES:
        x = ul.true_peak_signal(amp, div, phase)
        oracle = 20.0 * np.log10(ul.true_peak(x, _taps())[0])
        assert want - 0.4 <= oracle <= want + 0.2, (amp, div, phase, oracle)
        stats, _ = meter.measure(x)
        got = 20.0 * np.log10(float(stats[1]))
        print(amp, div, phase, got, oracle)
        assert want - 0.4 <= got <= want + 0.2, (amp, div, phase, got)


def _steady(n, seed, dbfs):
    """Seeded noise at one level: every block passes both gates whatever the gain, so the reading moves with the gain exactly."""
    return ul.ramp_noise(n, 16000, seed, lo_db=dbfs, hi_db=dbfs, dc=0.0)


def test_gain_and_output():
    import torch
    rate, n = 16000, 16000
    quiet, loud = _steady(n, 1, -40.0), _steady(n, 2, -3.0)
    silent, short = np.zeros(n, np.float32), _steady(n, 3, -20.0)
    meter = _meter(rate)
    batch = np.stack([quiet, loud, silent])
    out = meter.normalize(batch)
    gains = meter.gains(batch)
    stats, counts = meter.measure(batch)
    assert out.dtype == np.float32 and gains.dtype == np.float32 and stats.dtype == np.float64 and counts.dtype == np.int32
    assert np.array_equal(out.view(np.uint32), (batch * gains[:, None]).view(np.uint32))
    assert counts[:, 3].tolist() == [0, 0, ul.FLAG_UNMEASURED]
    again, _ = meter.measure(out)
    # the limit did not bind: the output reads the target
    assert abs(again[0, 0] - (-16.0)) <= 1e-4 and abs(again[1, 0] - (-16.0)) <= 1e-4, again[:2, 0]
    # it did (a target the row's peaks do not allow): the output's true peak is the limit, within what float32 allows: the gain carries
    # the relative error of the device's true peak and its own rounding, every output sample one more rounding, and the second
    # measurement its own bound on the scaled row
    hot = _meter(rate, target_lufs=-3.0)
    out_hot, gains_hot = hot.normalize(batch), hot.gains(batch)
    assert hot.measure(batch)[1][:, 3].tolist() == [ul.FLAG_PEAK_LIMITED, ul.FLAG_PEAK_LIMITED, ul.FLAG_UNMEASURED]
    again_hot, _ = hot.measure(out_hot)
    lim = 10.0 ** (-1.5 / 20.0)
    for b, x in enumerate((quiet, loud)):
        m = ul.measure(x, rate, _taps())
        assert ul.gain_of(m, target_lufs=-3.0)[1] == ul.FLAG_PEAK_LIMITED
        b_out = float(gains_hot[b]) * m["tp_bound"] * (1.0 + 2.0 ** -23)
        print("limited", b, again_hot[b, 1] - lim, lim * (m["tp_bound"] / m["true_peak"] + 2.0 ** -24) + 2.0 * b_out)
        assert abs(again_hot[b, 1] - lim) <= lim * (m["tp_bound"] / m["true_peak"] + 2.0 ** -24) + 2.0 * b_out, (b, again_hot[b, 1], lim)
        assert again_hot[b, 0] < -3.0
    # silence and a row shorter than a block come back untouched and flagged
    assert gains[2] == 1.0 and np.array_equal(out[2], silent) and stats[2, 0] == -np.inf and stats[2, 1] == 0.0
    lengths = [n, n, 6399]
    ragged = np.stack([quiet, loud, short])
    out2 = meter.normalize(ragged, lengths=lengths)
    s2, c2 = meter.measure(ragged, lengths=lengths)
    assert c2[2].tolist() == [0, 0, 0, ul.FLAG_UNMEASURED] and s2[2, 0] == -np.inf
    assert np.array_equal(out2[2, :6399], short[:6399]) and not out2[2, 6399:].any()
    assert np.array_equal(out2[:2], out[:2])
    # a rank-1 row, a tensor on the device, a strided view, an out tensor
    one = meter.normalize(quiet)
    assert one.shape == (n,) and np.array_equal(one, out[0])
    wide = torch.zeros((3, n + 11), dtype=torch.float32, device=DEV)
    wide[:, :n] = torch.from_numpy(batch)
    dst = torch.full((3, n + 5), 7.0, dtype=torch.float32, device=DEV)
    res = meter.normalize(wide[:, :n], out=dst[:, :n])
    assert res.is_cuda and res.data_ptr() == dst.data_ptr() and np.array_equal(dst[:, :n].cpu().numpy(), out) and bool((dst[:, n:] == 7.0).all())
    # an out that is wrong in device, dtype, shape or overlap is refused
    for bad in (torch.zeros((3, n)), torch.zeros((3, n), dtype=torch.float64, device=DEV), torch.zeros((2, n), device=DEV),
                torch.zeros((3, n + 1), device=DEV), torch.zeros((n, 3), device=DEV).t(), torch.zeros(n, device=DEV)[None].expand(3, n),
                wide[:, 5:n + 5], wide[:, :n]):
        with pytest.raises(ValueError):
            meter.normalize(wide[:, :n], out=bad)


def test_peak_mode():
    rate, n = 16000, 8000
    rows = np.stack([_steady(n, 5, -30.0), np.zeros(n, np.float32), _steady(n, 6, -1.0)])
    for kw in ({}, dict(headroom_db=3.0)):
        meter = _meter(rate, mode="peak", **kw)
        gains, out = meter.gains(rows), meter.normalize(rows)
        stats, counts = meter.measure(rows)
        for b in range(3):
            sp = float(np.abs(rows[b].astype(np.float64)).max())
            want, flags = ul.gain_of(dict(sample_peak=sp), mode="peak", headroom_db=kw.get("headroom_db", 0.1))
            assert stats[b, 2] == sp and _ulps(gains[b], want) <= 1 and counts[b, 3] == flags, (b, gains[b], want)
        assert np.array_equal(out.view(np.uint32), (rows * gains[:, None]).view(np.uint32)) and gains[1] == 1.0
        assert abs(20.0 * np.log10(np.abs(out[0]).max()) + kw.get("headroom_db", 0.1)) < 1e-5


def test_same_bits_twice_in_a_batch_alone_and_from_a_graph():
    import torch
    rate = 16000
    g = loudness.geometry(loudness.make_cfg(rate))
    n = 2 * g["tile"] + 777
    rows = np.stack([ul.ramp_noise(n, rate, 40 + b) for b in range(3)])
    meter = _meter(rate)
    first = _call(meter, rows)
    second = _call(meter, rows)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    for b in range(3):
        alone = _call(meter, rows[b:b + 1])
        for a, c in zip(first, alone):
            assert a[b].tobytes() == c[0].tobytes(), b
    other = _call(meter, np.stack([rows[2], _steady(n, 9, -12.0), rows[0]]))
    for a, c in zip(first, other):
        assert a[0].tobytes() == c[2].tobytes() and a[2].tobytes() == c[0].tobytes()
    # a captured graph replays the eager bits, also on new content in the same buffers
    x = torch.from_numpy(rows).to(DEV)
    lengths = torch.tensor([n, g["block"] + 3, n - 1], dtype=torch.int64, device=DEV)
    out = torch.empty_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        meter.normalize(x, lengths=lengths, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stats, counts = meter.measure(x, lengths=lengths)
        meter.normalize(x, lengths=lengths, out=out)
    for content in (rows, rows[::-1].copy()):
        x.copy_(torch.from_numpy(content))
        graph.replay()
        torch.cuda.synchronize()
        got = (stats.cpu().numpy(), counts.cpu().numpy(), out.cpu().numpy())
        e_stats, e_counts = meter.measure(x, lengths=lengths)
        e_out = meter.normalize(x, lengths=lengths)
        for a, b in zip(got, (e_stats.cpu().numpy(), e_counts.cpu().numpy(), e_out.cpu().numpy())):
            assert a.tobytes() == b.tobytes()
    assert np.isfinite(got[0][:, 0]).all() and got[1][1, 0] == 1


def _wav_bytes(x, rate):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(x, dtype="<i2").tobytes())
    return buf.getvalue()


def test_read_clips_normalize():
    import torch
    from multilingual_kws.embedding import input_data
    files = [_wav_bytes(ul.ramp_noise(16000, 16000, 50, np.int16, lo_db=-40.0, hi_db=-20.0), 16000),
             _wav_bytes(ul.ramp_noise(9000, 16000, 51, np.int16, lo_db=-30.0, hi_db=-10.0), 16000),
             _wav_bytes(ul.ramp_noise(5600, 8000, 52, np.int16, lo_db=-50.0, hi_db=-25.0), 8000),
             _wav_bytes(ul.ramp_noise(20000, 16000, 53, np.int16, lo_db=-12.0, hi_db=-2.0), 16000)]
    own = [16000, 9000, 11200, 16000]
    plain = input_data.read_clips(files)
    assert plain.shape == (4, 16000) and plain.dtype == torch.float32
    opts = dict(target_lufs=-20.0, true_peak_db=-2.0)
    levelled = input_data.read_clips(files, normalize=opts)
    assert torch.equal(levelled, input_data.normalize_loudness(input_data.read_clips(files), lengths=own, **opts))
    assert torch.equal(input_data.read_clips(files, normalize={}), input_data.normalize_loudness(plain, lengths=own))
    # the keyword left out, or None, is the function of before: the same bits as the single-file readers give
    assert torch.equal(plain, input_data.read_clips(files, normalize=None)) and torch.equal(plain, input_data.read_clips(files))
    for i in (0, 1, 3):
        assert np.array_equal(plain[i].cpu().numpy().view(np.uint32), input_data.decode_wav(files[i], 16000)[0].view(np.uint32)), i
    # the zero padding counts for nothing: a row reads what its own samples read, and the padding stays zero
    stats, counts = input_data.measure_loudness(plain, lengths=own)
    for i in range(4):
        alone, _ = input_data.measure_loudness(plain[i, :own[i]].contiguous())
        assert stats[i].cpu().numpy().tobytes() == alone.cpu().numpy().tobytes(), i
        assert not levelled[i, own[i]:].any()
    again, _ = input_data.measure_loudness(levelled, lengths=own)
    assert int(counts[1, 0]) == 2 and abs(float(again[0, 0]) + 20.0) < 0.5 and float(again[3, 1]) <= 10.0 ** (-2.0 / 20.0) * (1 + 1e-5)
    assert input_data.measure_loudness(plain.cpu().numpy(), lengths=own)[0].dtype == np.float64
