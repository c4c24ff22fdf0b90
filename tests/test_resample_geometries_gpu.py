"""The resampler's two kernels at every geometry of tests/resample_cases.py -- the history longer than the workgroup, the largest LDS
requests, L == 1 with M = 1, 2, 6, 12, L > 1 with L small, L = 320, L = 640 > M and L above one tile, and filters other than the default
-- against the emulator of tests/util_resample.py on the handle's own taps: bit-equal to its float32 form, within
(T + 1) * 2^-24 * sum_j |tab * x| of its float64 form.  The live kernel is compared with the emulator itself, not with the device's own
batch form, and the state block is read back and compared byte for byte with the input the header says it holds.

Every buffer is fenced (canary word and band width of tests/util_train_ops.py, buffers of tests/util_fenced.py): an input row sits
between bands, and between gaps where the stride is longer than the row, that poison a result computed from them (the canary NaN for
float32, -32768 for int16); an output row and a state block sit in canary-filled allocations whose bands and gaps must keep the canary."""
import ctypes

import numpy as np
import pytest

from multilingual_kws_amd import _lib, resample
from tests import resample_cases as cases
from tests.util_resample import _around_tile, _check, noise_f32, noise_i16, polyphase
from util_fenced import PAD, FencedBuffer, canary_array, holds_canary

pytestmark = pytest.mark.gpu
DEV = "cuda"
UNSUPPORTED = -2
OUT = cases.RATE_OUT
PUSHES = cases.PUSHES
GAP_WORDS = 2                          # the state stride exceeds live_state_bytes by 16 bytes


@pytest.fixture(scope="module")
def handles():
    """name -> (handle, its taps), built once and closed at the end."""
    hs = {}
    for name, rate, over in cases.ALL_CASES:
        rs = resample.Resampler(rate, OUT, **over)
        hs[name] = (rs, rs.taps())
    yield hs
    for rs, _ in hs.values():
        rs.close()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _as_f32(x):
    return x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x


# -- fenced buffers ---------------------------------------------------------------------------------------------------------------------

class _Input:
    """Rows [B, n] of float32 or int16 at `stride` elements in one allocation [band | rows and gaps | band].  float32: a FencedBuffer,
    every word outside the rows the canary NaN.  int16 (no buffer type of tests/util_fenced.py): an allocation of the same band bytes
    whose every sample outside the rows is -32768."""

    def __init__(self, rows, stride):
        import torch
        B, n = rows.shape
        span = (B - 1) * stride + n
        if rows.dtype == np.float32:
            self.buf = FencedBuffer(span, "float32", device=DEV)
            self.whole, mid = self.buf.whole, self.buf.mid
        else:
            assert rows.dtype == np.int16
            band = 2 * PAD
            self.whole = torch.full((band + span + band,), -32768, dtype=torch.int16, device=DEV)
            mid = self.whole[band:band + span]
        self.view = mid.as_strided((B, n), (stride, 1))
        self.load(rows)

    def load(self, rows):
        import torch
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
        self.snap = self.whole.clone()

    def unchanged(self):
        import torch
        return torch.equal(self.whole, self.snap)


class _Output:
    """float32 rows [B, n] at `stride` inside a canary-filled FencedBuffer."""

    def __init__(self, B, n, stride):
        self.B, self.n, self.stride = B, n, stride
        self.buf = FencedBuffer((B - 1) * stride + n, "float32", device=DEV)
        self.view = self.buf.mid.as_strided((B, n), (stride, 1))

    def reset(self):
        self.buf.reset()

    def rows(self, active=None):
        """The rows on the host, after: both bands and every gap still hold the canary, and so does every row that is not `active`."""
        assert self.buf.pads_intact(), "a band of the output was written"
        h = self.buf.host()
        inside = np.zeros(h.size, bool)
        for b in range(self.B):
            if active is None or active[b]:
                inside[b * self.stride:b * self.stride + self.n] = True
        assert holds_canary(h[~inside]).all(), "the output was written outside the rows of the active streams"
        return np.stack([h[b * self.stride:b * self.stride + self.n] for b in range(self.B)])


class _State:
    """S zero-filled state blocks at a stride of GAP_WORDS more int64 words than a block, inside a canary-filled FencedBuffer."""

    def __init__(self, rs, S):
        need = rs.L.mkws_resample_live_state_bytes(rs.h)
        assert need == (8 + 4 * (rs.geometry["T"] - 1) + 7) // 8 * 8
        self.S, self.words, self.stride = S, need // 8, need // 8 + GAP_WORDS
        start = canary_array(((S - 1) * self.stride + self.words,), np.int64)
        for s in range(S):
            start[s * self.stride:s * self.stride + self.words] = 0
        self.buf = FencedBuffer(start.size, "int64", fill=start, device=DEV)
        self.view = self.buf.mid.as_strided((S, self.words), (self.stride, 1))

    def blocks(self):
        """The blocks on the host, after: both bands and the gaps between the blocks still hold the canary."""
        assert self.buf.pads_intact(), "a band of the state was written"
        h = self.buf.host()
        inside = np.zeros(h.size, bool)
        for s in range(self.S):
            inside[s * self.stride:s * self.stride + self.words] = True
        assert holds_canary(h[~inside]).all(), "the gap between two state blocks was written"
        return [h[s * self.stride:s * self.stride + self.words].copy() for s in range(self.S)]


def _check_state(T, block, fed):
    """include/mkws.h: the int64 count of input samples pushed, then the last T - 1 input samples as float32 (int16: s / 32768), oldest
    first; +0.0 before the start of a stream shorter than that.  fed: everything the stream has been pushed so far."""
    n, H = len(fed), T - 1
    assert int(block[0]) == n, (int(block[0]), n)
    want = np.zeros(H, np.float32)
    k = min(H, n)
    if k:
        want[H - k:] = _as_f32(fed[n - k:])
    got = block[1:].view(np.float32)[:H]
    assert got.tobytes() == want.tobytes(), (n, H, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


# -- a. the batch kernel ------------------------------------------------------------------------------------------------------------------

def _batch_compare(rs, tab, lengths, dtype, centred, batches):
    make = noise_f32 if dtype == "float32" else noise_i16
    for n in lengths:
        n_out = rs.out_samples(n)
        for B in batches:
            rows = np.stack([make(n, 1000 * n + 10 * B + b) for b in range(B)])
            src = _Input(rows, n + 5)                                # (B > 1: a stride longer than the row)
            dst = _Output(B, n_out, n_out + 3)
            got = rs.forward(src.view, centred=centred, out=dst.view)
            assert got.data_ptr() == dst.view.data_ptr()
            back = dst.rows()
            assert src.unchanged()
            _check(rs, rows, back, centred, tab)


def _batch_lengths(rs):
    T = rs.geometry["T"]
    return sorted({1, T - 1, T} | set(_around_tile(rs, cases.TILE)) | set(_around_tile(rs, 2 * cases.TILE)))


@pytest.mark.parametrize("centred", [True, False], ids=["centred", "causal"])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("name", cases.NAMES)
def test_batch_equals_the_emulator(handles, name, dtype, centred):
    """Lengths 1, T - 1, T and one output each side of one tile and of two; one row, and three rows whose strides are longer than the rows."""
    rs, tab = handles[name]
    _batch_compare(rs, tab, _batch_lengths(rs), dtype, centred, (1, 3))


# -- c, d. the live kernel against the emulator, and the state against the input ----------------------------------------------------------

def _live_pass(rs, xs, out_samples):
    """xs [S, PUSHES * in_samples] pushed in PUSHES pushes, every buffer fenced -> the concatenated outputs [S, PUSHES * out_samples] and
    the state blocks after every push [PUSHES][S]."""
    S, n_in = xs.shape[0], rs.live_in_samples(out_samples)
    assert xs.shape[1] == PUSHES * n_in
    state, src, dst = _State(rs, S), _Input(xs[:, :n_in], n_in), _Output(S, out_samples, out_samples)
    outs, blocks = [], []
    for i in range(PUSHES):
        src.load(xs[:, i * n_in:(i + 1) * n_in])
        dst.reset()
        got = rs.live_push_many(state.view, src.view, out_samples, out=dst.view)
        assert got.data_ptr() == dst.view.data_ptr()
        outs.append(dst.rows())
        assert src.unchanged()
        blocks.append(state.blocks())
    return np.concatenate(outs, axis=1), blocks


def _live_run(rs, tab, seed):
    """Pushes of the smallest multiple of L that is at least a hop, of four times that (more than one tile), and -- where it brings fewer
    new samples than the state keeps -- of the smallest legal push: a float32 stream and int16's values as float32 side by side, then the
    int16 stream itself.  -> [(what, out_samples, input [n], emulator output [PUSHES * out_samples], device output, blocks [PUSHES])]."""
    g = rs.geometry
    L, M, T = g["L"], g["M"], g["T"]
    out1, short = cases.live_out_samples(L), cases.short_out_samples(L, M, T)
    n_long = PUSHES * 4 * out1 * M // L
    xf, pcm = noise_f32(n_long, seed), noise_i16(n_long, seed + 1)
    pf = _as_f32(pcm)
    want = [polyphase(x, tab, M, 0, np.float32) for x in (xf, pf)]               # causal: a shorter stream's outputs are a prefix of these
    assert want[0].shape == (PUSHES * 4 * out1,)
    ns = np.arange(2048)
    for x, w in zip((xf, pf), want):
        exact, mag = polyphase(x, tab, M, 0, np.float64, ns=ns, want_abs=True)
        assert np.all(np.abs(w[:2048] - exact) <= (T + 1) * 2.0 ** -24 * mag)
    runs = []
    for out in [out1, 4 * out1] + ([short] if short else []):
        n_in = rs.live_in_samples(out)
        assert n_in == out * M // L and (short is None or out != short or n_in < T - 1)
        n = PUSHES * n_in
        got, blocks = _live_pass(rs, np.stack([xf[:n], pf[:n]]), out)
        runs.append(("float32", out, xf[:n], want[0][:PUSHES * out], got[0], [b[0] for b in blocks]))
        runs.append(("int16's values as float32", out, pf[:n], want[1][:PUSHES * out], got[1], [b[1] for b in blocks]))
        got, blocks = _live_pass(rs, pcm[None, :n], out)
        runs.append(("int16", out, pcm[:n], want[1][:PUSHES * out], got[0], [b[0] for b in blocks]))
    return runs


def _outputs_equal_the_emulator(runs):
    for what, out, _, want, got, _ in runs:
        assert _same_bits(got, want), (what, out, int((got != want).sum()))


def _states_hold_the_input(T, runs):
    for what, out, x, _, _, blocks in runs:
        n_in = len(x) // PUSHES
        for i, block in enumerate(blocks):
            _check_state(T, block, x[:(i + 1) * n_in])


@pytest.fixture(scope="module")
def live_runs(handles):
    """name -> the runs of that case, made by the first of the two tests below that asks."""
    done = {}

    def get(name):
        if name not in done:
            rs, tab = handles[name]
            done[name] = _live_run(rs, tab, 50 + rs.geometry["T"])
        return done[name]
    return get


@pytest.mark.parametrize("name", cases.ALL_NAMES)
def test_live_pushes_equal_the_emulator(live_runs, name):
    """Twelve pushes, concatenated, are the first samples of the float32 emulator's causal output over the stream's whole input, bit for
    bit; int16 and the same values as float32 give the same bits."""
    _outputs_equal_the_emulator(live_runs(name))


@pytest.mark.parametrize("name", cases.ALL_NAMES)
def test_live_state_holds_the_input(handles, live_runs, name):
    """After every push of the same runs the state block holds the count and the last T - 1 input samples, byte for byte."""
    _states_hold_the_input(handles[name][0].geometry["T"], live_runs(name))


# -- b. the largest geometry create accepts -------------------------------------------------------------------------------------------------

def test_the_largest_geometry_create_accepts_launches():
    """rate_in = 16000 * k with the default filter, k = 1 .. 40: the accepted k are a prefix, every refusal is MKWS_ERR_UNSUPPORTED with a
    NULL handle, and the last accepted one -- the largest dynamic LDS request the library makes -- runs both kernels."""
    L = _lib.lib()
    accepted = []
    for k in range(1, 41):
        cfg, h = resample.make_cfg(OUT * k, OUT), ctypes.c_void_p()
        rc = L.mkws_resample_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc == 0:
            assert h.value
            L.mkws_resample_destroy(h)
            accepted.append(k)
        else:
            assert rc == UNSUPPORTED and not h.value, (k, rc)
    k_max = len(accepted)
    print("k_max", k_max)
    assert accepted == list(range(1, k_max + 1)) and 12 <= k_max < 40
    rs = resample.Resampler(OUT * k_max)
    try:
        tab, g = rs.taps(), rs.geometry
        print("T", g["T"], "live LDS bytes", 4 * ((1023 * g["M"]) // g["L"] + 2 * g["T"] - 1))
        for dtype in ("float32", "int16"):
            for centred in (True, False):
                _batch_compare(rs, tab, _around_tile(rs, cases.TILE), dtype, centred, (2,))
        runs = _live_run(rs, tab, 7)
        _outputs_equal_the_emulator(runs)
        _states_hold_the_input(g["T"], runs)
    finally:
        rs.close()


# -- e. streams beside each other ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["down6", "cd_quarter"])
def test_three_streams_with_a_changing_mask(handles, name):
    """An active stream gets the next samples of its own emulator output and its state holds its own input; an inactive one keeps its
    state bytes and its canary output row, and its input row, filled with NaN, is never read."""
    import torch
    rs, tab = handles[name]
    g = rs.geometry
    out, S, N = cases.live_out_samples(g["L"]), 3, 8
    n_in = rs.live_in_samples(out)
    xs = [noise_f32(N * n_in, 30 + s) for s in range(S)]
    want = [polyphase(x, tab, g["M"], 0, np.float32) for x in xs]
    state, src, dst = _State(rs, S), _Input(np.zeros((S, n_in), np.float32), n_in), _Output(S, out, out)
    at, sat_out = [0] * S, [0] * S
    for i in range(14):
        on = [int(i % 2 == 0 or i > 6), int(i % 3 != 1), int(i >= 3 and i != 6)]
        on = [int(o and at[s] < N) for s, o in enumerate(on)]
        if not any(on):
            continue
        rows = np.full((S, n_in), np.nan, np.float32)
        for s in range(S):
            if on[s]:
                rows[s] = xs[s][at[s] * n_in:(at[s] + 1) * n_in]
        src.load(rows)
        dst.reset()
        before = state.blocks()
        rs.live_push_many(state.view, src.view, out, active=torch.tensor(on, dtype=torch.int32, device=DEV), out=dst.view)
        got, after = dst.rows(active=on), state.blocks()
        assert src.unchanged()
        for s in range(S):
            if on[s]:
                assert _same_bits(got[s], want[s][at[s] * out:(at[s] + 1) * out]), (i, s)
                at[s] += 1
                _check_state(g["T"], after[s], xs[s][:at[s] * n_in])
            else:
                assert after[s].tobytes() == before[s].tobytes(), (i, s)
                sat_out[s] += int(0 < at[s] < N)
    assert at == [N] * S and min(sat_out) >= 1                        # every stream sat out a push in the middle of its audio


# -- f. whole-number pushes -----------------------------------------------------------------------------------------------------------------

def test_whole_number_pushes(handles):
    lib = _lib.lib()
    for name, rate, _ in cases.ALL_CASES:
        rs, _ = handles[name]
        L, M = rs.geometry["L"], rs.geometry["M"]
        assert (L, M) == cases.factors(rate)
        for k in (0, 1, 2, 7, -(-cases.HOP // L)):
            assert lib.mkws_resample_live_in_samples(rs.h, k * L) == k * M == rs.live_in_samples(k * L), (name, k)
        if L > 1:
            assert lib.mkws_resample_live_in_samples(rs.h, L + 1) == UNSUPPORTED, name
            with pytest.raises(ValueError, match="not a whole number"):
                rs.live_in_samples(L + 1)
        hops = next(h for h in range(1, L + 1) if (cases.HOP * h * M) % L == 0)
        assert resample.live_push_hops(rate, OUT, cases.HOP) == hops, name
        assert rs.live_in_samples(cases.HOP * hops) == cases.HOP * hops * M // L


# -- the alignment of the centred form ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.DEFAULT_FILTER_NAMES)
def test_tone_alignment_on_the_device(handles, name):
    """test_resample_entry_gpu.py's check at 48 kHz, at every default-filter geometry: a 1 kHz tone of 0.1 s comes back as the same
    tone, sample for sample, within 1e-4 away from the ends (test_resample_cpu.py: why the other filters are left out)."""
    rs, _ = handles[name]
    n_in = -(-rs.rate_in // 10)
    tone = (0.5 * np.sin(2 * np.pi * 1000 * np.arange(n_in) / rs.rate_in)).astype(np.float32)
    got = rs.forward(tone, centred=True)
    assert isinstance(got, np.ndarray) and got.shape == (rs.out_samples(n_in),) and got.size >= 1600
    err = np.abs(got[200:1400] - 0.5 * np.sin(2 * np.pi * 1000 * np.arange(200, 1400) / OUT)).max()
    print(name, "tone error", err)
    assert err < 1e-4
