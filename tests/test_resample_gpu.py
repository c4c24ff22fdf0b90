"""mkws_resample_forward on the device: every case bit-equal to the float32 restatement of the specification (tests/util_resample.py)
and within (T + 1) * 2^-24 * sum_j |tab * x| of its float64 form."""
import ctypes

import numpy as np
import pytest

from multilingual_kws_amd import _lib, resample
from tests.util_resample import _around_tile, _check, noise_f32, noise_i16, polyphase

pytestmark = pytest.mark.gpu
RATES = (48000, 44100, 8000)          # L = 1; L = 160, M = 441; up by 2
TILE = 1024                           # outputs of one workgroup (mkws_resample.hip)
GUARD = 12345.0


@pytest.fixture(scope="module")
def handles():
    hs = {r: resample.Resampler(r) for r in RATES}
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("rate", RATES)
def test_forward_equals_the_emulator(handles, rate, dtype):
    """Lengths 1, T - 1, T, three seconds and seven samples, and one output each side of a multiple of the tile; centred and causal; one row
    and three rows whose strides are larger than the rows; guard words around every output row."""
    import torch
    rs = handles[rate]
    T = rs.geometry["T"]
    make = noise_f32 if dtype == "float32" else noise_i16
    lengths = [1, T - 1, T, 3 * 16000 + 7] + _around_tile(rs, TILE) + _around_tile(rs, 2 * TILE)
    for n in lengths:
        for B in (1, 3):
            n_out = rs.out_samples(n)
            host = np.stack([make(n + 13, 100 * n + b) for b in range(B)])
            d_in = torch.from_numpy(host).cuda()
            for centred in (True, False):
                buf = torch.full((B, n_out + 11), GUARD, dtype=torch.float32, device="cuda")
                got = rs.forward(d_in[:, 2:2 + n], centred=centred, out=buf[:, 4:4 + n_out])
                assert got.data_ptr() == buf[:, 4:].data_ptr()
                back = buf.cpu().numpy()
                assert (back[:, :4] == GUARD).all() and (back[:, 4 + n_out:] == GUARD).all()
                _check(rs, host[:, 2:2 + n], back[:, 4:4 + n_out], centred)


def test_forward_kinds(handles):
    """numpy in -> numpy out, [n] -> [n_out], CPU tensor -> CPU tensor, CUDA tensor -> CUDA tensor; float32 and int16 holding the same values
    give the same bits; empty in -> empty out."""
    import torch
    rs = handles[48000]
    pcm = noise_i16(3001, 5)
    as_f32 = pcm.astype(np.float32) / np.float32(32768)
    a = rs.forward(pcm)
    b = rs.forward(as_f32)
    assert isinstance(a, np.ndarray) and a.shape == (1001,) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c = rs.forward(torch.from_numpy(as_f32))
    assert torch.is_tensor(c) and not c.is_cuda and np.array_equal(c.numpy(), a)
    d = rs.forward(torch.from_numpy(np.stack([as_f32, as_f32])).cuda(), centred=False)
    assert d.is_cuda and d.shape == (2, 1001) and torch.equal(d[0], d[1])
    assert rs.forward(np.zeros((2, 0), np.float32)).shape == (2, 0) and rs.forward(np.zeros(0, np.int16)).shape == (0,)
    with pytest.raises(TypeError):
        rs.forward(np.zeros(8, np.float64))
    assert rs.delay_ms == 2.0 and handles[44100].delay_ms == 2.0 and handles[8000].delay_ms == 4.0


def test_non_default_stream(handles):
    import torch
    rs = handles[44100]
    x = noise_f32(20000, 77)
    d_in = torch.from_numpy(x).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = rs.forward(d_in, centred=True)
        done = torch.cuda.Event()
        done.record(side)
    done.synchronize()
    _check(rs, [x], [got.cpu().numpy()], True)


def test_long_recording_64_bit_index(handles):
    """Five minutes of 44.1 kHz audio in one launch: compared where n * M crosses 2^31 and at the end of the row."""
    import torch
    rs = handles[44100]
    g, tab = rs.geometry, rs.taps()
    n_in = 13_500_000
    x = noise_f32(n_in, 2024)
    n_out = rs.out_samples(n_in)
    cross = 2 ** 31 // g["M"]
    assert abs(cross - 4_869_600) < 100 and cross + 4096 < n_out - 4096
    ns = np.concatenate([np.arange(cross - 4096, cross + 4096), np.arange(n_out - 4096, n_out)])
    got = rs.forward(torch.from_numpy(x).cuda(), centred=True)
    assert got.shape == (n_out,)
    got = got[torch.from_numpy(ns).cuda()].cpu().numpy()
    want = polyphase(x, tab, g["M"], g["half"], np.float32, ns=ns)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    exact, mag = polyphase(x, tab, g["M"], g["half"], np.float64, ns=ns, want_abs=True)
    assert np.all(np.abs(got - exact) <= (g["T"] + 1) * 2.0 ** -24 * mag)


def test_refusals_with_a_handle(handles):
    import torch
    rs, L = handles[48000], _lib.lib()
    INVALID, UNSUPPORTED = -1, -2
    d_in, d_out = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    pi, po, st = ctypes.c_void_p(d_in.data_ptr()), ctypes.c_void_p(d_out.data_ptr()), _lib.current_stream_ptr()
    assert L.mkws_resample_forward(rs.h, None, 0, 1, 30, 30, 1, po, 10, st) == INVALID
    assert L.mkws_resample_forward(rs.h, pi, 0, 1, 30, 30, 1, None, 10, st) == INVALID
    assert L.mkws_resample_forward(rs.h, pi, 0, -1, 30, 30, 1, po, 10, st) == INVALID
    assert L.mkws_resample_forward(rs.h, pi, 0, 1, -30, 30, 1, po, 10, st) == INVALID
    assert L.mkws_resample_forward(rs.h, pi, 0, 2, 30, 29, 1, po, 10, st) == INVALID
    assert L.mkws_resample_forward(rs.h, pi, 0, 2, 30, 30, 1, po, 9, st) == INVALID
    assert L.mkws_resample_forward(rs.h, None, 0, 0, 30, 30, 1, None, 10, st) == 0       # B == 0, n_in == 0: nothing launched
    assert L.mkws_resample_forward(rs.h, None, 0, 2, 0, 0, 1, None, 0, st) == 0
    need = L.mkws_resample_live_state_bytes(rs.h)
    assert need == (8 + 4 * (rs.geometry["T"] - 1) + 7) // 8 * 8
    states = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
    ps = ctypes.c_void_p(states.data_ptr())
    audio, out = torch.zeros(960, device="cuda"), torch.zeros(320, device="cuda")
    pa, pout = ctypes.c_void_p(audio.data_ptr()), ctypes.c_void_p(out.data_ptr())
    assert L.mkws_resample_live_push_many(rs.h, ps, need - 8, 1, None, pa, 0, 320, pout, st) == INVALID
    assert L.mkws_resample_live_push_many(rs.h, ps, need + 4, 1, None, pa, 0, 320, pout, st) == INVALID
    assert L.mkws_resample_live_push_many(rs.h, None, need, 1, None, pa, 0, 320, pout, st) == INVALID
    assert L.mkws_resample_live_push_many(rs.h, ps, need, 1, None, None, 0, 320, pout, st) == INVALID
    assert L.mkws_resample_live_push_many(rs.h, ps, need, 1, None, pa, 0, 320, None, st) == INVALID
    assert L.mkws_resample_live_push_many(rs.h, ps, need, -1, None, pa, 0, 320, pout, st) == INVALID
    assert L.mkws_resample_live_push_many(rs.h, ps, need, 1, None, pa, 0, -320, pout, st) == INVALID
    assert L.mkws_resample_live_push_many(rs.h, None, need, 0, None, None, 0, 320, None, st) == 0
    torch.cuda.synchronize()
    assert not states.any() and not out.any()
    assert [handles[r].live_in_samples(320) for r in RATES] == [960, 882, 160]
    odd = resample.Resampler(11025)
    assert L.mkws_resample_live_in_samples(odd.h, 320) == UNSUPPORTED and odd.live_in_samples(640) == 441
    with pytest.raises(ValueError, match="not a whole number"):
        odd.live_in_samples(320)
    odd.close()
    far = resample.make_cfg(16000 * 40, 16000)           # M / L = 40: one tile's input span does not fit the LDS
    h = ctypes.c_void_p()
    assert L.mkws_resample_create(ctypes.byref(far), ctypes.byref(h)) == UNSUPPORTED and not h.value
