"""mkws_pcm_decode against the numpy restatement of include/mkws.h's rule (tests/util_pcm.py), bit for bit (uint32 views): every
format, channel counts 1 / 2 / 3 / 8, byte offsets of every alignment, frame counts on both sides of a tile, padding and truncation,
the mix, the kernel's own refusal of bad items, and a byte offset above 2^31."""
import ctypes

import numpy as np
import pytest

from multilingual_kws_amd import _lib, pcm
from tests import util_pcm as up

pytestmark = pytest.mark.gpu
GUARD = 0xDEADBEEF
TILE = 1024                                              # outputs of one workgroup (mkws_pcm.hip)
FRAMES = [0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1]
OFFSETS = [0, 1, 2, 3, 44 + 1]


def _samples(fmt, frames, channels, rng):
    """Random sample bytes: every code of the integer formats, normal numbers for the float ones (NaN payloads through an add and
    results below the smallest normal float are not pinned by the specification)."""
    if fmt in ("f32", "f64"):
        return up.encode(fmt, rng.uniform(-1.5, 1.5, (frames, channels)))
    return rng.integers(0, 256, frames * channels * up.SAMPLE_BYTES[fmt], dtype=np.uint8).tobytes()


def _want_row(fmt, channels, data, n_frames, out_len, channel):
    v = up.decode_frames(fmt, channels, data[:n_frames * channels * up.SAMPLE_BYTES[fmt]], channel)
    row = np.zeros(out_len, np.float32)
    m = min(n_frames, out_len)
    row[:m] = v[:m]
    return row.view(np.uint32)


def _launch(buf, rows, out_floats, max_out_len=None, skew=0):
    """buf: bytes -> (the whole output as uint32 with GUARD wherever nothing was written, the kernel's count of refused items).  The host
    check is off: the kernel's own is what runs.  skew: the device buffer starts that many bytes past a 16-byte boundary."""
    import torch
    host = np.concatenate([np.zeros(skew, np.uint8), np.frombuffer(buf, np.uint8)])
    d = torch.from_numpy(host).cuda()[skew:]
    out = torch.full((out_floats,), GUARD - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32)
    got, bad = pcm.decode_on_device(d, pcm.make_items(rows), out=out, max_out_len=max_out_len, validate=False, check=False)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy().view(np.uint32), int(bad.cpu()[0])


class _Table:
    """Items laid out over one byte buffer and one output with a guard word in front of, between and behind the rows."""

    def __init__(self):
        self.buf, self.rows, self.want, self.at = bytearray(), [], [np.full(1, GUARD, np.uint32)], 1

    def add(self, fmt, channels, data, n_frames, out_len, channel, byte_offset):
        """The frames `data` placed so that they start at a byte whose offset is byte_offset modulo 16."""
        while len(self.buf) % 16 != byte_offset % 16:
            self.buf.append(0xA5)
        self.rows.append((len(self.buf), n_frames, self.at, out_len, fmt, channels, channel))
        self.buf += data
        self.want += [_want_row(fmt, channels, data, n_frames, out_len, channel), np.full(1, GUARD, np.uint32)]
        self.at += out_len + 1

    def check(self, skew=0):
        got, bad = _launch(bytes(self.buf), self.rows, self.at, skew=skew)
        want = np.concatenate(self.want)
        assert bad == 0
        if not np.array_equal(got, want):
            k = int(np.nonzero(got != want)[0][0])
            item = max(i for i, r in enumerate(self.rows) if r[2] - 1 <= k)
            raise AssertionError(f"float {k} differs (item {item}: {self.rows[item]}): got {got[k]:#x}, want {want[k]:#x}")


@pytest.mark.parametrize("fmt", up.FORMATS)
def test_shapes(fmt):
    """Every frame count x channel count, with the byte offset, the channel and the output length rotating through their values, three
    times with different rotations; the buffer ends with the last item's last byte."""
    rng = np.random.default_rng(up.FORMATS.index(fmt))
    t, idx = _Table(), 0
    for turn in range(3):
        for nf in FRAMES:
            for channels in (1, 2, 3, 8):
                channel = [0, channels - 1, "mix"][(idx + turn) % 3]
                out_len = [max(nf - 3, 0), nf, nf + 5, 0, nf + TILE][(idx // 3 + turn) % 5]
                t.add(fmt, channels, _samples(fmt, nf, channels, rng), nf, out_len, channel, OFFSETS[(idx + 2 * turn) % 5])
                idx += 1
    t.check()


@pytest.mark.parametrize("skew", [1, 7, 12])
def test_mixed_table_and_a_base_off_the_16_byte_grid(skew):
    """One launch whose table mixes all eight formats and several channel counts, guards around every row; the byte buffer itself starts
    off the 16-byte grid, so the first staged word of the first item would begin in front of the buffer."""
    rng = np.random.default_rng(100 + skew)
    t = _Table()
    plan = [("s16", 1, 700, 700, 0, 0), ("u8", 2, 300, 310, 1, 1), ("s24", 3, 1025, 1025, "mix", 3), ("s32", 8, 257, 200, 7, 2),
            ("f32", 2, 1500, 1500, "mix", 45), ("f64", 3, 683, 690, 2, 1), ("mulaw", 1, 2049, 2049, 0, 3), ("alaw", 2, 255, 255, "mix", 0),
            ("s24", 1, 5, 9, 0, 2), ("s16", 8, 1024, 1024, "mix", 1), ("f64", 8, 513, 513, 5, 3), ("u8", 1, 0, 7, 0, 0)]
    for fmt, channels, nf, out_len, channel, bo in plan:
        t.add(fmt, channels, _samples(fmt, nf, channels, rng), nf, out_len, channel, bo)
    t.check(skew=skew)


def test_all_codes_of_the_small_alphabets():
    codes = np.arange(256, dtype=np.uint8)
    t = _Table()
    for fmt in ("u8", "mulaw", "alaw"):
        t.add(fmt, 1, codes.tobytes(), 256, 256, 0, 1)
        # every code against every code in a two-channel mix
        pairs = np.stack([np.repeat(codes, 256), np.tile(codes, 256)], axis=1)
        t.add(fmt, 2, pairs.tobytes(), 65536, 65536, "mix", 3)
    t.check()


def test_edge_values():
    t = _Table()
    t.add("s16", 1, up.encode("s16", [-32768, 32767, -1, 0, 1]), 5, 5, 0, 1)
    t.add("s24", 1, up.encode("s24", [-8388608, 8388607, -1, 0, 1, 0x7FFF00, -0x7FFF01]), 7, 7, 0, 1)
    s32 = [-2 ** 31, 2 ** 31 - 1, -1, 0, 1, 16777217, -16777219, 16777216, 16777219, 2 ** 31 - 64, 2 ** 31 - 65, 2 ** 31 - 129]
    t.add("s32", 1, up.encode("s32", s32), len(s32), len(s32), 0, 2)
    want = up.decode_frames("s32", 1, up.encode("s32", s32), 0)
    assert want[1] == 1.0 and want[0] == -1.0 and want[5] == np.float32(16777216 * 2.0 ** -31) and want[6] == np.float32(-16777220 * 2.0 ** -31)
    # f64: a tie that must go to the even neighbour each way, +-0.0, the largest float, and one value that overflows to inf
    ties = [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24), 1.0 + 2.0 ** -24 + 2.0 ** -50, 0.0, -0.0,
            float(np.finfo(np.float32).max), 1e39, -1e39, 2.0 ** -126, 1.0 / 3.0]
    f64 = up.encode("f64", ties)
    t.add("f64", 1, f64, len(ties), len(ties), 0, 3)
    want = up.decode_frames("f64", 1, f64, 0)
    assert want[0] == 1.0 and want[1] == np.float32(1.0 + 2.0 ** -22) and want[3] == np.float32(1.0 + 2.0 ** -23)
    assert np.isposinf(want[7]) and np.isneginf(want[8]) and want.view(np.uint32)[5] == 0x80000000
    # f32: bit patterns pass through a chosen channel untouched -- NaN payloads, denormals, infinities, -0.0
    bits = np.asarray([0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x3F800000], "<u4")
    t.add("f32", 1, bits.tobytes(), len(bits), len(bits), 0, 1)
    t.add("f32", 2, np.stack([bits[::-1], bits], axis=1).tobytes(), len(bits), len(bits) + 2, 1, 2)
    assert np.array_equal(t.want[-2][:len(bits)], bits.astype(np.uint32))
    t.check()


def test_frames_wider_than_the_staging_buffer():
    """A frame above 16 KiB is read without staging: channel 0, the last channel and the mix over 2100 channels of f64."""
    rng = np.random.default_rng(5)
    t = _Table()
    for channel, bo in ((0, 1), (2099, 2), ("mix", 0)):
        t.add("f64", 2100, _samples("f64", 5, 2100, rng), 5, 8, channel, bo)
    t.check()


def test_byte_offset_above_2_to_31():
    import torch
    rng = np.random.default_rng(6)
    n_bytes = (1 << 31) + 4096
    d = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")
    data = _samples("s24", 113, 3, rng)                                  # 1017 bytes
    at = (1 << 31) + 3001                                                # odd, and the frames end 78 bytes before the buffer does
    d[at:at + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    rows = [(at, 113, 1, 120, "s24", 3, "mix"), (n_bytes - 16, 2, 122, 2, "f64", 1, 0), (at, 113, 125, 100, "s24", 3, 2)]
    out = torch.full((226,), GUARD - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32)
    pcm.decode_on_device(d, pcm.make_items(rows), out=out)
    want = np.concatenate([[GUARD], _want_row("s24", 3, data, 113, 120, "mix"), [GUARD], np.zeros(2, np.uint32), [GUARD],
                           _want_row("s24", 3, data, 113, 100, 2), [GUARD]]).astype(np.uint32)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    del d
    torch.cuda.empty_cache()


def test_invalid_items_write_nothing_and_are_counted():
    rng = np.random.default_rng(7)
    data = _samples("s16", 600, 2, rng)                                  # 2400 bytes
    n_bytes, out_floats, cap = len(data), 2000, 640
    good_a, good_b = (0, 600, 1, 610, "s16", 2, 1), (4, 500, 700, 500, "s16", 2, "mix")
    bad = [
        (n_bytes + 1, 0, 1300, 8, "s16", 2, 0),          # an offset past n_bytes
        (n_bytes - 3, 1, 1300, 8, "s16", 2, 0),          # its last frame ends one byte past n_bytes
        (-4, 1, 1300, 8, "s16", 2, 0),
        (1 << 62, 1 << 62, 1300, 8, "f64", 8, 0),        # sizes whose products do not fit 64 bits
        (0, 1 << 62, 1300, 8, "s16", 2, 0),              # more frames than 64-bit bytes
        (0, -1, 1300, 8, "s16", 2, 0),                   # a negative count
        (0, 10, 1300, -8, "s16", 2, 0),
        (0, 10, 1300, cap + 1, "s16", 2, 0),             # out_len > max_out_len
        (0, 10, 1300, 8, 8, 2, 0),                       # a bad format
        (0, 10, 1300, 8, -1, 2, 0),
        (0, 10, 1300, 8, "s16", 0, 0),                   # channels
        (0, 10, 1300, 8, "s16", -2, -1),
        (0, 10, 1300, 8, "s16", 2, 2),                   # a bad channel
        (0, 10, 1300, 8, "s16", 2, -2),
        (0, 10, out_floats - 7, 8, "s16", 2, 0),         # an output range past out_floats
        (0, 10, -1, 8, "s16", 2, 0),
        (0, 10, 1 << 62, 8, "s16", 2, 0),
    ]
    want = np.full(out_floats, GUARD, np.uint32)
    want[1:611] = _want_row("s16", 2, data, 600, 610, 1)
    want[700:1200] = _want_row("s16", 2, data[4:], 500, 500, "mix")
    for k, row in enumerate(bad):                        # one at a time between valid neighbours
        got, n_bad = _launch(data, [good_a, row, good_b], out_floats, max_out_len=cap)
        assert n_bad == 1 and np.array_equal(got, want), (k, row)
    rows = [good_a] + bad[:8] + [good_b] + bad[8:]       # and all of them in one table
    got, n_bad = _launch(data, rows, out_floats, max_out_len=cap)
    assert n_bad == len(bad) and np.array_equal(got, want)
    # the wrapper raises on the count, and its host check names the item before anything is launched
    import torch
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    with pytest.raises(ValueError, match="refused 1 of 3 items"):
        pcm.decode_on_device(d, pcm.make_items([good_a, bad[1], good_b]), out_floats=out_floats, max_out_len=cap, validate=False)
    with pytest.raises(ValueError, match="pcm item 1"):
        pcm.decode_on_device(d, pcm.make_items([good_a, bad[1], good_b]), out_floats=out_floats, max_out_len=cap)


def test_nothing_to_do_launches_nothing():
    import torch
    L = _lib.lib()
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.full((16,), 3.5, dtype=torch.float32, device="cuda")
    flag = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    items = torch.from_numpy(pcm.make_items([(0, 4, 0, 0, "s16", 1, 0)]).view(np.uint8).copy()).cuda()

    def call(d_items, n_items, max_out_len, n_bytes=64, out_floats=16):
        return L.mkws_pcm_decode(ctypes.c_void_p(d.data_ptr()), n_bytes, ctypes.c_void_p(d_items), n_items, max_out_len,
                                 ctypes.c_void_p(out.data_ptr()), out_floats, ctypes.c_void_p(flag.data_ptr()), _lib.current_stream_ptr())
    assert call(None, 0, 16) == 0 and call(items.data_ptr(), 1, 0) == 0
    torch.cuda.synchronize()
    assert flag.item() == 77 and bool((out == 3.5).all())             # not even the counter was touched
    assert call(items.data_ptr(), -1, 16) == -1 and call(items.data_ptr(), 1, -1) == -1 and call(items.data_ptr(), 1, 16, n_bytes=-1) == -1
    assert call(None, 1, 16) == -1 and b"NULL" in L.mkws_last_error()
    assert call(items.data_ptr() + 4, 1, 16) == -1 and b"aligned" in L.mkws_last_error()
    # an item with out_len 0 is legal and writes nothing; the wrapper returns an empty result for an empty table
    assert call(items.data_ptr(), 1, 16) == 0
    torch.cuda.synchronize()
    assert flag.item() == 0 and bool((out == 3.5).all())
    assert pcm.decode_on_device(d, pcm.make_items([])).numel() == 0


def test_capturable():
    """The launch inside a captured graph: replayed on new bytes it decodes them."""
    import torch
    rng = np.random.default_rng(8)
    first, second = _samples("s24", 300, 2, rng), _samples("s24", 300, 2, rng)
    d = torch.from_numpy(np.frombuffer(first, np.uint8).copy()).cuda()
    items = pcm.make_items([(0, 300, 0, 320, "s24", 2, "mix")])
    d_items = torch.from_numpy(items.view(np.uint8).copy()).cuda()
    out = torch.empty(320, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def call():
        _lib.check(L.mkws_pcm_decode(ctypes.c_void_p(d.data_ptr()), d.numel(), ctypes.c_void_p(d_items.data_ptr()), 1, 320,
                                     ctypes.c_void_p(out.data_ptr()), 320, ctypes.c_void_p(flag.data_ptr()), _lib.current_stream_ptr()))
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for data in (first, second):
        d.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), _want_row("s24", 2, data, 300, 320, "mix")) and flag.item() == 0
