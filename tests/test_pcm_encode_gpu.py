"""mkws_pcm_encode against the numpy restatement of include/mkws.h's rule (tests/util_pcm_encode.py), byte for byte, in an output buffer
pre-filled with a canary byte that must survive everywhere outside the items' own ranges: every format, frame counts on both sides of
a tile, byte offsets and buffer bases off the 16-byte grid, abutting items, windows that leave the recording, fades, edge values, the
audioop tables, offsets above 2^32, the kernel's own refusal of bad items, and capture in a graph."""
import ctypes
import os

import numpy as np
import pytest

from multilingual_kws_amd import _lib, pcm
from tests import util_pcm_encode as ue

pytestmark = pytest.mark.gpu
CANARY = 0xA5
TILE = 1024                                              # frames of one workgroup (mkws_pcm_encode.hip)
FRAMES = [0, 1, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
SKEWS = [0, 1, 7, 12]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_encode.npz")


def _launch(src, rows, out_bytes, max_frames=None, skew=0):
    """-> (the whole output with CANARY wherever nothing was written, the kernel's count of refused items).  The host check is off:
    the kernel's own is what runs.  skew: the output buffer starts that many bytes past a 16-byte boundary."""
    import torch
    d_src = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)).cuda()
    out = torch.full((skew + out_bytes,), CANARY, dtype=torch.uint8, device="cuda")[skew:]
    assert out.data_ptr() % 16 == skew
    got, bad = pcm.encode_on_device(d_src, pcm.make_encode_items(rows), out=out, max_frames=max_frames, validate=False, check=False)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy(), int(bad.cpu()[0])


class _Table:
    """Items laid out over one byte buffer: at a chosen offset modulo 16 with at least three canary bytes in front, or abutting."""

    def __init__(self, src):
        self.src, self.rows, self.at = np.ascontiguousarray(src, dtype=np.float32), [], 0

    def add(self, fmt, n_frames, start=0, fade_in=0, fade_out=0, gain=1.0, skew=None, src_offset=0, src_len=None):
        if skew is not None:
            self.at += 3
            while self.at % 16 != skew:
                self.at += 1
        src_len = self.src.size - src_offset if src_len is None else src_len
        self.rows.append((src_offset, src_len, start, n_frames, self.at, fade_in, fade_out, gain, fmt))
        self.at += n_frames * ue.SAMPLE_BYTES[fmt]

    def check(self, skew=0):
        total = self.at + 3
        got, bad = _launch(self.src, self.rows, total, skew=skew)
        want = ue.apply(self.src, self.rows, np.full(total, CANARY, np.uint8))
        assert bad == 0
        if not np.array_equal(got, want):
            k = int(np.nonzero(got != want)[0][0])
            item = max([i for i, r in enumerate(self.rows) if r[4] <= k], default=-1)
            raise AssertionError(f"byte {k} differs (item {item}: {self.rows[item] if item >= 0 else None}): got {got[k]:#x}, want {want[k]:#x}")


def _audio(n, seed):
    return np.random.default_rng(seed).uniform(-1.2, 1.2, n).astype(np.float32)


@pytest.mark.parametrize("fmt", ue.FORMATS)
def test_shapes(fmt):
    """Every frame count at every byte offset off the grid, the fades, the gain and the window rotating through their values; three
    canary bytes at least either side of every item (an s24 item's neighbours included)."""
    t, idx = _Table(_audio(3000, ue.FORMATS.index(fmt))), 0
    for nf in FRAMES:
        for skew in SKEWS:
            fade_in, fade_out = [(0, 0), (3, 0), (0, 4), (nf // 2, nf // 3)][idx % 4]
            t.add(fmt, nf, start=[0, 17, -9, 2990 - nf][(idx // 4) % 4], fade_in=fade_in, fade_out=fade_out, gain=[1.0, 0.5, -1.3][idx % 3], skew=skew)
            idx += 1
    t.check()


@pytest.mark.parametrize("skew", [0, 1, 7, 12])
def test_mixed_table_whose_ranges_abut(skew):
    """One launch over all eight formats, each item starting on the byte after the one before; the buffer itself starts off the grid."""
    t = _Table(_audio(4000, 100 + skew))
    plan = [("s24", 5), ("u8", 1023), ("s16", 1025), ("mulaw", 1), ("f64", 257), ("s24", 2049), ("alaw", 1024), ("s32", 1023), ("f32", 700),
            ("u8", 0), ("s24", 1), ("s16", 1), ("f32", 1025), ("mulaw", 2049), ("s24", 1024), ("f64", 1025)]
    t.at = 5
    for k, (fmt, nf) in enumerate(plan):
        t.add(fmt, nf, start=31 * k - 40, fade_in=k % 3 * 50, fade_out=k % 2 * 77, gain=[1.0, 0.8][k % 2])
    t.check(skew=skew)


def test_windows_that_leave_the_recording():
    """A 100-sample recording: windows in front of it, behind it, across either end and across both; `start` at its limits."""
    t = _Table(_audio(100, 1))
    for fmt in ("s16", "u8", "f32"):
        for start, nf in ((-30, 20), (-30, 30), (-30, 31), (-20, 150), (95, 20), (100, 7), (250, 9), (99, 1), (1 << 61, 1030), (-(1 << 61), 5)):
            t.add(fmt, nf, start=start, skew=(start + nf) % 16)
    t.check()
    got, _ = _launch(t.src, [(0, 100, -20, 150, 0, 0, 0, 1.0, "f32")], 600)
    v = got.view("<f4")
    assert not v[:20].any() and np.array_equal(v[20:120], t.src) and not v[120:].any()


def test_neighbouring_recordings_do_not_leak():
    """Two recordings side by side in one flat source: a window past the end of the first reads zeros, not the second."""
    src = np.concatenate([np.full(50, 0.25, np.float32), np.full(70, -0.5, np.float32)])
    t = _Table(src)
    t.add("f32", 80, start=-10, src_offset=0, src_len=50, skew=4)
    t.add("f32", 90, start=-10, src_offset=50, src_len=70, skew=8)
    t.add("s16", 60, start=45, src_offset=0, src_len=50, skew=1)
    t.add("s16", 10, start=0, src_offset=120, src_len=0, skew=3)
    t.check()
    got, _ = _launch(src, t.rows[:2], t.rows[1][4] + 360)
    first, second = got[t.rows[0][4]:][:320].view("<f4"), got[t.rows[1][4]:][:360].view("<f4")
    assert first.tolist() == [0.0] * 10 + [0.25] * 50 + [0.0] * 20 and second.tolist() == [0.0] * 10 + [-0.5] * 70 + [0.0] * 10


def test_fades():
    """A fade longer than a tile, fades that overlap, fades longer than the item, and a fade over a window that leaves the recording."""
    t = _Table(_audio(2100, 2))
    for fmt in ("f32", "s16", "s24"):
        t.add(fmt, 2049, fade_in=1500, skew=1)
        t.add(fmt, 2049, fade_out=1500, skew=7)
        t.add(fmt, 2049, fade_in=1500, fade_out=1500, skew=12)
        t.add(fmt, 100, fade_in=80, fade_out=70, skew=0)
        t.add(fmt, 10, fade_in=25, fade_out=1000, gain=2.0, skew=5)
        t.add(fmt, 1, fade_in=1, fade_out=1, skew=9)
        t.add(fmt, 1100, start=-30, fade_in=60, fade_out=60, skew=2)
        t.add(fmt, 300, start=1900, fade_in=1 << 40, fade_out=(1 << 62) + 1, skew=3)
    t.check()
    ones = np.ones(8, np.float32)
    got, _ = _launch(ones, [(0, 8, 0, 8, 0, 4, 2, 1.0, "f32")], 32)
    assert got.view("<f4").tolist() == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0, 0.5, 0.0]


EDGE = np.asarray([0.0, -0.0, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)),
                   np.nextafter(np.float32(-1), np.float32(0)), np.nextafter(np.float32(-1), np.float32(-2)), np.inf, -np.inf, np.nan,
                   1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, 1e30, -1e30, 3e38, -3e38,
                   0.5 / 128, 1.5 / 128, 2.5 / 128, -0.5 / 128, -1.5 / 128, 126.5 / 128, 127.5 / 128, 127.0 / 128, -127.5 / 128, -128.5 / 128,
                   0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, -2.5 / 32768, 32766.5 / 32768, 32767.5 / 32768,
                   32767.0 / 32768, -32767.5 / 32768, -32768.5 / 32768,
                   0.5 / 8388608, 1.5 / 8388608, 2.5 / 8388608, -1.5 / 8388608, 8388606.5 / 8388608, 8388607.0 / 8388608, -8388607.5 / 8388608,
                   0.5 * 2.0 ** -31, 1.5 * 2.0 ** -31, 2.5 * 2.0 ** -31, -1.5 * 2.0 ** -31, 1.0 - 2.0 ** -24, -1.0 + 2.0 ** -24, 2.0, -2.0],
                  dtype=np.float32)


@pytest.mark.parametrize("fmt", ue.FORMATS)
def test_edge_values(fmt):
    """+-0, +-1, the neighbours of each rail, infinities, NaN, denormals, and the half-way points of every integer grid; with gain 1 and
    no fade the float formats carry a finite value bit for bit."""
    sb, n = ue.SAMPLE_BYTES[fmt], EDGE.size
    got, bad = _launch(EDGE, [(0, n, 0, n, 3, 0, 0, 1.0, fmt)], 3 + n * sb + 3)
    want = ue.encode(fmt, EDGE)
    assert bad == 0 and (got[:3] == CANARY).all() and (got[-3:] == CANARY).all()
    assert ue.same_bytes(fmt, got[3:-3], want), [(float(EDGE[i]), got[3 + i * sb:3 + (i + 1) * sb].tolist(), want[i * sb:(i + 1) * sb].tolist())
                                                  for i in range(n) if not np.array_equal(got[3 + i * sb:3 + (i + 1) * sb], want[i * sb:(i + 1) * sb])]
    nan = int(np.nonzero(np.isnan(EDGE))[0][0])
    if fmt == "f32":
        finite = np.isfinite(EDGE)
        assert np.array_equal(got[3:-3].view("<u4")[finite], EDGE.view(np.uint32)[finite])
    elif fmt != "f64":
        assert got[3 + nan * sb:3 + (nan + 1) * sb].tolist() == [ue.ZERO_CODE.get(fmt, 0)] * sb
    # a NaN gain makes every v a NaN: the code of zero everywhere in the integer formats
    if fmt not in ("f32", "f64"):
        got, bad = _launch(np.asarray([0.5, -0.5, 0.0], np.float32), [(0, 3, 0, 3, 0, 0, 0, float("nan"), fmt)], 3 * sb)
        assert bad == 0 and got.tolist() == [ue.ZERO_CODE.get(fmt, 0)] * (3 * sb)


@pytest.mark.parametrize("fmt", ["mulaw", "alaw"])
def test_every_16_bit_sample_against_the_audioop_tables(fmt):
    golden = np.load(GOLDEN)[fmt]
    grid = np.arange(-32768, 32768).astype(np.float32) / np.float32(32768.0)
    got, bad = _launch(grid, [(0, 65536, 0, 65536, 1, 0, 0, 1.0, fmt)], 65536 + 2)
    assert bad == 0 and got[0] == CANARY and got[-1] == CANARY and np.array_equal(got[1:-1], golden)


def test_offsets_above_2_to_32():
    """A byte offset above 2^32 and a source offset above 2^31 floats: an index cut to 32 bits would land in the low regions, which
    must keep their canary."""
    import torch
    out_bytes, src_floats = (1 << 32) + 4096, (1 << 31) + 4096
    audio = _audio(1500, 10)
    src = torch.zeros(src_floats, dtype=torch.float32, device="cuda")
    at_src = (1 << 31) + 2001
    src[at_src:at_src + 1500] = torch.from_numpy(audio).cuda()
    src[2001:2001 + 1500] = 0.75                                          # what a source index cut to 31 bits would read
    out = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device="cuda")
    at = (1 << 32) + 1001                                                 # odd; the s16 item ends with the buffer's last byte
    rows = [(at_src, 1500, -7, 1025, at, 30, 30, 1.0, "s24"), (at_src, 1500, 100, 8, out_bytes - 16, 0, 0, 1.0, "s16")]
    pcm.encode_on_device(src, pcm.make_encode_items(rows), out=out)
    local = [(0, 1500, -7, 1025, 1001, 30, 30, 1.0, "s24"), (0, 1500, 100, 8, 4096 - 16, 0, 0, 1.0, "s16")]
    want = ue.apply(audio, local, np.full(4096, CANARY, np.uint8))
    assert np.array_equal(out[1 << 32:].cpu().numpy(), want)
    assert bool((out[:8192] == CANARY).all()) and bool((out[(1 << 32) - 4096:1 << 32] == CANARY).all())
    del src, out
    torch.cuda.empty_cache()


def test_invalid_items_write_nothing_and_are_counted():
    src = _audio(1000, 7)
    out_bytes, cap = 4000, 640
    good_a, good_b = (0, 1000, 5, 600, 1, 10, 10, 1.0, "s16"), (100, 900, -3, 500, 1300, 0, 20, 0.5, "s24")
    bad = [
        (0, 1000, 0, 10, 3000, 0, 0, 1.0, 8),                  # a bad format
        (0, 1000, 0, 10, 3000, 0, 0, 1.0, -1),
        (0, 1000, 0, -1, 3000, 0, 0, 1.0, "s16"),              # negative counts
        (0, 1000, 0, 10, 3000, -1, 0, 1.0, "s16"),
        (0, 1000, 0, 10, 3000, 0, -1, 1.0, "s16"),
        (0, -1, 0, 10, 3000, 0, 0, 1.0, "s16"),
        (0, 1000, 0, cap + 1, 2900, 0, 0, 1.0, "u8"),          # n_frames > max_frames
        (0, 1000, (1 << 61) + 1, 10, 3000, 0, 0, 1.0, "s16"),  # start beyond its limits
        (0, 1000, -(1 << 61) - 1, 10, 3000, 0, 0, 1.0, "s16"),
        (0, 1000, -(1 << 63), 10, 3000, 0, 0, 1.0, "s16"),
        (-1, 10, 0, 10, 3000, 0, 0, 1.0, "s16"),               # a source span outside the source
        (1001, 0, 0, 10, 3000, 0, 0, 1.0, "s16"),
        (1, 1000, 0, 10, 3000, 0, 0, 1.0, "s16"),
        (1 << 62, 1 << 62, 0, 10, 3000, 0, 0, 1.0, "s16"),
        (0, (1 << 63) - 1, 0, 10, 3000, 0, 0, 1.0, "s16"),
        (0, 1000, 0, 10, -1, 0, 0, 1.0, "s16"),                # a byte range outside the output
        (0, 1000, 0, 10, out_bytes + 1, 0, 0, 1.0, "s16"),
        (0, 1000, 0, 10, out_bytes - 19, 0, 0, 1.0, "s16"),    # its last sample ends one byte past the output
        (0, 1000, 0, 10, out_bytes - 29, 0, 0, 1.0, "s24"),
        (0, 1000, 0, 10, 1 << 62, 0, 0, 1.0, "f64"),
        (0, 1000, 0, 1, out_bytes, 0, 0, 1.0, "u8"),
    ]
    want = ue.apply(src, [good_a, good_b], np.full(out_bytes, CANARY, np.uint8))
    for k, row in enumerate(bad):                              # one at a time between valid neighbours
        got, n_bad = _launch(src, [good_a, row, good_b], out_bytes, max_frames=cap)
        assert n_bad == 1 and np.array_equal(got, want), (k, row)
    rows = [good_a] + bad[:9] + [good_b] + bad[9:]             # and all of them in one table
    got, n_bad = _launch(src, rows, out_bytes, max_frames=cap)
    assert n_bad == len(bad) and np.array_equal(got, want)
    # items at the very limits are taken
    edge = [(1000, 0, 0, 4, out_bytes - 4, 0, 0, 1.0, "u8"), (0, 1000, 1 << 61, cap, 0, 0, 0, 1.0, "s16"), (0, 1000, 0, 0, out_bytes, 5, 5, 1.0, "f64")]
    got, n_bad = _launch(src, edge, out_bytes, max_frames=cap)
    assert n_bad == 0 and np.array_equal(got, ue.apply(src, edge, np.full(out_bytes, CANARY, np.uint8)))
    # the wrapper raises on the count, and its host check names the item before anything is launched
    import torch
    d = torch.from_numpy(src).cuda()
    with pytest.raises(ValueError, match="refused 1 of 3 items"):
        pcm.encode_on_device(d, pcm.make_encode_items([good_a, bad[17], good_b]), out_bytes=out_bytes, max_frames=cap, validate=False)
    with pytest.raises(ValueError, match="pcm encode item 1"):
        pcm.encode_on_device(d, pcm.make_encode_items([good_a, bad[17], good_b]), out_bytes=out_bytes, max_frames=cap)
    # by default the output reaches as far as the items do; the host form writes the same bytes
    dev = pcm.encode_on_device(d, pcm.make_encode_items([good_a, good_b])).cpu().numpy()
    host = pcm.encode_items_host(src, pcm.make_encode_items([good_a, good_b]))
    assert dev.size == host.size == 2800
    for got in (dev, host):
        assert np.array_equal(got[1:1201], want[1:1201]) and np.array_equal(got[1300:], want[1300:2800])


def test_nothing_to_do_launches_nothing():
    import torch
    L = _lib.lib()
    src = torch.full((64,), 0.5, dtype=torch.float32, device="cuda")
    out = torch.full((64,), CANARY, dtype=torch.uint8, device="cuda")
    flag = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    items = torch.from_numpy(pcm.make_encode_items([(0, 64, 0, 0, 0, 0, 0, 1.0, "s16")]).view(np.uint8).copy()).cuda()

    def call(d_items, n_items, max_frames, src_floats=64, out_bytes=64):
        return L.mkws_pcm_encode(ctypes.c_void_p(src.data_ptr()), src_floats, ctypes.c_void_p(d_items), n_items, max_frames,
                                 ctypes.c_void_p(out.data_ptr()), out_bytes, ctypes.c_void_p(flag.data_ptr()), _lib.current_stream_ptr())
    assert call(None, 0, 16) == 0 and call(items.data_ptr(), 1, 0) == 0
    torch.cuda.synchronize()
    assert flag.item() == 77 and bool((out == CANARY).all())          # not even the counter was touched
    assert call(items.data_ptr(), -1, 16) == -1 and call(items.data_ptr(), 1, -1) == -1
    assert call(items.data_ptr(), 1, 16, src_floats=-1) == -1 and call(items.data_ptr(), 1, 16, out_bytes=-1) == -1
    assert call(None, 1, 16) == -1 and b"NULL" in L.mkws_last_error()
    assert call(items.data_ptr() + 4, 1, 16) == -1 and b"aligned" in L.mkws_last_error()
    assert call(items.data_ptr(), 1 << 21, 1 << 40) == -2 and b"exceed one launch" in L.mkws_last_error()      # MKWS_ERR_UNSUPPORTED
    # an item of no frames is legal and writes nothing; the wrapper returns an empty result for an empty table
    assert call(items.data_ptr(), 1, 16) == 0
    torch.cuda.synchronize()
    assert flag.item() == 0 and bool((out == CANARY).all())
    assert pcm.encode_on_device(src, pcm.make_encode_items([])).numel() == 0


def test_capturable():
    """The launch inside a captured graph (one stream, no branches): replayed on new audio it encodes it."""
    import torch
    first, second = _audio(300, 8), _audio(300, 9)
    d = torch.from_numpy(first).cuda()
    rows = [(0, 300, -10, 320, 1, 40, 40, 0.9, "s24")]
    d_items = torch.from_numpy(pcm.make_encode_items(rows).view(np.uint8).copy()).cuda()
    out = torch.full((962,), CANARY, dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def call():
        _lib.check(L.mkws_pcm_encode(ctypes.c_void_p(d.data_ptr()), 300, ctypes.c_void_p(d_items.data_ptr()), 1, 320,
                                     ctypes.c_void_p(out.data_ptr()), 962, ctypes.c_void_p(flag.data_ptr()), _lib.current_stream_ptr()))
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for audio in (first, second):
        d.copy_(torch.from_numpy(audio))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ue.apply(audio, rows, np.full(962, CANARY, np.uint8))) and flag.item() == 0
