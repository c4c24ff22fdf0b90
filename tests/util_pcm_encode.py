"""Shared by the encode tests: the numpy restatement of include/mkws.h's "Device audio encoded into WAV sample data", written from the
header's text and independent of multilingual_kws_amd/pcm.py (which has its own, encode_host).  The G.711 compressors are spelled the
classic way, a search through the table of segment ends, one sample at a time, and kept as two 65 536-entry tables.  Nothing here
calls the library."""
import functools

import numpy as np

FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64", "mulaw", "alaw")
SAMPLE_BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8, "mulaw": 1, "alaw": 1}
ZERO_CODE = {"u8": 128, "mulaw": 0xFF, "alaw": 0xD5}
ULAW_ENDS = (0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF)
ALAW_ENDS = (0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF)


def _search(value, ends):
    for k, end in enumerate(ends):
        if value <= end:
            return k
    return len(ends)


def _ulaw_one(q):
    m, mask = q >> 2, 0xFF
    if m < 0:
        m, mask = -m, 0x7F
    m = min(m, 8159) + 33
    seg = _search(m, ULAW_ENDS)
    return (0x7F if seg >= 8 else (seg << 4) | ((m >> (seg + 1)) & 15)) ^ mask


def _alaw_one(q):
    m, mask = q >> 3, 0xD5
    if m < 0:
        m, mask = -m - 1, 0x55
    seg = _search(m, ALAW_ENDS)
    if seg >= 8:
        return 0x7F ^ mask
    return ((seg << 4) | ((m >> 1 if seg < 2 else m >> seg) & 15)) ^ mask


@functools.lru_cache(maxsize=None)
def g711_table(fmt):
    """uint8 [65536]: entry q + 32768 is the code of the 16-bit sample q."""
    one = _ulaw_one if fmt == "mulaw" else _alaw_one
    return np.asarray([one(q) for q in range(-32768, 32768)], dtype=np.uint8)


def _round_clamp(v, scale, lo, hi):
    """rint(v * scale), the product in float32, half-way cases to even, clamped to [lo, hi]; NaN -> 0.  int64."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = (v.astype(np.float32) * np.float32(scale)).astype(np.float64)            # a float32 value, held exactly
    out = np.zeros(t.shape, np.int64)
    fin = np.isfinite(t)
    out[fin] = np.clip(np.round(t[fin]), lo, hi).astype(np.int64)                    # np.round: half to even
    out[np.isposinf(t)], out[np.isneginf(t)] = hi, lo
    return out


def encode(fmt, v):
    """float32 [n] -> uint8 [n * sample bytes] by the header's rule for `fmt`."""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    if fmt == "u8":
        return (_round_clamp(v, 128.0, -128, 127) + 128).astype(np.uint8)
    if fmt == "s16":
        return _round_clamp(v, 32768.0, -32768, 32767).astype("<i2").view(np.uint8)
    if fmt == "s24":
        q = _round_clamp(v, 8388608.0, -8388608, 8388607)
        return np.stack([q & 0xFF, (q >> 8) & 0xFF, (q >> 16) & 0xFF], axis=1).astype(np.uint8).reshape(-1)
    if fmt == "s32":
        # t >= 2^31 -> 2^31 - 1, t <= -2^31 -> -2^31, else rint(t): a clamp of the rounded value, since |t| < 2^31 rounds inside
        return _round_clamp(v, 2147483648.0, -2 ** 31, 2 ** 31 - 1).astype("<i4").view(np.uint8)
    if fmt == "f32":
        return v.astype("<f4").view(np.uint8)
    if fmt == "f64":
        return v.astype("<f8").view(np.uint8)
    return g711_table(fmt)[_round_clamp(v, 32768.0, -32768, 32767) + 32768]


def values(src, row):
    """The float32 v of every frame of one item.  row: (src_offset, src_len, start, n_frames, byte_offset, fade_in, fade_out, gain,
    format), the order of pcm.make_encode_items."""
    so, sl, start, n, _, fade_in, fade_out, gain, _ = row
    rec = np.asarray(src, dtype=np.float32).reshape(-1)[so:so + sl]
    x = np.zeros(n, np.float32)
    lo, hi = max(0, -start), min(n, sl - start)          # frames [lo, hi) lie inside the recording
    if hi > lo:
        x[lo:hi] = rec[start + lo:start + hi]
    f = np.ones(n, np.float32)
    for i in range(min(fade_in, n)):
        f[i] = np.float32(i) / np.float32(fade_in)
    for i in range(max(n - fade_out, 0), n):
        f[i] = f[i] * (np.float32(n - 1 - i) / np.float32(fade_out))
    with np.errstate(over="ignore", invalid="ignore"):
        return ((x * np.float32(gain)).astype(np.float32) * f).astype(np.float32)


def item_bytes(src, row):
    fmt = row[8] if isinstance(row[8], str) else FORMATS[row[8]]
    return encode(fmt, values(src, row))


def apply(src, rows, canvas):
    """canvas: uint8 array -> the same array with every item's bytes written at its byte_offset."""
    for row in rows:
        code = item_bytes(src, row)
        canvas[row[4]:row[4] + code.size] = code
    return canvas


def same_bytes(fmt, got, want):
    """Byte equality, except that where `want` holds a NaN of a float format `got` need only hold a NaN too (the header pins no NaN
    payload)."""
    got, want = np.asarray(got, np.uint8), np.asarray(want, np.uint8)
    if got.shape != want.shape:
        return False
    if fmt in ("f32", "f64"):
        kind = "<f4" if fmt == "f32" else "<f8"
        g, w = got.view(kind), want.view(kind)
        nan = np.isnan(w)
        return bool(np.isnan(g[nan]).all()) and np.array_equal(got.reshape(-1, SAMPLE_BYTES[fmt])[~nan], want.reshape(-1, SAMPLE_BYTES[fmt])[~nan])
    return np.array_equal(got, want)
