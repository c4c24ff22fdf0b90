"""Shared by the PCM tests: a WAV writer for every format and header style, and the numpy restatement of the arithmetic that
include/mkws.h states ("WAV sample data decoded on the device").  Nothing here calls the library."""
import struct

import numpy as np

FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64", "mulaw", "alaw")
SAMPLE_BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8, "mulaw": 1, "alaw": 1}
FMT_CODE = {"u8": 1, "s16": 1, "s24": 1, "s32": 1, "f32": 3, "f64": 3, "alaw": 6, "mulaw": 7}
GUID_TAIL = bytes.fromhex("000000001000800000AA00389B71")


def mulaw_table():
    """int [256]: the linear value of every mu-law code, by the header's rule."""
    out = np.zeros(256, np.int64)
    for b in range(256):
        u = ~b & 0xFF
        t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)
        out[b] = 0x84 - t if u & 0x80 else t - 0x84
    return out


def alaw_table():
    out = np.zeros(256, np.int64)
    for b in range(256):
        a = b ^ 0x55
        t, seg = (a & 0x0F) << 4, (a & 0x70) >> 4
        if seg == 0:
            t += 8
        elif seg == 1:
            t += 0x108
        else:
            t = (t + 0x108) << (seg - 1)
        out[b] = t if a & 0x80 else -t
    return out


def sample_values(fmt, raw):
    """raw: uint8 [..., sample bytes] little-endian -> float32 [...] by the header's rule for `fmt`."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    lead = raw.shape[:-1]
    if fmt == "u8":
        return ((raw[..., 0].astype(np.int32) - 128).astype(np.float32) / np.float32(128.0)).reshape(lead)
    if fmt == "s16":
        return (raw.view("<i2").reshape(lead).astype(np.float32) / np.float32(32768.0))
    if fmt == "s24":
        v = raw[..., 0].astype(np.int32) | (raw[..., 1].astype(np.int32) << 8) | (raw[..., 2].astype(np.int8).astype(np.int32) << 16)
        return v.astype(np.float32) / np.float32(8388608.0)
    if fmt == "s32":
        return raw.view("<i4").reshape(lead).astype(np.float32) * np.float32(2.0 ** -31)      # int32 -> float32 rounds to nearest even
    if fmt == "f32":
        return raw.view("<f4").reshape(lead).copy()
    if fmt == "f64":
        with np.errstate(over="ignore"):
            return raw.view("<f8").reshape(lead).astype(np.float32)                           # round to nearest even
    table = mulaw_table() if fmt == "mulaw" else alaw_table()
    return (table[raw[..., 0]].astype(np.float32) / np.float32(32768.0)).reshape(lead)


def decode_frames(fmt, channels, data, channel):
    """The restatement: the bytes of whole frames -> float32 [frames] of channel `channel` (an int, or -1 / "mix").  The mix is a
    sequential float32 sum from +0.0 in channel order and one division by float32(channels)."""
    sb = SAMPLE_BYTES[fmt]
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    frames = raw.size // (sb * channels)
    v = sample_values(fmt, raw[:frames * sb * channels].reshape(frames, channels, sb))
    if channel in (-1, "mix"):
        acc = np.zeros(frames, np.float32)
        for c in range(channels):
            acc = (acc + v[:, c]).astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            return (acc / np.float32(channels)).astype(np.float32)
    return np.ascontiguousarray(v[:, channel])


def encode(fmt, x):
    """x: int array (the integer formats and the G.711 codes) or float array (f32, f64), any shape -> its little-endian bytes."""
    x = np.asarray(x)
    if fmt in ("u8", "mulaw", "alaw"):
        return x.astype(np.uint8).tobytes()
    if fmt == "s16":
        return x.astype("<i2").tobytes()
    if fmt == "s24":
        b = x.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :3]
        return np.ascontiguousarray(b).tobytes()
    if fmt == "s32":
        return x.astype("<i4").tobytes()
    return x.astype("<f4" if fmt == "f32" else "<f8").tobytes()


def from_int16(fmt, pcm16):
    """An int16 signal carried in `fmt` at full scale (G.711: the low byte pattern of the sample, any code is a legal one)."""
    p = np.asarray(pcm16).astype(np.int64)
    if fmt == "u8":
        return encode(fmt, (p >> 8) + 128)
    if fmt == "s16":
        return encode(fmt, p)
    if fmt == "s24":
        return encode(fmt, p * 256 + (p & 0xFF))
    if fmt == "s32":
        return encode(fmt, p * 65536 + (p & 0xFFFF))
    if fmt in ("f32", "f64"):
        return encode(fmt, p.astype(np.float64) / 32768.0 * 1.0000001)
    return encode(fmt, (p ^ (p >> 7)) & 0xFF)


def wav_image(fmt, channels, rate, data, extensible=False, junk=None, data_size=None, valid_bits=None, code=None, bits=None,
              block_align=None, guid_tail=GUID_TAIL, tail=b""):
    """A RIFF/WAVE file image around the sample bytes `data`.  extensible: the WAVE_FORMAT_EXTENSIBLE header; junk: the body of a chunk put
    in front of `data` (an odd length is word-padded); data_size: the size field of the data chunk when it should lie; code / bits /
    block_align / guid_tail: overrides that make the header illegal; tail: bytes after the data chunk."""
    sb = SAMPLE_BYTES[fmt]
    code = FMT_CODE[fmt] if code is None else code
    bits = 8 * sb if bits is None else bits
    block_align = sb * channels if block_align is None else block_align
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else code, channels, rate, rate * block_align, block_align, bits)
    if extensible:
        body += struct.pack("<HHI", 22, bits if valid_bits is None else valid_bits, (1 << channels) - 1 if channels < 32 else 0)
        body += struct.pack("<H", code) + guid_tail
    elif code != 1:
        body += struct.pack("<H", 0)
    chunks = b"fmt " + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")
    if junk is not None:
        chunks += b"LIST" + struct.pack("<I", len(junk)) + junk + (b"\0" if len(junk) & 1 else b"")
    data = bytes(data)
    chunks += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data + (b"\0" if len(data) & 1 else b"") + tail
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks
