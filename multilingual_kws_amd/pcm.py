"""WAV sample data decoded on the device: thin host side of mkws_pcm_* (include/mkws.h).

wav_info parses a RIFF/WAVE header on the host (no GPU needed) and says where the sample bytes are and what they hold; decode_on_device
turns a table of work items over one device byte buffer into float32 audio in one launch.  The formats, the rule for each and the mix
of channels are stated in include/mkws.h; embedding/input_data.read_clips and read_recording are the readers built on this.

The way out: wav_header writes a file's header, encode_on_device turns a table of encode items -- windows of
float32 recordings in device memory, with a gain and two linear fades -- into mono sample data of any of the formats in one launch
(mkws_pcm_encode), and encode_host / encode_items_host are the same rule in numpy: the specification in code, and what the writers
(input_data.encode_wav / write_clips / convert_clips, word_extraction.extract_shots, batch_streaming_analysis.extract_detections)
fall back to for audio that is not on a device."""
import ctypes
import struct
from collections import namedtuple

import numpy as np

from . import _lib

FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64", "mulaw", "alaw")          # index = MKWS_PCM_*
FORMAT_ID = {name: i for i, name in enumerate(FORMATS)}
SAMPLE_BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8, "mulaw": 1, "alaw": 1}
MIX = -1

# mkws_pcm_item
ITEM_DTYPE = np.dtype([("byte_offset", "<i8"), ("n_frames", "<i8"), ("out_offset", "<i8"), ("out_len", "<i8"),
                       ("format", "<i4"), ("channels", "<i4"), ("channel", "<i4"), ("reserved", "<i4")])
assert ITEM_DTYPE.itemsize == ctypes.sizeof(_lib.PcmItem) == 48

# mkws_pcm_encode_item
ENCODE_ITEM_DTYPE = np.dtype([("src_offset", "<i8"), ("src_len", "<i8"), ("start", "<i8"), ("n_frames", "<i8"), ("byte_offset", "<i8"),
                              ("fade_in", "<i8"), ("fade_out", "<i8"), ("gain", "<f4"), ("format", "<i4")])
assert ENCODE_ITEM_DTYPE.itemsize == ctypes.sizeof(_lib.PcmEncodeItem) == 64
START_LIMIT = 1 << 61                                                          # |start| of an encode item
FORMAT_CODE = {"u8": 1, "s16": 1, "s24": 1, "s32": 1, "f32": 3, "f64": 3, "alaw": 6, "mulaw": 7}      # wFormatTag

WavInfo = namedtuple("WavInfo", "format channels rate data_offset frames frame_bytes")

_GUID_TAIL = bytes.fromhex("000000001000800000AA00389B71")                    # KSDATAFORMAT_SUBTYPE_*: the 14 bytes after the code
_BY_CODE = {(1, 8): "u8", (1, 16): "s16", (1, 24): "s24", (1, 32): "s32", (3, 32): "f32", (3, 64): "f64", (6, 8): "alaw", (7, 8): "mulaw"}


def channel_index(channel):
    """An int stays what it is; "mix" is MIX (-1)."""
    if isinstance(channel, str):
        if channel != "mix":
            raise ValueError(f'channel must be an int or "mix", not {channel!r}')
        return MIX
    return int(channel)


def frame_bytes(fmt, channels):
    """Host-only: mkws_pcm_frame_bytes of a format (name or MKWS_PCM_* index) and a channel count; ValueError for what it refuses."""
    L = _lib.lib()
    n = L.mkws_pcm_frame_bytes(FORMAT_ID.get(fmt, -1) if isinstance(fmt, str) else int(fmt), int(channels))
    if n < 0:
        raise ValueError(L.mkws_last_error().decode("utf-8", "replace"))
    return n


def wav_info(data):
    """Host-only: the bytes of a RIFF/WAVE file -> WavInfo(format name, channels, rate, data_offset, frames, frame_bytes).  The chunk walk
    is decode_wav's (word-padded chunks, the first `data` chunk ends it).  Accepted: PCM at 8, 16, 24 or 32 bits, IEEE float at 32 or 64,
    A-law and mu-law at 8, and WAVE_FORMAT_EXTENSIBLE resolved through its sub-format GUID (the container size decides the decoding;
    wValidBitsPerSample is ignored: samples are left-justified).  A `data` size past the end of the file (a streamed WAV) is clamped to
    the file and a trailing partial frame is dropped.  ValueError for anything else."""
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    pos, fmt, body, at = 12, None, None, None
    while pos + 8 <= len(data):
        cid, size = bytes(data[pos:pos + 4]), struct.unpack("<I", data[pos + 4:pos + 8])[0]
        if cid == b"fmt ":
            body = bytes(data[pos + 8:pos + 8 + size])
            if len(body) < 16:
                raise ValueError("WAV file has a fmt chunk shorter than 16 bytes")
            fmt = struct.unpack("<HHIIHH", body[:16])
        elif cid == b"data":
            at = pos + 8
            data_bytes = min(size, len(data) - at)
            break
        pos += 8 + size + (size & 1)
    if fmt is None or at is None:
        raise ValueError("WAV file lacks a fmt or data chunk")
    code, channels, rate, _, block_align, bits = fmt
    if code == 0xFFFE:
        if len(body) < 40 or struct.unpack("<H", body[16:18])[0] < 22:
            raise ValueError("WAVE_FORMAT_EXTENSIBLE header shorter than its 22-byte extension")
        if body[26:40] != _GUID_TAIL:
            raise ValueError(f"WAVE_FORMAT_EXTENSIBLE with an unknown sub-format GUID {body[24:40].hex()}")
        code = struct.unpack("<H", body[24:26])[0]
    name = _BY_CODE.get((code, bits))
    if name is None:
        raise ValueError(f"unsupported WAV sample format (format {code}, {bits} bits)")
    if channels < 1:
        raise ValueError(f"WAV file with {channels} channels")
    fb = SAMPLE_BYTES[name] * channels
    if block_align != fb:
        raise ValueError(f"WAV block_align {block_align} is not channels * bits / 8 = {fb}")
    return WavInfo(name, channels, rate, at, data_bytes // fb, fb)


def make_items(rows):
    """[(byte_offset, n_frames, out_offset, out_len, format name or index, channels, channel)] -> the numpy mirror of the item table."""
    items = np.zeros(len(rows), dtype=ITEM_DTYPE)
    if len(rows):
        bo, nf, oo, ol, fmt, chans, ch = zip(*rows)
        items["byte_offset"], items["n_frames"], items["out_offset"], items["out_len"], items["channels"] = bo, nf, oo, ol, chans
        items["format"] = [FORMAT_ID[f] if isinstance(f, str) else int(f) for f in fmt]
        items["channel"] = [channel_index(c) for c in ch]
    return items


def check_items(items, n_bytes, out_floats, max_out_len):
    """The kernel's own check of every item, on the host mirror: ValueError naming the first item that fails and why."""
    fmt, chans = items["format"], items["channels"].astype(np.int64)
    ok = (fmt >= 0) & (fmt < len(FORMATS)) & (chans >= 1) & (items["channel"] >= -1) & (items["channel"] < chans)
    fb = np.asarray([SAMPLE_BYTES[f] for f in FORMATS], np.int64)[np.clip(fmt, 0, len(FORMATS) - 1)] * np.maximum(chans, 1)
    bo, nf, oo, ol = items["byte_offset"], items["n_frames"], items["out_offset"], items["out_len"]
    ok &= (nf >= 0) & (ol >= 0) & (ol <= max_out_len) & (bo >= 0) & (bo <= n_bytes) & (nf <= (n_bytes - np.clip(bo, 0, n_bytes)) // fb)
    ok &= (oo >= 0) & (oo <= out_floats) & (ol <= out_floats - np.clip(oo, 0, out_floats))
    for k in np.nonzero(~ok)[0][:1]:                    # the first refused item, in words
        it = items[k]
        bo, nf, oo, ol = int(it["byte_offset"]), int(it["n_frames"]), int(it["out_offset"]), int(it["out_len"])
        fmt, chans, ch = int(it["format"]), int(it["channels"]), int(it["channel"])
        why = None
        if not 0 <= fmt < len(FORMATS):
            why = f"format {fmt} (0 .. {len(FORMATS) - 1})"
        elif chans < 1:
            why = f"{chans} channels"
        elif not -1 <= ch < chans:
            why = f"channel {ch} of {chans}"
        elif nf < 0 or ol < 0:
            why = f"n_frames = {nf}, out_len = {ol}"
        elif ol > max_out_len:
            why = f"out_len = {ol} above max_out_len = {max_out_len}"
        elif not 0 <= bo <= n_bytes or nf > (n_bytes - bo) // (SAMPLE_BYTES[FORMATS[fmt]] * chans):
            why = f"{nf} frames of {SAMPLE_BYTES[FORMATS[fmt]] * chans} bytes at byte {bo} pass the buffer's {n_bytes} bytes"
        elif not 0 <= oo <= out_floats or ol > out_floats - oo:
            why = f"outputs [{oo}, {oo + ol}) pass the output's {out_floats} floats"
        if why is not None:
            raise ValueError(f"pcm item {k}: {why}")


def decode_on_device(byte_tensor, items, out=None, out_floats=None, max_out_len=None, validate=True, check=True):
    """mkws_pcm_decode.  byte_tensor: contiguous uint8 tensor, the sample bytes; items: the numpy mirror of the table (ITEM_DTYPE,
    make_items); out: a contiguous CUDA float32 tensor the items index as a flat array (default: a fresh one of out_floats floats, or of
    what the items reach) -> out.  Only the items' own ranges are written.  validate: the host mirror is checked first, before anything
    touches the device (ValueError with the item's index).  check: after the launch the kernel's count of refused items is read
    (one synchronising copy) and a non-zero count raises; with check=False -> (out, the count as an int32 CUDA tensor [1]), asynchronous
    on the current stream."""
    import torch
    items = np.ascontiguousarray(items, dtype=ITEM_DTYPE).reshape(-1)
    if not torch.is_tensor(byte_tensor) or byte_tensor.dtype != torch.uint8 or not byte_tensor.is_contiguous():
        raise ValueError("byte_tensor must be a contiguous uint8 tensor")
    n_bytes, n_items = int(byte_tensor.numel()), len(items)
    if max_out_len is None:
        max_out_len = int(items["out_len"].max()) if n_items else 0
    if out is not None:
        out_floats = int(out.numel())
    elif out_floats is None:
        out_floats = int((items["out_offset"] + items["out_len"]).max()) if n_items else 0
    if validate:
        check_items(items, n_bytes, int(out_floats), int(max_out_len))
    if not byte_tensor.is_cuda:
        raise ValueError("byte_tensor must be on the device (there is no CPU path)")
    device = byte_tensor.device
    if out is None:
        out = torch.empty(int(out_floats), dtype=torch.float32, device=device)
    elif not out.is_cuda or out.device != device or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous CUDA float32 tensor on the bytes' device")
    with torch.cuda.device(device):
        d_items = torch.from_numpy(items.view(np.uint8).reshape(-1).copy()).to(device, non_blocking=True) if n_items else None
        invalid = torch.zeros(1, dtype=torch.int32, device=device)
        _lib.check(_lib.lib().mkws_pcm_decode(
            ctypes.c_void_p(byte_tensor.data_ptr()), n_bytes, ctypes.c_void_p(d_items.data_ptr()) if n_items else None, n_items,
            int(max_out_len), ctypes.c_void_p(out.data_ptr()), int(out_floats), ctypes.c_void_p(invalid.data_ptr()), _lib.current_stream_ptr()))
    if not check:
        return out, invalid
    bad = int(invalid.cpu()[0])
    if bad:
        raise ValueError(f"mkws_pcm_decode refused {bad} of {n_items} items")
    return out


# ---------------------------------------------------------------------------------------------------
# the way out: device audio encoded into WAV sample data (mkws_pcm_encode)
# ---------------------------------------------------------------------------------------------------
def _format_name(fmt):
    if isinstance(fmt, str):
        if fmt not in FORMAT_ID:
            raise ValueError(f"unknown sample format {fmt!r} (one of {', '.join(FORMATS)})")
        return fmt
    if not 0 <= int(fmt) < len(FORMATS):
        raise ValueError(f"format {fmt} (0 .. {len(FORMATS) - 1})")
    return FORMATS[int(fmt)]


def wav_header(fmt, rate, frames, channels=1):
    """Host-only: the bytes of a RIFF/WAVE file in front of its sample data, for `frames` frames of `channels` samples of format `fmt`
    (name or MKWS_PCM_* index) at `rate`.  u8 / s16 / s24 / s32: format code 1 and a 16-byte fmt chunk (44 bytes in all); f32 / f64 /
    A-law / mu-law: codes 3 / 6 / 7, an 18-byte fmt chunk and a fact chunk holding the frame count (58 bytes).  The sizes are exact:
    the data chunk's is the sample bytes, the RIFF chunk's counts the pad byte that follows an odd data size (the writer appends it)."""
    name = _format_name(fmt)
    rate, frames, channels = int(rate), int(frames), int(channels)
    if rate < 1 or frames < 0 or channels < 1:
        raise ValueError(f"wav_header: rate = {rate}, frames = {frames}, channels = {channels}")
    block = SAMPLE_BYTES[name] * channels
    code, data = FORMAT_CODE[name], frames * block
    body = struct.pack("<HHIIHH", code, channels, rate, rate * block, block, 8 * SAMPLE_BYTES[name])
    chunks = b""
    if code != 1:
        body += struct.pack("<H", 0)
        chunks = b"fact" + struct.pack("<II", 4, frames)
    chunks = b"fmt " + struct.pack("<I", len(body)) + body + chunks + b"data"
    riff = 4 + len(chunks) + 4 + data + (data & 1)
    if riff > 0xFFFFFFFF:
        raise ValueError(f"wav_header: {data} bytes of samples do not fit a RIFF file")
    return b"RIFF" + struct.pack("<I", riff) + b"WAVE" + chunks + struct.pack("<I", data)


def make_encode_items(rows):
    """[(src_offset, src_len, start, n_frames, byte_offset, fade_in, fade_out, gain, format name or index)] -> the numpy mirror of the
    mkws_pcm_encode_item table."""
    items = np.zeros(len(rows), dtype=ENCODE_ITEM_DTYPE)
    if len(rows):
        so, sl, st, nf, bo, fi, fo, gain, fmt = zip(*rows)
        items["src_offset"], items["src_len"], items["start"], items["n_frames"], items["byte_offset"] = so, sl, st, nf, bo
        items["fade_in"], items["fade_out"], items["gain"] = fi, fo, gain
        items["format"] = [FORMAT_ID[f] if isinstance(f, str) else int(f) for f in fmt]
    return items


def _encode_sample_bytes(fmt):
    return np.asarray([SAMPLE_BYTES[f] for f in FORMATS], np.int64)[np.clip(fmt, 0, len(FORMATS) - 1)]


def check_encode_items(items, src_floats, out_bytes, max_frames):
    """The kernel's own check of every encode item, on the host mirror: ValueError naming the first item that fails and why."""
    fmt = items["format"]
    so, sl, st, nf, bo = items["src_offset"], items["src_len"], items["start"], items["n_frames"], items["byte_offset"]
    ok = (fmt >= 0) & (fmt < len(FORMATS)) & (nf >= 0) & (nf <= max_frames) & (items["fade_in"] >= 0) & (items["fade_out"] >= 0) & (sl >= 0)
    ok &= (st >= -START_LIMIT) & (st <= START_LIMIT)
    ok &= (so >= 0) & (so <= src_floats) & (sl <= src_floats - np.clip(so, 0, src_floats))
    ok &= (bo >= 0) & (bo <= out_bytes) & (nf <= (out_bytes - np.clip(bo, 0, out_bytes)) // _encode_sample_bytes(fmt))
    for k in np.nonzero(~ok)[0][:1]:                    # the first refused item, in words
        it = items[k]
        so, sl, st, nf, bo = (int(it[f]) for f in ("src_offset", "src_len", "start", "n_frames", "byte_offset"))
        fi, fo, fmt = int(it["fade_in"]), int(it["fade_out"]), int(it["format"])
        why = None
        if not 0 <= fmt < len(FORMATS):
            why = f"format {fmt} (0 .. {len(FORMATS) - 1})"
        elif nf < 0 or fi < 0 or fo < 0 or sl < 0:
            why = f"n_frames = {nf}, fade_in = {fi}, fade_out = {fo}, src_len = {sl}"
        elif nf > max_frames:
            why = f"n_frames = {nf} above max_frames = {max_frames}"
        elif not -START_LIMIT <= st <= START_LIMIT:
            why = f"start = {st} beyond +-2^61"
        elif not 0 <= so <= src_floats or sl > src_floats - so:
            why = f"source [{so}, {so + sl}) passes the source's {src_floats} floats"
        elif not 0 <= bo <= out_bytes or nf > (out_bytes - bo) // SAMPLE_BYTES[FORMATS[fmt]]:
            why = f"{nf} frames of {SAMPLE_BYTES[FORMATS[fmt]]} bytes at byte {bo} pass the output's {out_bytes} bytes"
        if why is not None:
            raise ValueError(f"pcm encode item {k}: {why}")


def _encode_reach(items):
    return int((items["byte_offset"] + items["n_frames"] * _encode_sample_bytes(items["format"])).max()) if len(items) else 0


def encode_on_device(src, items, out=None, out_bytes=None, max_frames=None, validate=True, check=True):
    """mkws_pcm_encode.  src: a contiguous CUDA float32 tensor the items index as a flat array; items: the numpy mirror of the table
    (ENCODE_ITEM_DTYPE, make_encode_items); out: a contiguous CUDA uint8 tensor (default: a fresh one of out_bytes bytes, or of what the
    items reach) -> out.  Only the items' own byte ranges are written.  validate: the host mirror is checked first, before anything
    touches the device (ValueError with the item's index).  check: after the launch the kernel's count of refused items is read (one
    synchronising copy) and a non-zero count raises; with check=False -> (out, the count as an int32 CUDA tensor [1]), asynchronous on
    the current stream."""
    import torch
    items = np.ascontiguousarray(items, dtype=ENCODE_ITEM_DTYPE).reshape(-1)
    if not torch.is_tensor(src) or src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("src must be a contiguous float32 tensor")
    src_floats, n_items = int(src.numel()), len(items)
    if max_frames is None:
        max_frames = int(items["n_frames"].max()) if n_items else 0
    if out is not None:
        out_bytes = int(out.numel())
    elif out_bytes is None:
        out_bytes = _encode_reach(items)
    if validate:
        check_encode_items(items, src_floats, int(out_bytes), int(max_frames))
    if not src.is_cuda:
        raise ValueError("src must be on the device (the host form is encode_items_host)")
    device = src.device
    if out is None:
        out = torch.empty(int(out_bytes), dtype=torch.uint8, device=device)
    elif not out.is_cuda or out.device != device or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("out must be a contiguous CUDA uint8 tensor on the source's device")
    with torch.cuda.device(device):
        d_items = torch.from_numpy(items.view(np.uint8).reshape(-1).copy()).to(device, non_blocking=True) if n_items else None
        invalid = torch.zeros(1, dtype=torch.int32, device=device)
        _lib.check(_lib.lib().mkws_pcm_encode(
            ctypes.c_void_p(src.data_ptr()), src_floats, ctypes.c_void_p(d_items.data_ptr()) if n_items else None, n_items,
            int(max_frames), ctypes.c_void_p(out.data_ptr()), int(out_bytes), ctypes.c_void_p(invalid.data_ptr()), _lib.current_stream_ptr()))
    if not check:
        return out, invalid
    bad = int(invalid.cpu()[0])
    if bad:
        raise ValueError(f"mkws_pcm_encode refused {bad} of {n_items} items")
    return out


def _quantise(v, scale, lo, hi):
    """rint(v * scale) clamped to [lo, hi] as int64; NaN -> 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(v * np.float32(scale))
    return np.clip(np.where(np.isnan(r), np.float32(0), r), lo, hi).astype(np.int64)


def _segment(m, first_end):
    """The index of the first of the 8 segment ends first_end, 2 * first_end + 1, ... that m does not exceed (8: above them all)."""
    seg = np.zeros(m.shape, np.int64)
    for k in range(8):
        seg += m > ((first_end + 1) << k) - 1
    return seg


def encode_host(fmt, v):
    """The specification of mkws_pcm_encode's sample rule in numpy (include/mkws.h): float32 values [n] -> uint8 [n * sample bytes], the
    little-endian samples of format `fmt` (name or MKWS_PCM_* index).  The writers use it when there is no GPU."""
    name = _format_name(fmt)
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    if name == "u8":
        return (_quantise(v, 128.0, -128, 127) + 128).astype(np.uint8)
    if name == "s16":
        return _quantise(v, 32768.0, -32768, 32767).astype("<i2").view(np.uint8)
    if name == "s24":
        return np.ascontiguousarray(_quantise(v, 8388608.0, -8388608, 8388607).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)
    if name == "s32":
        with np.errstate(over="ignore", invalid="ignore"):
            t = v * np.float32(2147483648.0)
            r = np.where(np.isnan(t), np.float32(0), np.rint(t)).astype(np.float64)
        q = np.where(t >= np.float32(2147483648.0), 2 ** 31 - 1, np.where(t <= np.float32(-2147483648.0), -2 ** 31, np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1)))
        return q.astype(np.int64).astype("<i4").view(np.uint8)
    if name == "f32":
        return v.astype("<f4").view(np.uint8)
    if name == "f64":
        return v.astype("<f8").view(np.uint8)
    q = _quantise(v, 32768.0, -32768, 32767)
    if name == "mulaw":
        m = q >> 2
        mask = np.where(m < 0, 0x7F, 0xFF)
        m = np.minimum(np.abs(m), 8159) + 33
        seg = _segment(m, 0x3F)
        code = np.where(seg >= 8, 0x7F, (seg << 4) | ((m >> (np.minimum(seg, 7) + 1)) & 15))
    else:
        m = q >> 3
        mask = np.where(m < 0, 0x55, 0xD5)
        m = np.where(m < 0, -m - 1, m)
        seg = _segment(m, 0x1F)
        code = np.where(seg >= 8, 0x7F, (seg << 4) | (np.where(seg < 2, m >> 1, m >> np.minimum(seg, 7)) & 15))
    return (code ^ mask).astype(np.uint8)


def item_values_host(src, item):
    """The float32 values v of one encode item's frames (include/mkws.h: the window with its zero padding, the gain, the two fades), in
    numpy with the kernel's operation order.  src: the flat float32 source."""
    so, sl, st, n = (int(item[f]) for f in ("src_offset", "src_len", "start", "n_frames"))
    fi, fo, gain = int(item["fade_in"]), int(item["fade_out"]), np.float32(item["gain"])
    i = np.arange(n, dtype=np.int64)
    pos = st + i
    inside = (pos >= 0) & (pos < sl)
    x = np.zeros(n, np.float32)
    x[inside] = np.asarray(src, dtype=np.float32).reshape(-1)[so:so + sl][pos[inside]]
    f_in, f_out = np.ones(n, np.float32), np.ones(n, np.float32)
    if fi > 0:
        f_in[i < fi] = i[i < fi].astype(np.float32) / np.float32(fi)
    if fo > 0:
        late = i >= n - fo
        f_out[late] = (n - 1 - i[late]).astype(np.float32) / np.float32(fo)
    with np.errstate(over="ignore", invalid="ignore"):
        return (x * gain) * (f_in * f_out)


def encode_items_host(src, items, out=None, out_bytes=None, max_frames=None):
    """What encode_on_device computes, on the host: numpy float32 src, the item table -> uint8 array (`out`, or a fresh one of
    out_bytes bytes, or of what the items reach).  The items are checked as the kernel checks them; a refused one raises."""
    items = np.ascontiguousarray(items, dtype=ENCODE_ITEM_DTYPE).reshape(-1)
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
    if out is None:
        out = np.zeros(_encode_reach(items) if out_bytes is None else int(out_bytes), np.uint8)
    if max_frames is None:
        max_frames = int(items["n_frames"].max()) if len(items) else 0
    check_encode_items(items, src.size, out.size, int(max_frames))
    for it in items:
        code = encode_host(int(it["format"]), item_values_host(src, it))
        out[int(it["byte_offset"]):int(it["byte_offset"]) + code.size] = code
    return out
