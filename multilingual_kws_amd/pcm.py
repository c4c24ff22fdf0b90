"""WAV sample data decoded on the device: thin host side of mkws_pcm_* (include/mkws.h).

wav_info parses a RIFF/WAVE header on the host (no GPU needed) and says where the sample bytes are and what they hold; decode_on_device
turns a table of work items over one device byte buffer into float32 audio in one launch.  The formats, the rule for each and the mix
of channels are stated in include/mkws.h; embedding/input_data.read_clips and read_recording are the readers built on this."""
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
