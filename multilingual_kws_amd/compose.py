"""Test streams assembled on the device: thin host side of mkws_stream_* (include/mkws.h).

make_stream_items / make_stream_descs build the numpy mirrors of the two tables, check_stream_tables is the kernel's own check of them
(plus the ordering the kernel takes for granted), mix_on_device / power_on_device / bed_gain_on_device are the three launches, and
mix_host / power_host / bed_gain_host are the same rule in numpy: the specification in code, and what
embedding/generate_stream_sentences.compose_streams falls back to for audio that is not on a device."""
import ctypes
import math

import numpy as np

from . import _lib, pcm

CLIP = 1                                                                       # MKWS_STREAM_CLIP
TILE = 1024                                                                    # positions of one workgroup: sizes the partials
START_LIMIT = pcm.START_LIMIT                                                  # |start| and |out_start| of an item

# mkws_stream_item
ITEM_DTYPE = np.dtype([("src_offset", "<i8"), ("src_len", "<i8"), ("start", "<i8"), ("n_frames", "<i8"), ("out_start", "<i8"),
                       ("fade_in", "<i8"), ("fade_out", "<i8"), ("gain", "<f4"), ("stream", "<i4")])
assert ITEM_DTYPE.itemsize == ctypes.sizeof(_lib.StreamItem) == 64

# mkws_stream_desc
DESC_DTYPE = np.dtype([("out_offset", "<i8"), ("n_out", "<i8"), ("bed_offset", "<i8"), ("bed_len", "<i8"), ("bed_start", "<i8"),
                       ("max_frames", "<i8"), ("first_item", "<i4"), ("n_items", "<i4")])
assert DESC_DTYPE.itemsize == ctypes.sizeof(_lib.StreamDesc) == 56


def make_stream_items(rows, return_order=False):
    """[(src_offset, src_len, start, n_frames, out_start, fade_in, fade_out, gain, stream)] -> the numpy mirror of the item table, sorted
    (stably) by stream and out_start as the kernel wants it; with return_order also the row every table entry came from."""
    items = np.zeros(len(rows), dtype=ITEM_DTYPE)
    if len(rows):
        for name, col in zip(ITEM_DTYPE.names, zip(*rows)):
            items[name] = col
    order = np.lexsort((items["out_start"], items["stream"]))                  # stable; the last key is the primary one
    items = items[order]
    return (items, order) if return_order else items


def make_stream_descs(rows, items):
    """[(out_offset, n_out, bed_offset, bed_len, bed_start)], one row per stream, and the SORTED item table -> the numpy mirror of the
    descriptor table: first_item, n_items and max_frames are filled in from the items that name the stream."""
    descs = np.zeros(len(rows), dtype=DESC_DTYPE)
    if len(rows):
        for name, col in zip(DESC_DTYPE.names[:5], zip(*rows)):
            descs[name] = col
    stream = np.asarray(items["stream"], np.int64)
    first = np.searchsorted(stream, np.arange(len(rows)), side="left")
    last = np.searchsorted(stream, np.arange(len(rows)), side="right")
    descs["first_item"], descs["n_items"] = first, last - first
    for r in range(len(rows)):
        descs["max_frames"][r] = max(0, int(items["n_frames"][first[r]:last[r]].max())) if last[r] > first[r] else 0
    return descs


def item_problem(it, k, descs, src_floats):
    """Why the kernel refuses item k (None: it does not), in words."""
    so, sl, st, nf, os_, fi, fo = (int(it[f]) for f in ("src_offset", "src_len", "start", "n_frames", "out_start", "fade_in", "fade_out"))
    r = int(it["stream"])
    if not 0 <= r < len(descs):
        return f"stream {r} (0 .. {len(descs) - 1})"
    first, n, mf = int(descs[r]["first_item"]), int(descs[r]["n_items"]), int(descs[r]["max_frames"])
    if not first <= k < first + n:
        return f"it lies outside the items [{first}, {first + n}) of its stream {r}"
    if nf < 0 or fi < 0 or fo < 0 or sl < 0:
        return f"n_frames = {nf}, fade_in = {fi}, fade_out = {fo}, src_len = {sl}"
    if nf > mf:
        return f"n_frames = {nf} above max_frames = {mf} of its stream {r}"
    if not -START_LIMIT <= st <= START_LIMIT:
        return f"start = {st} beyond +-2^61"
    if not -START_LIMIT <= os_ <= START_LIMIT:
        return f"out_start = {os_} beyond +-2^61"
    if not 0 <= so <= src_floats or sl > src_floats - so:
        return f"source [{so}, {so + sl}) passes the source's {src_floats} floats"
    return None


def stream_problem(d, n_items, src_floats, out_floats, max_out):
    """Why the kernel refuses a stream descriptor (None: it does not), in words.  out_floats None: the power launch, which writes nothing
    at out_offset and checks only its sign."""
    oo, no, bo, bl, bs = (int(d[f]) for f in ("out_offset", "n_out", "bed_offset", "bed_len", "bed_start"))
    first, n = int(d["first_item"]), int(d["n_items"])
    if not 0 <= no <= max_out:
        return f"n_out = {no} (0 .. max_out = {max_out})"
    if oo < 0 or (out_floats is not None and (oo > out_floats or no > out_floats - oo)):
        return f"outputs [{oo}, {oo + no}) pass the output's {out_floats} floats"
    if first < 0 or n < 0 or first + n > n_items:
        return f"items [{first}, {first + n}) pass the table's {n_items} items"
    if bl < 0:
        return f"bed_len = {bl}"
    if bl > 0 and (not 0 <= bo <= src_floats or bl > src_floats - bo):
        return f"bed [{bo}, {bo + bl}) passes the source's {src_floats} floats"
    if bl > 0 and not 0 <= bs < bl:
        return f"bed_start = {bs} (0 .. bed_len - 1 = {bl - 1})"
    return None


def _items_ok(items, descs, src_floats):
    """item_problem(...) is None for every item at once: a boolean array."""
    k, r = np.arange(len(items), dtype=np.int64), items["stream"].astype(np.int64)
    ok = (r >= 0) & (r < len(descs))
    if not len(descs):
        return ok
    rc = np.clip(r, 0, len(descs) - 1)
    first, n, mf = descs["first_item"].astype(np.int64)[rc], descs["n_items"].astype(np.int64)[rc], descs["max_frames"][rc]
    so, sl, st, nf, at = items["src_offset"], items["src_len"], items["start"], items["n_frames"], items["out_start"]
    ok &= (k >= first) & (k - first < n) & (nf >= 0) & (nf <= mf) & (items["fade_in"] >= 0) & (items["fade_out"] >= 0) & (sl >= 0)
    ok &= (st >= -START_LIMIT) & (st <= START_LIMIT) & (at >= -START_LIMIT) & (at <= START_LIMIT)
    ok &= (so >= 0) & (so <= src_floats) & (sl <= src_floats - np.clip(so, 0, src_floats))
    return ok


def check_stream_tables(items, descs, src_floats, out_floats, max_out):
    """The kernel's own check of every item and stream, on the host mirrors, and the ascending out_start inside a stream that the kernel
    takes for granted: ValueError naming the first item or stream that fails and why."""
    for k in np.nonzero(~_items_ok(items, descs, src_floats))[0][:1]:       # the first refused item, in words
        raise ValueError(f"stream item {k}: {item_problem(items[k], int(k), descs, src_floats)}")
    for r, d in enumerate(descs):
        why = stream_problem(d, len(items), src_floats, out_floats, max_out)
        if why is not None:
            raise ValueError(f"stream {r}: {why}")
        first, n = int(d["first_item"]), int(d["n_items"])
        down = np.nonzero(np.diff(items["out_start"][first:first + n]) < 0)[0]
        if len(down):
            k = first + int(down[0]) + 1
            raise ValueError(f"stream {r}: item {k} has out_start = {int(items['out_start'][k])} below item {k - 1}'s "
                             f"{int(items['out_start'][k - 1])} (ascending out_start is required)")


def _tables(items, descs):
    return (np.ascontiguousarray(items, dtype=ITEM_DTYPE).reshape(-1), np.ascontiguousarray(descs, dtype=DESC_DTYPE).reshape(-1))


def _max_out(descs, max_out):
    return (int(descs["n_out"].max()) if len(descs) else 0) if max_out is None else int(max_out)


def _reach(descs):
    return int((descs["out_offset"] + descs["n_out"]).max()) if len(descs) else 0


def n_tiles(max_out):
    return (int(max_out) + TILE - 1) // TILE


# ---------------------------------------------------------------------------------------------------
# the specification in numpy
# ---------------------------------------------------------------------------------------------------
def foreground_host(src, items, d, r):
    """The foreground s of stream r (descriptor d) over its n_out positions, float32: the first covering item in table order sets a
    position, every further one adds to it with one float32 add."""
    n_out = int(d["n_out"])
    s, covered = np.zeros(n_out, np.float32), np.zeros(n_out, bool)
    first = int(d["first_item"])
    for k in range(first, first + int(d["n_items"])):
        it = items[k]
        if int(it["stream"]) != r:
            continue
        at, n = int(it["out_start"]), int(it["n_frames"])
        lo, hi = max(0, -at), min(n, n_out - at)
        if hi <= lo:
            continue
        v = pcm.item_values_host(src, it)[lo:hi]
        seg, cov = s[at + lo:at + hi], covered[at + lo:at + hi]
        with np.errstate(over="ignore", invalid="ignore"):
            seg[...] = np.where(cov, seg + v, v)
        cov[...] = True
    return s


def _bed_host(src, d):
    idx = (int(d["bed_start"]) + np.arange(int(d["n_out"]), dtype=np.int64)) % int(d["bed_len"])
    return src[int(d["bed_offset"]):int(d["bed_offset"]) + int(d["bed_len"])][idx]


def mix_host(src, items, descs, bed_gain=None, clip=True, out=None, out_floats=None):
    """What mix_on_device computes, on the host (include/mkws.h, "Test streams assembled on the device"): numpy float32 src, the two
    tables, bed_gain float32 [streams] or None (no stream gets its bed) -> float32 array (`out`, or a fresh zeroed one of out_floats
    floats, or of what the streams reach).  The tables are checked as check_stream_tables checks them; a refused one raises."""
    items, descs = _tables(items, descs)
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
    if out is None:
        out = np.zeros(_reach(descs) if out_floats is None else int(out_floats), np.float32)
    check_stream_tables(items, descs, src.size, out.size, _max_out(descs, None))
    gains = None if bed_gain is None else np.asarray(bed_gain, dtype=np.float32).reshape(-1)
    for r, d in enumerate(descs):
        y = foreground_host(src, items, d, r)
        if gains is not None and int(d["bed_len"]) > 0:
            with np.errstate(over="ignore", invalid="ignore"):
                y = y + _bed_host(src, d) * gains[r]
        if clip:
            with np.errstate(invalid="ignore"):
                y = np.where(y > np.float32(1), np.float32(1), np.where(y < np.float32(-1), np.float32(-1), y))
        out[int(d["out_offset"]):int(d["out_offset"]) + int(d["n_out"])] = y
    return out


def power_host(src, items, descs):
    """(P_fg, P_bed), float64 [streams] each: the exactly rounded sums (math.fsum) of the squares of the foreground and of the raw bed over
    every stream's n_out positions; P_bed is 0 for a stream without a bed."""
    items, descs = _tables(items, descs)
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
    check_stream_tables(items, descs, src.size, None, _max_out(descs, None))
    p_fg, p_bed = np.zeros(len(descs)), np.zeros(len(descs))
    for r, d in enumerate(descs):
        s = foreground_host(src, items, d, r).astype(np.float64)
        p_fg[r] = math.fsum(s * s)
        if int(d["bed_len"]) > 0:
            b = _bed_host(src, d).astype(np.float64)
            p_bed[r] = math.fsum(b * b)
    return p_fg, p_bed


def snr_scale(snr_db):
    """10^(-snr_db / 20) as float64: what the host hands to mkws_stream_bed_gain."""
    return np.asarray([10.0 ** (-float(v) / 20.0) for v in np.asarray(snr_db, dtype=np.float64).reshape(-1)], dtype=np.float64)


def bed_gain_host(p_fg, p_bed, descs, scale):
    """mkws_stream_bed_gain's rule: float32 (sqrt(P_fg / P_bed) * scale) per stream, 0 where either power is not above zero or the
    stream has no bed."""
    g = np.zeros(len(descs), np.float32)
    for r, d in enumerate(descs):
        if int(d["bed_len"]) > 0 and p_fg[r] > 0.0 and p_bed[r] > 0.0:
            g[r] = np.float32(math.sqrt(p_fg[r] / p_bed[r]) * float(scale[r]))
    return g


# ---------------------------------------------------------------------------------------------------
# the launches
# ---------------------------------------------------------------------------------------------------
def upload_tables(items, descs, device):
    """Both tables in one non-blocking copy -> (the tensor that owns the memory, device pointer of the items or None, of the streams)."""
    import torch
    items, descs = _tables(items, descs)
    raw = np.concatenate([items.view(np.uint8).reshape(-1), descs.view(np.uint8).reshape(-1), np.zeros(8, np.uint8)])
    d_raw = torch.from_numpy(raw).to(device, non_blocking=True)
    return d_raw, (d_raw.data_ptr() if len(items) else None), d_raw.data_ptr() + items.nbytes


def _src_tensor(src):
    import torch
    if not torch.is_tensor(src) or src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("src must be a contiguous float32 tensor")
    return src


def _raise_refused(name, invalid, items, descs):
    bad = int(invalid.cpu()[0])
    if bad:
        raise ValueError(f"{name} refused {bad} of {len(items)} items and {len(descs)} streams")


def mix_on_device(src, items, descs, bed_gain=None, clip=True, out=None, out_floats=None, max_out=None, validate=True, check=True,
                  tables=None):
    """mkws_stream_mix.  src: a contiguous CUDA float32 tensor the tables index as a flat array; items, descs: the numpy mirrors
    (make_stream_items, make_stream_descs); bed_gain: a float32 CUDA tensor [streams] (bed_gain_on_device's, or any) or None; out: a
    contiguous CUDA float32 tensor (default: a fresh one of out_floats floats, or of what the streams reach) -> out.  Only the streams'
    own ranges are written.  validate: the host mirrors are checked first, before anything touches the device (ValueError naming the
    item or stream).  check: after the launch the kernel's count of refused items and streams is read (one synchronising copy) and a
    non-zero count raises; with check=False -> (out, the count as an int32 CUDA tensor [1]), asynchronous on the current stream.
    tables: upload_tables' result, to share one upload among the three launches."""
    import torch
    items, descs = _tables(items, descs)
    src = _src_tensor(src)
    max_out = _max_out(descs, max_out)
    if out is not None:
        out_floats = int(out.numel())
    elif out_floats is None:
        out_floats = _reach(descs)
    if validate:
        check_stream_tables(items, descs, int(src.numel()), int(out_floats), max_out)
    if not src.is_cuda:
        raise ValueError("src must be on the device (the host form is mix_host)")
    device = src.device
    if out is None:
        out = torch.empty(int(out_floats), dtype=torch.float32, device=device)
    elif not out.is_cuda or out.device != device or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous CUDA float32 tensor on the source's device")
    if bed_gain is not None and (not torch.is_tensor(bed_gain) or bed_gain.device != device or bed_gain.dtype != torch.float32
                                 or not bed_gain.is_contiguous() or bed_gain.numel() != len(descs)):
        raise ValueError("bed_gain must be a contiguous CUDA float32 tensor [streams] on the source's device")
    with torch.cuda.device(device):
        keep, p_items, p_descs = tables if tables is not None else upload_tables(items, descs, device)
        invalid = torch.zeros(1, dtype=torch.int32, device=device)
        _lib.check(_lib.lib().mkws_stream_mix(
            ctypes.c_void_p(src.data_ptr()), int(src.numel()), ctypes.c_void_p(p_items), len(items), ctypes.c_void_p(p_descs), len(descs),
            ctypes.c_void_p(bed_gain.data_ptr()) if bed_gain is not None else None, CLIP if clip else 0, max_out,
            ctypes.c_void_p(out.data_ptr()), int(out_floats), ctypes.c_void_p(invalid.data_ptr()), _lib.current_stream_ptr()))
    if not check:
        return out, invalid
    _raise_refused("mkws_stream_mix", invalid, items, descs)
    return out


def power_on_device(src, items, descs, partials=None, max_out=None, validate=True, check=True, tables=None):
    """mkws_stream_power -> float64 CUDA tensor [streams, tiles, 2] (`partials`, or a fresh one): per tile of 1024 positions the sum of
    the squares of the foreground and of the raw bed.  validate / check / tables: as in mix_on_device."""
    import torch
    items, descs = _tables(items, descs)
    src = _src_tensor(src)
    max_out = _max_out(descs, max_out)
    if validate:
        check_stream_tables(items, descs, int(src.numel()), None, max_out)
    if not src.is_cuda:
        raise ValueError("src must be on the device (the host form is power_host)")
    device = src.device
    shape = (len(descs), n_tiles(max_out), 2)
    if partials is None:
        partials = torch.zeros(shape, dtype=torch.float64, device=device)
    elif partials.device != device or partials.dtype != torch.float64 or not partials.is_contiguous() or tuple(partials.shape) != shape:
        raise ValueError(f"partials must be a contiguous CUDA float64 tensor {shape} on the source's device")
    with torch.cuda.device(device):
        keep, p_items, p_descs = tables if tables is not None else upload_tables(items, descs, device)
        invalid = torch.zeros(1, dtype=torch.int32, device=device)
        _lib.check(_lib.lib().mkws_stream_power(
            ctypes.c_void_p(src.data_ptr()), int(src.numel()), ctypes.c_void_p(p_items), len(items), ctypes.c_void_p(p_descs), len(descs),
            max_out, ctypes.c_void_p(partials.data_ptr()), ctypes.c_void_p(invalid.data_ptr()), _lib.current_stream_ptr()))
    if not check:
        return partials, invalid
    _raise_refused("mkws_stream_power", invalid, items, descs)
    return partials


def bed_gain_on_device(partials, descs, scale, bed_gain=None, max_out=None, tables=None):
    """mkws_stream_bed_gain.  partials: power_on_device's; scale: snr_scale(snr_db) as a float64 CUDA tensor [streams] (a host array is
    uploaded) -> float32 CUDA tensor [streams] (`bed_gain`, or a fresh one).  Asynchronous on the current stream."""
    import torch
    descs = np.ascontiguousarray(descs, dtype=DESC_DTYPE).reshape(-1)
    max_out = _max_out(descs, max_out)
    device = partials.device
    if not partials.is_cuda or partials.dtype != torch.float64 or not partials.is_contiguous() or partials.numel() != len(descs) * n_tiles(max_out) * 2:
        raise ValueError("partials must be power_on_device's contiguous CUDA float64 tensor [streams, tiles, 2]")
    if not torch.is_tensor(scale):
        scale = torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)).to(device, non_blocking=True)
    if scale.device != device or scale.dtype != torch.float64 or not scale.is_contiguous() or scale.numel() != len(descs):
        raise ValueError("scale must be a contiguous float64 tensor [streams] on the partials' device")
    if bed_gain is None:
        bed_gain = torch.zeros(len(descs), dtype=torch.float32, device=device)
    elif bed_gain.device != device or bed_gain.dtype != torch.float32 or not bed_gain.is_contiguous() or bed_gain.numel() != len(descs):
        raise ValueError("bed_gain must be a contiguous CUDA float32 tensor [streams] on the partials' device")
    with torch.cuda.device(device):
        keep, _, p_descs = tables if tables is not None else upload_tables(np.zeros(0, ITEM_DTYPE), descs, device)
        _lib.check(_lib.lib().mkws_stream_bed_gain(
            ctypes.c_void_p(partials.data_ptr()), ctypes.c_void_p(p_descs), len(descs), max_out, ctypes.c_void_p(scale.data_ptr()),
            ctypes.c_void_p(bed_gain.data_ptr()), _lib.current_stream_ptr()))
    return bed_gain
