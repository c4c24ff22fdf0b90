"""Shared by the stream-assembly tests: the restatement of include/mkws.h's "Test streams assembled on the device", written from the
header's text one position at a time in plain Python on numpy float32 scalars, independent of multilingual_kws_amd/compose.py (which
has its own, mix_host); a float64 power reference; and the list of cases both the host and the device form are held to.  Nothing
here calls the library."""
import functools
import math
import warnings

import numpy as np

F = np.float32
LIMIT = 1 << 61
CANARY = F(-7.25)

ITEM = np.dtype([("src_offset", "<i8"), ("src_len", "<i8"), ("start", "<i8"), ("n_frames", "<i8"), ("out_start", "<i8"), ("fade_in", "<i8"),
                 ("fade_out", "<i8"), ("gain", "<f4"), ("stream", "<i4")])
DESC = np.dtype([("out_offset", "<i8"), ("n_out", "<i8"), ("bed_offset", "<i8"), ("bed_len", "<i8"), ("bed_start", "<i8"), ("max_frames", "<i8"),
                 ("first_item", "<i4"), ("n_items", "<i4")])


def item(src_offset, src_len, start, n_frames, out_start, fade_in=0, fade_out=0, gain=1.0, stream=0):
    return dict(src_offset=src_offset, src_len=src_len, start=start, n_frames=n_frames, out_start=out_start, fade_in=fade_in,
                fade_out=fade_out, gain=gain, stream=stream)


def pack(rows, dtype):
    a = np.zeros(len(rows), dtype)
    for i, row in enumerate(rows):
        for name in dtype.names:
            a[name][i] = row[name]
    return a


def item_ok(it, k, descs, src_floats):
    r = it["stream"]
    if not 0 <= r < len(descs):
        return False
    d = descs[r]
    if not d["first_item"] <= k < d["first_item"] + d["n_items"]:
        return False
    if it["n_frames"] < 0 or it["n_frames"] > d["max_frames"] or it["fade_in"] < 0 or it["fade_out"] < 0 or it["src_len"] < 0:
        return False
    if abs(it["start"]) > LIMIT or abs(it["out_start"]) > LIMIT:
        return False
    return 0 <= it["src_offset"] and it["src_offset"] + it["src_len"] <= src_floats


def stream_ok(d, n_items, src_floats, out_floats, max_out):
    """out_floats None: the power launch's check, which only wants out_offset >= 0."""
    if not 0 <= d["n_out"] <= max_out or d["out_offset"] < 0:
        return False
    if out_floats is not None and d["out_offset"] + d["n_out"] > out_floats:
        return False
    if d["first_item"] < 0 or d["n_items"] < 0 or d["first_item"] + d["n_items"] > n_items:
        return False
    if d["bed_len"] < 0:
        return False
    if d["bed_len"] > 0 and (d["bed_offset"] < 0 or d["bed_offset"] + d["bed_len"] > src_floats or not 0 <= d["bed_start"] < d["bed_len"]):
        return False
    return True


def value(src, it, i):
    """v of frame i of an item: the window with its zero padding, the gain, the two fades, every operation one float32 operation."""
    p = it["start"] + i
    x = src[it["src_offset"] + p] if 0 <= p < it["src_len"] else F(0)
    f_in = F(i) / F(it["fade_in"]) if i < it["fade_in"] else F(1)
    f_out = F(it["n_frames"] - 1 - i) / F(it["fade_out"]) if i >= it["n_frames"] - it["fade_out"] else F(1)
    return (x * F(it["gain"])) * (f_in * f_out)


def foreground(src, items, descs, r, cache=None):
    """s at every position of the valid stream r: float32 [n_out].  cache: a dict shared by launches over the SAME source, keyed by
    everything the foreground depends on, so that streams with the same items are walked once."""
    d = descs[r]
    mine = [(k, items[k]) for k in range(d["first_item"], d["first_item"] + d["n_items"])]
    mine = [it for k, it in mine if it["stream"] == r and item_ok(it, k, descs, len(src))]
    key = (d["n_out"], tuple(tuple(v for f, v in sorted(it.items()) if f != "stream") for it in mine))
    if cache is not None and key in cache:
        return cache[key].copy()
    s = np.zeros(d["n_out"], F)
    for t in range(d["n_out"]):
        first = True
        for it in mine:
            i = t - it["out_start"]
            if 0 <= i < it["n_frames"]:
                v = value(src, it, i)
                s[t] = v if first else s[t] + v
                first = False
    if cache is not None:
        cache[key] = s.copy()
    return s


def bed(src, d):
    return np.asarray([src[d["bed_offset"] + (d["bed_start"] + t) % d["bed_len"]] for t in range(d["n_out"])], F)


def mix(src, items, descs, bed_gain, clip, out, max_out, cache=None):
    """The launch on host copies: writes the valid streams into `out` (a float32 array, in place) -> the count *d_invalid ends with.
    The bed and the clip are elementwise float32 operations, one multiply, one add and two comparisons per position."""
    invalid = sum(not item_ok(it, k, descs, len(src)) for k, it in enumerate(items))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for r, d in enumerate(descs):
            if not stream_ok(d, len(items), len(src), len(out), max_out):
                invalid += 1
                continue
            y = foreground(src, items, descs, r, cache)
            if bed_gain is not None and d["bed_len"] > 0:
                y = y + bed(src, d) * F(bed_gain[r])
            if clip:
                y = np.where(y > F(1), F(1), np.where(y < F(-1), F(-1), y))
            out[d["out_offset"]:d["out_offset"] + d["n_out"]] = y
    return invalid


def powers(src, items, descs, max_out, cache=None):
    """(P_fg, P_bed) per stream in float64, each an exactly rounded sum (math.fsum) of exact squares; zeros for an invalid stream."""
    p_fg, p_bed = np.zeros(len(descs)), np.zeros(len(descs))
    for r, d in enumerate(descs):
        if not stream_ok(d, len(items), len(src), None, max_out):
            continue
        s = foreground(src, items, descs, r, cache).astype(np.float64)
        p_fg[r] = math.fsum(s * s)
        if d["bed_len"] > 0:
            b = bed(src, d).astype(np.float64)
            p_bed[r] = math.fsum(b * b)
    return p_fg, p_bed


def gain_for(p_fg, p_bed, has_bed, snr_db):
    """The bed gain in float64 (not rounded to float32): sqrt(P_fg / P_bed) * 10^(-snr_db / 20), or 0."""
    if not has_bed or not p_fg > 0 or not p_bed > 0:
        return 0.0
    return math.sqrt(p_fg / p_bed) * 10.0 ** (-snr_db / 20.0)


# ---------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------
class Case:
    """One launch: src float32, the packed tables (and their rows as dicts), bed_gain or None, clip, the output's size and max_out."""

    def __init__(self, name, src, items, descs, bed_gain=None, clip=True, out_floats=None, max_out=None, cache=None):
        self.cache = {} if cache is None else cache         # foregrounds, shared only among cases over the same source
        self.name, self.src, self.item_rows, self.desc_rows = name, np.asarray(src, F), items, descs
        self.items, self.descs = pack(items, ITEM), pack(descs, DESC)
        self.bed_gain = None if bed_gain is None else np.asarray(bed_gain, F)
        self.clip = clip
        reach = max([d["out_offset"] + d["n_out"] for d in descs if d["out_offset"] >= 0 and d["n_out"] >= 0], default=0)
        self.out_floats = reach + 5 if out_floats is None else out_floats
        self.max_out = max([d["n_out"] for d in descs], default=0) if max_out is None else max_out

    def powers(self):
        return powers(self.src, self.item_rows, self.desc_rows, self.max_out, self.cache)

    @functools.cached_property
    def expected(self):
        """(the output over a canary-filled buffer, the invalid count): computed once, never changed."""
        out = np.full(self.out_floats, CANARY, F)
        bad = mix(self.src, self.item_rows, self.desc_rows, self.bed_gain, self.clip, out, self.max_out, self.cache)
        out.setflags(write=False)
        return out, bad


def layout(streams, n_out_gap=None):
    """streams: [dict(n_out, items=[item rows without `stream`], off=floats past a 16-byte boundary or None to abut, bed=(offset, len,
    start) or None)] -> (item rows, desc rows): items sorted by out_start inside each stream, first_item / n_items / max_frames filled."""
    items, descs, at = [], [], 0
    for r, s in enumerate(streams):
        mine = sorted(s.get("items", []), key=lambda it: it["out_start"])
        off = s.get("off")
        if off is not None:
            at = ((at + 3) & ~3) + off
        bo, bl, bs = s.get("bed") or (0, 0, 0)
        descs.append(dict(out_offset=at, n_out=s["n_out"], bed_offset=bo, bed_len=bl, bed_start=bs,
                          max_frames=s.get("max_frames", max([it["n_frames"] for it in mine], default=0)), first_item=len(items), n_items=len(mine)))
        items += [dict(it, stream=r) for it in mine]
        at += max(s["n_out"], 0)
    return items, descs


def _noise(n, seed):
    return np.random.default_rng(seed).uniform(-0.9, 0.9, n).astype(F)


def case_single_items():
    """Lone items of 0 .. 2049 frames at five places of streams that start 0, 1 and 3 floats past a 16-byte boundary."""
    src = _noise(2100, 1)
    streams, idx = [], 0
    for n in (0, 1, 1023, 1024, 1025, 2049):
        n_out = max(n, 1024) + 9
        for at in (-5, 0, 1, 1019, n_out - 3):
            for off in (0, 1, 3):
                streams.append(dict(n_out=n_out, off=off, items=[item(0, 2100, idx % 5, n, at)]))
                idx += 1
    return Case("single_items", src, *layout(streams))


def case_lengths():
    """Streams of 0, 1 and 4099 positions and one more, abutting in the output; the long one has two items and a bed."""
    src = _noise(6000, 2)
    streams = [dict(n_out=0, items=[item(0, 100, 0, 50, 0)]), dict(n_out=1, items=[item(7, 100, 0, 50, 0)]),
               dict(n_out=4099, items=[item(0, 3000, 0, 3000, 2), item(3000, 2000, 0, 2000, 2500, 100, 100, 0.5)], bed=(5000, 1000, 3)),
               dict(n_out=30, items=[item(100, 30, 0, 30, 0)])]
    return Case("lengths", src, *layout(streams), bed_gain=[0.0, 0.0, 0.25, 0.0])


def case_windows():
    """Windows that leave their recording on the left, on the right and on both sides; the neighbours in the flat source are loud."""
    src = np.concatenate([np.full(50, 0.9, F), _noise(40, 3) * F(0.5), np.full(50, -0.9, F)])
    streams = [dict(n_out=70, off=1, items=[item(50, 40, -10, 30, 3)]), dict(n_out=70, off=2, items=[item(50, 40, 20, 50, 3)]),
               dict(n_out=70, off=3, items=[item(50, 40, -5, 50, 3)]), dict(n_out=1100, off=0, items=[item(50, 40, -500, 1100, 0)])]
    return Case("windows", src, *layout(streams))


def case_add_order():
    """Three items on one position whose float32 sum depends on the order (1e8 + 1 - 1e8), and three long ones overlapping."""
    src = np.concatenate([np.asarray([1e8, 1.0, -1e8], F), _noise(3000, 4)])
    streams = [dict(n_out=12, off=1, items=[item(0, 1, 0, 1, 5), item(1, 1, 0, 1, 5), item(2, 1, 0, 1, 5)]),
               dict(n_out=12, off=1, items=[item(1, 1, 0, 1, 5), item(0, 1, 0, 1, 5), item(2, 1, 0, 1, 5)]),
               dict(n_out=2600, off=3, items=[item(3, 3000, 0, 1500, 10, 0, 0, 0.7), item(3, 3000, 1000, 1400, 900, 0, 0, 0.6),
                                              item(3, 3000, 77, 1300, 1000, 50, 50, -0.9)])]
    return Case("add_order", src, *layout(streams), clip=False)


def case_fades():
    """Fades longer than a tile, fades that overlap inside one item, and fades longer than the item."""
    src = _noise(3100, 5)
    streams = [dict(n_out=3010, off=0, items=[item(0, 3100, 0, 3000, 4, 1300, 1200)]),
               dict(n_out=3010, off=1, items=[item(0, 3100, 5, 3000, 0, 2000, 2000)]),
               dict(n_out=300, off=2, items=[item(0, 3100, 5, 200, 10, 500, 700)]),
               dict(n_out=2100, off=0, items=[item(0, 3100, 0, 2100, 0, 16, 0)])]
    return Case("fades", src, *layout(streams))


def case_outside():
    """An item wholly before its stream, one wholly after it, and one that only touches its ends."""
    src = _noise(300, 6)
    streams = [dict(n_out=100, off=0, items=[item(0, 300, 0, 50, -100)]), dict(n_out=100, off=1, items=[item(0, 300, 0, 50, 105)]),
               dict(n_out=100, off=2, items=[item(0, 300, 0, 50, -49), item(0, 300, 0, 50, 99), item(0, 300, 0, 50, -50), item(0, 300, 0, 50, 100)]),
               dict(n_out=1100, off=3, items=[item(0, 300, 0, 300, -1 << 40), item(0, 300, 0, 300, 1 << 40)])]
    return Case("outside", src, *layout(streams))


def case_special_values():
    """-0.0f, a quiet NaN, the infinities and denormals through a lone item at gain 1: unchanged.  No clip (it would take the infinities)."""
    vals = np.asarray([-0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, 1.1754942e-38, 0.0, 3.4028235e38], F)
    src = np.concatenate([vals, _noise(1100, 7), vals])
    streams = [dict(n_out=len(vals), off=1, items=[item(0, len(vals), 0, len(vals), 0)]),
               dict(n_out=len(src), off=0, items=[item(0, len(src), 0, len(src), 0)]),                # the aligned body and its tail
               dict(n_out=len(src) + 2, off=3, items=[item(0, len(src), 0, len(src), 1)])]
    return Case("special_values", src, *layout(streams), clip=False)


def _bed_streams():
    src = np.concatenate([_noise(2400, 8), _noise(1, 9), _noise(7, 10), _noise(1000, 11), _noise(5000, 12)])
    streams, at = [], 2400
    for n in (1, 7, 1000, 5000):
        for start in (0, n - 1):
            streams.append(dict(n_out=2300, off=len(streams) % 4, items=[item(0, 2400, 3, 2200, 50, 0, 0, 0.5)], bed=(at, n, start)))
        at += n
    streams.append(dict(n_out=1500, off=2, items=[], bed=(2408, 1000, 999)))                           # bed only
    streams.append(dict(n_out=1500, off=1, items=[item(0, 2400, 0, 1500, 0)], bed=None))                # no bed, with a gain given
    return src, streams


def case_beds():
    """Beds of 1, 7, 1000 and 5000 samples from their first and their last sample on, a stream of bed alone and one without."""
    src, streams = _bed_streams()
    return Case("beds", src, *layout(streams), bed_gain=[0.1 * (r + 1) for r in range(len(streams))])


def case_beds_unused():
    """The same tables with d_bed_gain == NULL: no stream gets its bed."""
    src, streams = _bed_streams()
    return Case("beds_unused", src, *layout(streams), bed_gain=None)


def _clip_case(name, clip):
    one = F(1)
    vals = np.asarray([1.0, -1.0, np.nextafter(one, F(2)), np.nextafter(one, F(0)), np.nextafter(-one, F(-2)), np.nextafter(-one, F(0)), np.nan,
                       2.0, -2.0, 0.5, np.inf, -np.inf], F)
    src = np.concatenate([vals, np.asarray([0.75], F)])
    streams = [dict(n_out=len(vals), off=1, items=[item(0, len(vals), 0, len(vals), 0)]),
               dict(n_out=len(vals), off=2, items=[item(0, len(vals), 0, len(vals), 0, 0, 0, 0.5)], bed=(len(vals), 1, 0))]   # 0.5 x + 0.75
    return Case(name, src, *layout(streams), bed_gain=[0.0, 1.0], clip=clip)


def case_clip_on():
    """Exactly +-1.0f, their float neighbours, NaN and values beyond, clipped."""
    return _clip_case("clip_on", True)


def case_clip_off():
    """The same values with the flag off."""
    return _clip_case("clip_off", False)


# every way a table entry can be refused: (what, field, value); "other" re-points an item at a stream whose range it is not in
BAD_ITEMS = [("stream", -1), ("stream", "past"), ("stream", "other"), ("n_frames", -1), ("n_frames", "above"), ("fade_in", -1), ("fade_out", -2),
             ("src_len", -1), ("start", LIMIT + 1), ("start", -LIMIT - 1), ("out_start", LIMIT + 1), ("out_start", -LIMIT - 1),
             ("src_offset", -1), ("src_offset", "past"), ("src_len", "past")]
BAD_STREAMS = [("n_out", -1), ("n_out", "above"), ("out_offset", -3), ("out_offset", "past"), ("first_item", -1), ("n_items", -1),
               ("n_items", "past"), ("bed_len", -1), ("bed_offset", -1), ("bed_len", "past"), ("bed_start", -1), ("bed_start", "len")]
INVALID_SRC, INVALID_N_OUT = 400, 40


def invalid_base():
    """One stream per entry of BAD_ITEMS and BAD_STREAMS between two untouched ones: three items each (the middle one is the one to
    spoil, kept where the ascending order wants it), a bed of 10 samples each."""
    n = len(BAD_ITEMS) + len(BAD_STREAMS) + 2
    streams = [dict(n_out=INVALID_N_OUT, off=r % 4, bed=(300 + r, 10, r % 10),
                    items=[item(0, 100, 0, 10, 2, 0, 0, 0.5), item(100, 100, 0, 10, 8), item(200, 100, 5, 10, 14, 3, 3)]) for r in range(n)]
    return layout(streams)


def spoil(items, descs, what, index, field, value):
    """One defect: what is "item" (index: the stream whose middle item is spoilt) or "stream" -> the index of the spoilt table entry."""
    n_streams, n_items = len(descs), len(items)
    if what == "item":
        k = descs[index]["first_item"] + 1
        it = items[k]
        value = {("stream", "past"): n_streams, ("stream", "other"): 0, ("n_frames", "above"): descs[index]["max_frames"] + 1,
                 ("src_offset", "past"): INVALID_SRC + 1, ("src_len", "past"): INVALID_SRC - it["src_offset"] + 1}.get((field, value), value)
        if field == "out_start" and value > 0:
            k += 1                                          # the last item of the stream, so that the order still ascends
        elif field == "out_start":
            k -= 1
        items[k][field] = value
        return k
    d = descs[index]
    value = {("n_out", "above"): INVALID_N_OUT + 1, ("out_offset", "past"): 1 << 40, ("n_items", "past"): n_items - d["first_item"] + 1,
             ("bed_len", "past"): INVALID_SRC - d["bed_offset"] + 1, ("bed_start", "len"): d["bed_len"]}.get((field, value), value)
    d[field] = value
    return index


def case_invalid():
    """Every kind of invalid item and stream in one launch, each in a stream of its own between valid neighbours."""
    items, descs = invalid_base()
    for m, (field, value) in enumerate(BAD_ITEMS):
        spoil(items, descs, "item", m + 1, field, value)
    for m, (field, value) in enumerate(BAD_STREAMS):
        spoil(items, descs, "stream", len(BAD_ITEMS) + m + 1, field, value)
    reach = max(d["out_offset"] for d in descs if d["out_offset"] < 1 << 39) + INVALID_N_OUT + 8
    return Case("invalid", _noise(INVALID_SRC, 13), items, descs, bed_gain=[0.5] * len(descs), out_floats=reach, max_out=INVALID_N_OUT)


CASES = [case_single_items, case_lengths, case_windows, case_add_order, case_fades, case_outside, case_special_values, case_beds,
         case_beds_unused, case_clip_on, case_clip_off]


@functools.lru_cache(maxsize=None)
def get(maker):
    return maker()
