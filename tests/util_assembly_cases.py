"""Case tables and float64 references for the batch-assembly kernels of mkws_augment.hip (mkws_augment_batch, mkws_specaug_apply,
mkws_specaug_apply_n).  Plain numpy: no torch, no GPU, nothing of the package.  tests/test_assembly_cases_cpu.py states what every
group of cases is there for and ties the references to the product's host code; tests/test_assembly_kernels_gpu.py runs the tables.

Sources of one clip length n (augment_sources):
  bank 0   [3, n]  two dense rows, then the SPIKE row: zero except 0.75 at SPIKE_SRC(n)
  bank 1   [2, n]  two dense rows
  track 0  [2n+37] zero except -0.5 at SPIKE_BG(n) = n + 18: a slice at offset SPIKE_BG - q has its only sample at q, the slice at
                   offset 0 is all zero
  track 1  [2n+37] dense on [0, n + 37), then 1/32768 on the last n samples (the slice that ends on the last sample of the last track)
Dense values lie on the int16 grid (k / 32768, |k| >= 1), foreground up to 0.5, background up to 0.3.  The stride is odd, so track 1 --
and, for odd n, every second bank row -- starts off the 8- and 16-byte boundaries.
"""
import functools

import numpy as np

ITEM_DTYPE = np.dtype([("mode", "<i4"), ("bank", "<i4"), ("src", "<i4"), ("shift", "<i4"),
                       ("bg_idx", "<i4"), ("bg_off", "<i4"), ("bg_vol", "<f4"), ("reserved", "<i4")])     # == mkws_augment_item

AUGMENT_LENGTHS = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 9600, 16000)
VOLUMES = (0.05, 1.0, 3.0)
SPIKE_POSITIONS = (0, 255, 256, 2047, 2048)          # and n - 1: the edges of a wave's share, of the block and of the 8-wide pass
SPIKE_FG, SPIKE_BG_VALUE = 0.75, -0.5
BOUND = 2e-6                                         # mode 2, times scale[j]: the bound tests/test_pipeline_gpu.py already asserts


def bg_stride_of(n):
    return 2 * n + 37


def spike_src(n):
    """Where the spike row of bank 0 holds its sample: shifts of both signs are needed to move it over SPIKE_POSITIONS."""
    return 256 if n > 512 else (n - 1) // 2


def spike_bg(n):
    return n + 18


# ---------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------
def shifted(fg, shift):
    """out[t] = fg[t - shift], zero outside: element by element, for any shift."""
    n = fg.shape[0]
    out = np.zeros(n, dtype=fg.dtype)
    t = np.arange(n, dtype=np.int64)
    s = t - int(shift)
    ok = (s >= 0) & (s < n)
    out[t[ok]] = fg[s[ok]]
    return out


def ref_augment(bank0, bank1, bg, bg_stride, items, n):
    """The item semantics of include/mkws.h in float64 -> (out64 [B, n], scale [B]).  bank0 / bank1 [rows, n], bg flat or
    [tracks, bg_stride] (None where no item needs it).  scale[j] = max(1, max|bg_slice| * snr * bg_vol) for mode 2, else 1: what the
    mode 2 bound is multiplied with."""
    B = len(items)
    out, scale = np.zeros((B, n), dtype=np.float64), np.ones(B, dtype=np.float64)
    flat = None if bg is None else np.asarray(bg).reshape(-1)
    for j in range(B):
        it = items[j]
        mode, vol = int(it["mode"]), float(np.float32(it["bg_vol"]))
        if mode in (0, 2):
            bank = bank0 if int(it["bank"]) == 0 else bank1
            fg = shifted(np.asarray(bank[int(it["src"])], dtype=np.float64), int(it["shift"]))
        if mode in (1, 2):
            at = int(it["bg_idx"]) * int(bg_stride) + int(it["bg_off"])
            sl = flat[at:at + n].astype(np.float64)
            assert at >= 0 and sl.shape[0] == n
        if mode == 0:
            out[j] = fg
        elif mode == 1:
            out[j] = sl * vol
        else:
            fg_rms, bg_rms = np.sqrt(np.mean(fg * fg)), np.sqrt(np.mean(sl * sl))
            snr = fg_rms / bg_rms if bg_rms > 0 else 0.0
            out[j] = np.clip(fg + sl * snr * vol, -1.0, 1.0)
            scale[j] = max(1.0, float(np.abs(sl).max()) * snr * vol)
    return out, scale


def spike_bound(ref_row):
    """Element-wise bound of a spike item: one float32 ulp of the result (plus the float64 reference's own rounding, 4 eps relative;
    the exact result of these items is a short binary fraction, the reference reaches it through two square roots and a division)."""
    return np.spacing(np.abs(ref_row).astype(np.float32)).astype(np.float64) + 4 * np.finfo(np.float64).eps * np.abs(ref_row)


def ref_specaug(spec, masks, n_freq, n_time):
    """Element (f, c) of clip b is zero iff some channel mask of row b has start <= c < start + size or some frame mask has
    start <= f < start + size; every other element is the input's, bit for bit.  Index sets, no slicing."""
    spec, masks = np.asarray(spec), np.asarray(masks, dtype=np.int64).reshape(spec.shape[0], 2 * (n_freq + n_time))
    B, F, C = spec.shape
    f, c = np.arange(F, dtype=np.int64), np.arange(C, dtype=np.int64)
    out = spec.copy()
    for b in range(B):
        zc, zf = np.zeros(C, dtype=bool), np.zeros(F, dtype=bool)
        for k in range(n_freq):
            start, size = masks[b, 2 * k], masks[b, 2 * k + 1]
            zc |= (start <= c) & (c < start + size)
        for k in range(n_time):
            start, size = masks[b, 2 * (n_freq + k)], masks[b, 2 * (n_freq + k) + 1]
            zf |= (start <= f) & (f < start + size)
        out[b][zf[:, None] | zc[None, :]] = 0
    return out


# ---------------------------------------------------------------------------------------------------
# augmentation cases
# ---------------------------------------------------------------------------------------------------
def _dense(rng, shape, peak):
    k = rng.integers(1, peak + 1, size=shape) * rng.choice(np.asarray([-1, 1]), size=shape)
    return (k / 32768.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def augment_sources(n):
    """-> (bank0 [3, n], bank1 [2, n], bg [2, 2n + 37]) float32, read-only."""
    rng = np.random.default_rng(1000 + n)
    stride = bg_stride_of(n)
    bank0, bank1 = _dense(rng, (3, n), 16384), _dense(rng, (2, n), 16384)
    bank0[2] = 0
    bank0[2, spike_src(n)] = SPIKE_FG
    bg = np.zeros((2, stride), dtype=np.float32)
    bg[0, spike_bg(n)] = SPIKE_BG_VALUE
    bg[1, :n + 37] = _dense(rng, n + 37, 9830)
    bg[1, n + 37:] = 1.0 / 32768.0
    for a in (bank0, bank1, bg):
        a.setflags(write=False)
    return bank0, bank1, bg


def dense_shifts(n):
    """0, +-1, +-(n-1), +-n, +-(n+5), the block / pass edges where they fit inside the clip, two seeded random ones."""
    out = [0]
    for s in (1, n - 1, n, n + 5) + tuple(s for s in (255, 256, 2047, 2048) if s < n):
        out += [s, -s]
    rng = np.random.default_rng(2000 + n)
    out += [int(s) for s in rng.integers(-(n - 1), n, 2)]
    return list(dict.fromkeys(out))


def spike_positions(n):
    return [p for p in SPIKE_POSITIONS if p < n - 1] + [n - 1]


def _item(mode, bank=0, src=0, shift=0, bg_idx=0, bg_off=0, vol=0.0, tag=""):
    return (mode, bank, src, shift, bg_idx, bg_off, vol), tag


@functools.lru_cache(maxsize=None)
def augment_case(n):
    """-> (items [B <= 64] of ITEM_DTYPE, tags [B]): the item table of clip length n.  Tags name what an item is there for:
    'dense' | 'zero_bg' | 'fg_out' | 'tiny_bg' | 'clip+' | 'clip-' | 'spike p q' | 'spike_out q'."""
    stride = bg_stride_of(n)
    rows = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2)]                  # (bank, src): every row, the last of each bank included
    dense_rows = rows[:4]
    last_off = stride - n
    table = []
    # mode 0: every shift, the rows taken in turn (the spike row too: a copy that shows an off-by-one shift as a moved sample)
    for i, s in enumerate(dense_shifts(n)):
        bank, src = rows[i % len(rows)]
        table.append(_item(0, bank, src, s, tag="dense"))
    # mode 1: both tracks, offset 0, the dense stretch's last offset, the slice that ends the last track; every volume
    for i, (idx, off) in enumerate(((1, 0), (1, 37), (1, last_off), (0, spike_bg(n) - (n - 1)), (1, 5 % 38))):
        bank, src = rows[i % len(rows)]
        table.append(_item(1, bank, src, 3, idx, off, VOLUMES[i % 3], tag="dense"))
    # mode 2 on dense signals: every shift, both banks, offsets over the dense stretch of the last track
    for i, s in enumerate(dense_shifts(n)):
        bank, src = dense_rows[(i + 1) % 4]
        table.append(_item(2, bank, src, s, 1, (0, 37, 11, 36)[i % 4], VOLUMES[i % 3], tag="dense"))
    # mode 2 at its degenerate ends
    table.append(_item(2, 1, 1, 1 if n > 1 else 0, 0, 0, 1.0, tag="zero_bg"))             # rms(bg) == 0: the ratio is 0, not inf
    table.append(_item(2, 0, 1, n, 1, 7, 3.0, tag="fg_out"))                              # rms(shift(fg)) == 0
    table.append(_item(2, 1, 0, -n, 1, 7, 1.0, tag="fg_out"))
    table.append(_item(2, 0, 0, 0, 1, last_off, 0.05, tag="tiny_bg"))                     # ratio ~ 1e4
    # mode 2 that clips at each sign: the first dense combination whose reference output reaches it
    bank0, bank1, bg = augment_sources(n)
    for sign, tag in ((1.0, "clip+"), (-1.0, "clip-")):
        found = None
        for off in range(38):
            for bank, src in dense_rows:
                cand = np.zeros(1, dtype=ITEM_DTYPE)
                cand[0] = (2, bank, src, 0, 1, off, 3.0, 0)
                if (ref_augment(bank0, bank1, bg, stride, cand, n)[0] == sign).any():
                    found = (bank, src, off)
                    break
            if found:
                break
        assert found, (n, tag)
        table.append(_item(2, found[0], found[1], 0, 1, found[2], 3.0, tag=tag))
    # spikes: foreground sample moved to p, background sample at q; each of p and q goes over every listed position
    pos = spike_positions(n)
    # (volume 1 leaves the ratio of the two RMS values as the only rounded quantity of the output, volume 3 clips it; where both
    # samples meet, p == q, the background is quiet so that the sum does not cancel: see test_assembly_kernels_gpu.py on their bound)
    for i, p in enumerate(pos):
        q = pos[(i + 1) % len(pos)]
        table.append(_item(2, 0, 2, p - spike_src(n), 0, spike_bg(n) - q, 0.05 if p == q else (1.0, 3.0)[i % 2], tag=f"spike {p} {q}"))
    # both samples on the last position of the clip, and the foreground moved just past either end
    table.append(_item(2, 0, 2, n - 1 - spike_src(n), 0, spike_bg(n) - (n - 1), 0.05, tag=f"spike {n - 1} {n - 1}"))
    table.append(_item(2, 0, 2, n - spike_src(n), 0, spike_bg(n) - (n - 1), 1.0, tag=f"spike_out {n - 1}"))
    table.append(_item(2, 0, 2, -spike_src(n) - 1, 0, spike_bg(n), 1.0, tag="spike_out 0"))
    items = np.zeros(len(table), dtype=ITEM_DTYPE)
    for j, (fields, _) in enumerate(table):
        items[j] = fields + (0,)
    assert len(items) <= 64
    items.setflags(write=False)
    return items, tuple(tag for _, tag in table)


@functools.lru_cache(maxsize=None)
def augment_expected(n):
    """ref_augment on the table of n, computed once -> (out64, scale), read-only."""
    bank0, bank1, bg = augment_sources(n)
    out, scale = ref_augment(bank0, bank1, bg, bg_stride_of(n), augment_case(n)[0], n)
    out.setflags(write=False)
    scale.setflags(write=False)
    return out, scale


CONTRACT_CASES = ("null_bank1", "null_bg", "one_item")


def contract_case(name):
    """-> (n, bank0, bank1 or None, bg or None, bg_stride, items): launches the contract of include/mkws.h allows."""
    n = {"null_bank1": 2049, "null_bg": 257, "one_item": 2049}[name]
    bank0, bank1, bg = augment_sources(n)
    items, tags = augment_case(n)
    if name == "null_bank1":                        # every item in bank 0, all three modes
        return n, bank0, None, bg, bg_stride_of(n), items[items["bank"] == 0]
    if name == "null_bg":                           # every item mode 0, both banks; no background at all
        return n, bank0, bank1, None, 0, items[items["mode"] == 0]
    return n, bank0, bank1, bg, bg_stride_of(n), items[[tags.index("tiny_bg")]]


# ---------------------------------------------------------------------------------------------------
# SpecAugment cases
# ---------------------------------------------------------------------------------------------------
SPECAUG_SHAPES = ((49, 40), (29, 33), (1, 1), (3, 100), (7, 36), (8, 32), (64, 5))      # 7 x 36 = 252, 8 x 32 = 256 = one block's stride
SPECAUG_COUNTS = ((2, 2), (0, 1), (1, 0), (3, 5), (6, 0))                                 # (n_freq, n_time); (2, 2) is also the [B, 8] table
SPECAUG_ROWS = 24
PLANTED = (np.uint32(0x7FC12345), np.uint32(0xC2F6E979), np.uint32(0x7F800000))           # NaN with a payload, -123.456, +inf

# one axis of one row: a pattern name -> its masks.  Rows: (channel-axis pattern, frame-axis pattern)
ROW_PATTERNS = (("none", "none"), ("end_exact", "none"), ("none", "end_exact"), ("one_at_0", "none"), ("none", "one_at_0"),
                ("overhang", "none"), ("none", "overhang"), ("neg_start", "none"), ("none", "neg_start"), ("overlap", "none"),
                ("none", "overlap"), ("identical", "none"), ("none", "identical"), ("whole", "none"), ("none", "whole"),
                ("end_exact", "end_exact"), ("one_at_0", "overhang"), ("neg_start", "one_at_0"), ("overlap", "identical"),
                ("overhang", "neg_start"), ("random", "random"), ("random", "random"), ("random", "none"), ("none", "random"))
assert len(ROW_PATTERNS) == SPECAUG_ROWS


SINGLE = ("end_exact", "one_at_0", "overhang", "neg_start", "whole")


def _axis_masks(pattern, L, K, r, rng, singles):
    """K {start, size} slots of an axis of length L.  Unused slots have size 0 or less and a start that would matter if the size were
    honoured; the patterns of one mask take the slots in turn (`singles` of them came before on this axis), so that every slot is the
    only live one of some row."""
    slots = [[1 + (k + r) % 3, 0 if (k + r) % 2 == 0 else -2] for k in range(K)]
    if K == 0 or pattern == "none":
        return slots
    k0 = singles % K
    k1 = (k0 + 1) % K
    mid = max(0, (L - 4) // 2)
    if pattern == "end_exact":
        size = min(2, L)
        slots[k0] = [L - size, size]
    elif pattern == "one_at_0":
        slots[k0] = [0, 1]
    elif pattern == "overhang":
        slots[k0] = [L - 1, 3]
    elif pattern == "neg_start":
        slots[k0] = [-1, 2]
    elif pattern == "overlap":
        slots[k0] = [mid, 3]
        slots[k1] = [mid + 1, 3]              # (one slot: the second mask alone)
    elif pattern == "identical":
        slots[k0] = [mid, 2]
        slots[k1] = [mid, 2]
    elif pattern == "whole":
        slots[k0] = [0, L]
    elif pattern == "random":                 # the host law's shape: inside the image, one or two wide, in every slot
        for k in range(K):
            size = int(rng.integers(1, min(2, L) + 1))
            slots[k] = [int(rng.integers(0, L - size + 1)), size]
    else:
        raise KeyError(pattern)
    return slots


@functools.lru_cache(maxsize=None)
def specaug_table(F, C, n_freq, n_time):
    """int32 [24, 2 * (n_freq + n_time)] in mkws_specaug_apply_n's layout, read-only."""
    rng = np.random.default_rng(3000 + 1000 * F + 10 * C + 7 * n_freq + n_time)
    rows, singles = [], [0, 0]
    for r, (pc, pf) in enumerate(ROW_PATTERNS):
        rows.append(sum(_axis_masks(pc, C, n_freq, r, rng, singles[0]) + _axis_masks(pf, F, n_time, r, rng, singles[1]), []))
        singles = [singles[0] + (pc in SINGLE), singles[1] + (pf in SINGLE)]
    masks = np.asarray(rows, dtype=np.int32).reshape(SPECAUG_ROWS, 2 * (n_freq + n_time))
    masks.setflags(write=False)
    return masks


def in_image(masks, F, C, n_freq, n_time):
    """bool [B]: every live mask of the row has 0 <= start and start + size <= its axis (what the host law draws)."""
    m = np.asarray(masks, dtype=np.int64).reshape(len(masks), n_freq + n_time, 2)
    L = np.asarray([C] * n_freq + [F] * n_time, dtype=np.int64)[None, :]
    live = m[..., 1] > 0
    return (~live | ((m[..., 0] >= 0) & (m[..., 0] + m[..., 1] <= L))).all(axis=1)


@functools.lru_cache(maxsize=None)
def specaug_case(F, C, n_freq, n_time):
    """-> (spec float32 [24, F, C], masks, expected, planted): the usual integers(1, 670) * 10 / 256 image with up to three PLANTED bit
    patterns at elements this table leaves alone (the last, the first and the middle one of them); planted = their flat indices."""
    masks = specaug_table(F, C, n_freq, n_time)
    spec = (np.random.default_rng(4000 + 100 * F + C).integers(1, 670, size=(SPECAUG_ROWS, F, C)).astype(np.float32) * np.float32(10 / 256))
    kept = np.flatnonzero(ref_specaug(spec, masks, n_freq, n_time).reshape(-1) != 0)
    planted = list(dict.fromkeys([int(kept[-1]), int(kept[0]), int(kept[len(kept) // 2])]))
    bits = spec.view(np.uint32).reshape(-1)
    for at, value in zip(planted, PLANTED):
        bits[at] = value
    expected = ref_specaug(spec, masks, n_freq, n_time)
    for a in (spec, expected):
        a.setflags(write=False)
    return spec, masks, expected, tuple(planted)
