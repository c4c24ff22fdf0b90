"""What the batch-assembly case tables (tests/util_assembly_cases.py) are for, and that their float64 references are the product's
semantics: ref_augment against input_data.add_background composed with AudioDataset._timeshift_host, ref_specaug against the host masking
of tests/test_finetune_gpu.py, and a float32 restatement of augment_kernel's mode 2 arithmetic that shows the 2e-6 bound of
tests/test_assembly_kernels_gpu.py is one the float64 reference can be held to.  No GPU needed.  Fails when a table is edited so that a
case it exists for is no longer in it."""
import types

import numpy as np
import pytest

from tests.util_assembly_cases import (AUGMENT_LENGTHS, BOUND, CONTRACT_CASES, ITEM_DTYPE, PLANTED, ROW_PATTERNS, SPECAUG_COUNTS,
                                       SPECAUG_ROWS, SPECAUG_SHAPES, SPIKE_POSITIONS, VOLUMES, augment_case, augment_expected,
                                       augment_sources, bg_stride_of, contract_case, dense_shifts, in_image, ref_augment, ref_specaug,
                                       shifted, specaug_case, specaug_table, spike_bound, spike_positions)


def _slice(bg, it, n):
    return bg[it["bg_idx"], it["bg_off"]:it["bg_off"] + n]


# ---------------------------------------------------------------------------------------------------
# the references are the product's host semantics
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", AUGMENT_LENGTHS)
def test_ref_augment_is_the_host_arithmetic(n):
    """Dense items with |shift| < n: mode 0 == _timeshift_host and mode 1 == slice * float32(volume) exactly; mode 2 == add_background
    (float32 numpy) of the shifted clip within the bound the device is held to."""
    from multilingual_kws_amd.embedding import input_data
    assert ITEM_DTYPE == input_data._ITEM_DTYPE
    bank0, bank1, bg = augment_sources(n)
    items, tags = augment_case(n)
    ref, scale = augment_expected(n)
    seen = set()
    for j, it in enumerate(items):
        if tags[j] != "dense" or (it["mode"] != 1 and abs(int(it["shift"])) >= n):
            continue
        seen.add(int(it["mode"]))
        if it["mode"] == 1:
            host = _slice(bg, it, n) * np.float32(it["bg_vol"])                        # _background_sample_host's product
            assert host.dtype == np.float32 and np.array_equal(ref[j].astype(np.float32), host), j
            continue
        fg = (bank0 if it["bank"] == 0 else bank1)[it["src"]]
        stub = types.SimpleNamespace(_draw_shift=lambda a=int(it["shift"]): a, model_settings={"desired_samples": n})
        moved = input_data.AudioDataset._timeshift_host(stub, fg)
        assert np.array_equal(moved, shifted(fg, int(it["shift"])))
        if it["mode"] == 0:
            assert np.array_equal(ref[j], moved.astype(np.float64)), j
        else:
            host = input_data.add_background(moved, _slice(bg, it, n), float(it["bg_vol"]))
            assert host.dtype == np.float32 and (np.abs(host - ref[j]) <= BOUND * scale[j]).all(), (j, np.abs(host - ref[j]).max())
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("shape", SPECAUG_SHAPES)
def test_ref_specaug_is_the_host_masking(shape):
    """On rows whose masks lie inside the image -- all the host law can draw -- ref_specaug equals _apply_masks, bit for bit."""
    from tests.test_finetune_gpu import _apply_masks
    F, C = shape
    for nf, nt in SPECAUG_COUNTS:
        spec, masks, expected, _ = specaug_case(F, C, nf, nt)
        rows = np.flatnonzero(in_image(masks, F, C, nf, nt))
        assert len(rows) >= 8 and not in_image(masks, F, C, nf, nt).all()
        host = _apply_masks(spec[rows], masks[rows], nf, nt)
        assert np.array_equal(host.view(np.uint32), expected[rows].view(np.uint32)), (shape, nf, nt)


# ---------------------------------------------------------------------------------------------------
# the float64 reference stays inside the device's bound
# ---------------------------------------------------------------------------------------------------
def _block_sum_f32(per_thread):
    """block_sum of mkws_augment.hip on 256 float32 partial sums: xor butterfly over each wave's 64 lanes, then (s0 + s1) + (s2 + s3)."""
    v = per_thread.astype(np.float32).reshape(4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ off]).astype(np.float32)
    s = v[:, 0]
    return np.float32(np.float32(s[0] + s[1]) + np.float32(s[2] + s[3]))


def _thread_sums_f32(x):
    """Thread t adds the squares of samples t, t + 256, ... one after the other, in float32."""
    n = x.shape[0]
    pad = np.zeros(-(-n // 256) * 256, dtype=np.float32)
    pad[:n] = x
    sq = (pad * pad).astype(np.float32).reshape(-1, 256)
    acc = np.zeros(256, dtype=np.float32)
    for row in sq:
        acc = (acc + row).astype(np.float32)
    return acc


def _mode2_f32(fg, bg, vol):
    """augment_kernel's mode 2 in float32 numpy, operation for operation (the library is built without contraction, and division and
    square root are correctly rounded on both sides)."""
    n = np.float32(fg.shape[0])
    fg_rms = np.sqrt(np.float32(_block_sum_f32(_thread_sums_f32(fg)) / n), dtype=np.float32)
    bg_rms = np.sqrt(np.float32(_block_sum_f32(_thread_sums_f32(bg)) / n), dtype=np.float32)
    snr = np.float32(fg_rms / bg_rms) if bg_rms > 0 else np.float32(0)
    v = ((bg * snr).astype(np.float32) * np.float32(vol)).astype(np.float32) + fg
    return np.minimum(np.maximum(v.astype(np.float32), np.float32(-1)), np.float32(1))


@pytest.mark.parametrize("n", AUGMENT_LENGTHS)
def test_a_float32_restatement_of_the_kernel_meets_the_bound(n):
    """|restatement - ref64| <= 2e-6 * scale on every mode 2 item, and at most one ulp on the spike items: the bounds of the device
    test are ones a faithful float32 kernel meets, with room (the largest difference is printed; about 2e-7 on dense clips)."""
    bank0, bank1, bg = augment_sources(n)
    items, tags = augment_case(n)
    ref, scale = augment_expected(n)
    worst = 0.0
    for j, it in enumerate(items):
        if it["mode"] != 2:
            continue
        fg = shifted((bank0 if it["bank"] == 0 else bank1)[it["src"]], int(it["shift"]))
        got = _mode2_f32(fg, _slice(bg, it, n), it["bg_vol"])
        err = np.abs(got.astype(np.float64) - ref[j])
        assert (err <= BOUND * scale[j]).all(), (n, j, tags[j], err.max(), scale[j])
        assert got.min() >= -1 and got.max() <= 1
        if tags[j].startswith("spike"):
            assert (err <= spike_bound(ref[j])).all(), (n, j, tags[j], err.max())
        worst = max(worst, float((err / scale[j]).max()))
    print(f"n = {n}: largest |float32 restatement - float64 reference| / scale = {worst:.3g}")
    assert worst <= BOUND / 4


# ---------------------------------------------------------------------------------------------------
# the tables hold what they exist for
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", AUGMENT_LENGTHS)
def test_the_augmentation_table_of_every_length(n):
    bank0, bank1, bg = augment_sources(n)
    items, tags = augment_case(n)
    ref, scale = augment_expected(n)
    stride = bg_stride_of(n)
    assert bank0.shape == (3, n) and bank1.shape == (2, n) and bg.shape == (2, stride) and stride == 2 * n + 37 and len(items) <= 64
    # sources: the int16 grid, never zero on the dense stretches, amplitudes about 0.5 and 0.3
    for a in (bank0, bank1, bg):
        assert a.dtype == np.float32 and np.array_equal(a * 32768, np.round(a * 32768))
    dense_fg, dense_bg = np.concatenate([bank0[:2].ravel(), bank1.ravel()]), bg[1, :n + 37]
    assert (dense_fg != 0).all() and (dense_bg != 0).all() and np.abs(dense_fg).max() <= 0.5 and np.abs(dense_bg).max() <= 0.3
    if n >= 255:
        assert np.abs(dense_fg).max() > 0.49 and np.abs(dense_bg).max() > 0.29
    assert np.count_nonzero(bank0[2]) == 1 and np.count_nonzero(bg[0]) == 1 and (bg[1, n + 37:] == np.float32(1 / 32768)).all()
    # every item names a row of its bank and a slice inside its track, so no launch of the table reads out of bounds
    assert ((items["bank"] == 0) & (items["src"] < 3) | (items["bank"] == 1) & (items["src"] < 2)).all() and (items["src"] >= 0).all()
    assert (items["bg_idx"] >= 0).all() and (items["bg_idx"] < 2).all() and (items["bg_off"] >= 0).all() and (items["bg_off"] + n <= stride).all()
    assert (items["bg_vol"][items["mode"] != 0] >= 1e-3).all()                          # no product is subnormal
    # every mode with both banks, the last row of each bank in every mode, both tracks
    for mode in (0, 1, 2):
        m = items[items["mode"] == mode]
        assert {(0, 2), (1, 1)} <= set(zip(m["bank"].tolist(), m["src"].tolist())), mode
    assert set(items["bg_idx"][items["mode"] != 0].tolist()) == {0, 1}
    last = items[(items["bg_idx"] == 1) & (items["mode"] != 0)]
    assert 0 in last["bg_off"] and stride - n in last["bg_off"]                         # a slice ending on the last sample of the last track
    # the shifts, on mode 0 and on mode 2
    want = {0, 1, -1, n - 1, 1 - n, n, -n, n + 5, -n - 5} | {s * k for s in (255, 256, 2047, 2048) if s < n for k in (1, -1)}
    assert want <= set(dense_shifts(n)) and len(set(dense_shifts(n)) - want) >= (2 if n > 2 else 0)
    for mode in (0, 2):
        assert set(dense_shifts(n)) <= set(items["shift"][items["mode"] == mode].tolist())
    assert {np.float32(v) for v in VOLUMES} == set(items["bg_vol"][items["mode"] == 2].tolist())
    # mode 2: clipping at both signs, both degenerate RMS values, the tiny background under a loud clip
    m2 = np.flatnonzero(items["mode"] == 2)
    assert any((ref[j] == 1).any() for j in m2) and any((ref[j] == -1).any() for j in m2)
    assert (ref[tags.index("clip+")] == 1).any() and (ref[tags.index("clip-")] == -1).any()
    assert (scale >= 1).all() and (scale[items["mode"] != 2] == 1).all() and ((scale > 1.4).any() or n <= 2)     # the bound is widened somewhere
    j = tags.index("zero_bg")
    assert not _slice(bg, items[j], n).any() and ref[j].any() and np.array_equal(ref[j], shifted(bank1[1], items[j]["shift"]))
    for j in (k for k, t in enumerate(tags) if t == "fg_out"):
        assert abs(items[j]["shift"]) >= n and _slice(bg, items[j], n).all() and not ref[j].any()
    j = tags.index("tiny_bg")
    sl = _slice(bg, items[j], n)
    snr = np.sqrt(np.mean(np.square(bank0[0], dtype=np.float64))) * 32768
    assert (sl == np.float32(1 / 32768)).all() and items[j]["bg_vol"] == np.float32(0.05) and (snr > 3000 if n > 2 else snr >= 1)
    # spikes: the foreground sample lands on every listed position and so does the background's
    ps, qs = set(), set()
    for j, t in enumerate(tags):
        if not t.startswith("spike "):
            continue
        p, q = (int(x) for x in t.split()[1:])
        fg = shifted(bank0[2], int(items[j]["shift"]))
        sl = _slice(bg, items[j], n)
        assert items[j]["mode"] == 2 and np.flatnonzero(fg).tolist() == [p] and fg[p] == 0.75 and np.flatnonzero(sl).tolist() == [q] and sl[q] == -0.5
        ps.add(p)
        qs.add(q)
    assert ps == qs == set(spike_positions(n)) == {p for p in SPIKE_POSITIONS if p < n} | {n - 1}
    assert any(items[j]["shift"] > 0 for j, t in enumerate(tags) if t.startswith(f"spike {n - 1} ")) or n == 1   # a shift moves it to n - 1
    outs = [j for j, t in enumerate(tags) if t.startswith("spike_out")]
    assert len(outs) == 2 and {int(np.sign(items[j]["shift"])) for j in outs} == {1, -1}
    for j in outs:                                                                      # one sample past the clip: the RMS after the shift is 0
        assert items[j]["bank"] == 0 and items[j]["src"] == 2 and not shifted(bank0[2], int(items[j]["shift"])).any() and not ref[j].any()
        assert shifted(bank0[2], int(items[j]["shift"]) - int(np.sign(items[j]["shift"]))).any() and _slice(bg, items[j], n).any()
    # the 8-wide pass of 2048 samples: none, exactly one, one and a sample; above 2048 the last pass is partial
    if n > 2048:
        assert n % 2048 != 0
    # rows off the 8-byte boundary: every second bank row of an odd length, and the last track always
    assert stride % 2 == 1
    if n % 2 == 1 and n > 1:
        assert any((it["src"] * n) % 2 == 1 for it in items)
    assert any((it["bg_idx"] * stride + it["bg_off"]) % 2 == 1 for it in items[items["mode"] != 0])


def test_the_lengths_and_the_contract_table():
    assert {255, 256, 257, 2047, 2048, 2049} <= set(AUGMENT_LENGTHS) and min(AUGMENT_LENGTHS) == 1 and max(AUGMENT_LENGTHS) == 16000
    assert any(n % 2 == 1 and n > 2048 for n in AUGMENT_LENGTHS) and 9600 in AUGMENT_LENGTHS
    assert CONTRACT_CASES == ("null_bank1", "null_bg", "one_item")
    n, bank0, bank1, bg, stride, items = contract_case("null_bank1")
    assert bank1 is None and bg is not None and (items["bank"] == 0).all() and set(items["mode"].tolist()) == {0, 1, 2} and len(items) > 8
    n, bank0, bank1, bg, stride, items = contract_case("null_bg")
    assert bg is None and stride == 0 and (items["mode"] == 0).all() and set(items["bank"].tolist()) == {0, 1} and len(items) > 8
    n, bank0, bank1, bg, stride, items = contract_case("one_item")
    assert len(items) == 1 and items[0]["mode"] == 2


@pytest.mark.parametrize("shape", SPECAUG_SHAPES)
def test_the_specaugment_tables(shape):
    F, C = shape
    assert SPECAUG_COUNTS[0] == (2, 2) and set(SPECAUG_COUNTS) == {(2, 2), (0, 1), (1, 0), (3, 5), (6, 0)}
    for nf, nt in SPECAUG_COUNTS:
        spec, masks, expected, planted = specaug_case(F, C, nf, nt)
        assert masks.shape == (SPECAUG_ROWS, 2 * (nf + nt)) and masks.dtype == np.int32 and spec.shape == (SPECAUG_ROWS, F, C)
        assert np.array_equal(masks, specaug_table(F, C, nf, nt))
        m = masks.reshape(SPECAUG_ROWS, nf + nt, 2).astype(np.int64)
        axis_len = np.asarray([C] * nf + [F] * nt)
        start, size, end = m[..., 0], m[..., 1], m[..., 0] + m[..., 1]
        live = size > 0
        chan, frame = np.arange(nf + nt) < nf, np.arange(nf + nt) >= nf
        # the edge rows, on each axis that has masks
        assert not live[0].any() and (start[0] != 0).all() and (size <= 0).all(axis=1).sum() >= 1      # all sizes zero or less, nonzero starts
        assert (size < 0).any()
        for axis in ([chan] if nf else []) + ([frame] if nt else []):
            a = live & axis[None, :]
            assert (a & (end == axis_len[None, :])).any()                                  # ends exactly on the last channel / frame
            assert (a & (start == 0) & (size == 1)).any()                                  # one pixel wide at index 0
            assert (a & (end > axis_len[None, :])).any()                                   # start + size past the edge
            assert (a & (start == -1) & (size == 2)).any()                                 # start -1, size 2
            assert (a & (start == 0) & (size == axis_len[None, :])).any()                  # the whole axis
            assert (a.any(axis=1) & ~(live & ~axis[None, :]).any(axis=1)).any()            # a row with masks on this axis only
            for k in range(nf + nt):                                                       # every slot is the only live one of some row
                if axis[k]:
                    assert (a[:, k] & (a.sum(axis=1) == 1)).any(), (nf, nt, k)
            if axis.sum() >= 2:
                ks = np.flatnonzero(axis)
                same = overlap = False
                for r in range(SPECAUG_ROWS):
                    for i in ks:
                        for j in ks:
                            if i < j and live[r, i] and live[r, j]:
                                same |= bool(start[r, i] == start[r, j] and size[r, i] == size[r, j])
                                overlap |= bool(start[r, i] != start[r, j] and max(start[r, i], start[r, j]) < min(end[r, i], end[r, j]))
                assert same and (overlap or axis_len[ks[0]] == 1)                          # two identical masks; two overlapping ones
        # masked and unmasked elements, and the planted bit patterns where the table leaves them alone
        bits = expected.view(np.uint32)
        zero = bits == 0
        if shape != (1, 1):
            assert len(planted) == 3 and sum(zero[r].any() and (~zero[r]).any() for r in range(SPECAUG_ROWS)) >= 6
        assert zero.any() and (~zero).any() and not zero[0].any()
        assert [int(b) for b in bits.reshape(-1)[list(planted)]] == [int(v) for v in PLANTED[:len(planted)]]
        assert np.array_equal(spec.view(np.uint32)[~zero], bits[~zero]) and np.isnan(spec).sum() == 1 and np.isinf(spec).sum() == (len(planted) == 3)
        assert len(planted) < 2 or spec.reshape(-1)[planted[1]] < 0
    assert len(ROW_PATTERNS) == SPECAUG_ROWS == 24
    assert {7 * 36, 8 * 32} == {252, 256} and (7, 36) in SPECAUG_SHAPES and (8, 32) in SPECAUG_SHAPES
