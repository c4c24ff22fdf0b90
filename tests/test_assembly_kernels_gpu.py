"""-m gpu: augment_kernel, specaug_kernel and specaug_n_kernel (mkws_augment.hip) against the float64 references and the case tables of
tests/util_assembly_cases.py, through the C ABI.  tests/test_assembly_cases_cpu.py states what each group of cases is there for.

Bounds.  Modes 0 and 1 are bit for bit: a copy, and one correctly rounded float32 multiply of representable operands.  Mode 2 is held
to |got - ref64| <= 2e-6 * scale element by element (the bound of tests/test_pipeline_gpu.py; scale exceeds 1 only where the scaled
background does before the clip).  Spike items -- one foreground and one background sample -- are held to ONE float32 ulp of the result
(util_assembly_cases.spike_bound): their sums of squares are exact, so the ratio of the two RMS values is the only quantity that is
rounded more than once (two divisions by n, two square roots, one division; exactly 1.5 where n is a power of four, within one ulp of
it for every length of the table, as the float32 restatement of the CPU test shows), and their volumes are chosen so that nothing else
adds to it: 1.0 leaves the ratio itself in the output, 3.0 clips, and 0.05 is used only where both samples meet and 0.75 dominates.

Largest mode 2 deviation from the float64 reference measured on the MI355X, |got - ref64| / scale per clip length:
    n      1        2        255      256      257      2047     2048     2049     4097     9600     16000
           2.33e-8  2.54e-8  1.15e-7  7.93e-8  1.13e-7  1.04e-7  1.68e-7  1.58e-7  1.27e-7  1.48e-7  1.07e-7
(and 9.68e-8 on the dataset batch of the last test): the figures of the CPU test's float32 restatement, digit for digit -- the kernel
adds in the order that restatement states -- and a twelfth of the bound.
"""
import ctypes

import numpy as np
import pytest

from tests.util_assembly_cases import (AUGMENT_LENGTHS, BOUND, CONTRACT_CASES, SPECAUG_COUNTS, SPECAUG_ROWS, SPECAUG_SHAPES, augment_case,
                                       augment_expected, augment_sources, bg_stride_of, contract_case, ref_augment, ref_specaug,
                                       specaug_case, specaug_table, spike_bound)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INVALID_ARG = -1                         # MKWS_ERR_INVALID_ARG
CANARY = 0x7FC0FFEE                      # as float32: a NaN no kernel here produces
MARGIN = 64


def _lib():
    from multilingual_kws_amd import _lib as L
    return L


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()              # (a copy: the tables are read-only)


def _items_dev(items):
    return torch.from_numpy(np.ascontiguousarray(items).view(np.uint8).reshape(-1).copy()).cuda()


class _Guarded:
    """A float32 [rows, cols] view in the middle of a buffer filled with CANARY; the view starts `lead` floats into the allocation."""

    def __init__(self, rows, cols, lead=MARGIN):
        self.lead, self.size = lead, rows * cols
        self.flat = torch.full((lead + self.size + MARGIN + 1,), CANARY, dtype=torch.int32, device="cuda")
        self.view = self.flat[lead:lead + self.size].view(torch.float32).view(rows, cols)
        assert self.view.data_ptr() == self.flat.data_ptr() + 4 * lead

    def load(self, array):
        """The bits of a float32 host array into the view (copied as integers: a NaN keeps its payload)."""
        self.flat[self.lead:self.lead + self.size].copy_(torch.from_numpy(np.ascontiguousarray(array).view(np.int32).reshape(-1).copy()).cuda())

    def margins_intact(self):
        return bool((self.flat[:self.lead] == CANARY).all().cpu()) and bool((self.flat[self.lead + self.size:] == CANARY).all().cpu())


def _augment(n, bank0, bank1, bg, stride, items, d_src=None):
    """One mkws_augment_batch launch into a guarded output (at an odd float offset for odd n) -> float32 [B, n] on the host."""
    L = _lib()
    d_bank0, d_bank1, d_bg = d_src if d_src is not None else (_dev(bank0), _dev(bank1), _dev(bg))
    d_items = _items_dev(items)
    out = _Guarded(len(items), n, MARGIN + n % 2)
    assert n % 2 == 0 or (out.view.data_ptr() // 4) % 2 == 1
    L.check(L.lib().mkws_augment_batch(_p(d_bank0), _p(d_bank1), _p(d_bg), stride, _p(d_items), len(items), n, _p(out.view), L.current_stream_ptr()))
    torch.cuda.synchronize()
    got = out.view.cpu().numpy()
    assert out.margins_intact(), "mkws_augment_batch wrote outside d_out [B, n_samples]"
    assert not (got.view(np.int32) == CANARY).any(), "mkws_augment_batch left an element of d_out unwritten"
    return got


def _check_augment(got, ref, scale, items, tags, what):
    """The bounds of the module docstring on one launch -> largest mode 2 |got - ref64| / scale."""
    worst = 0.0
    for j, it in enumerate(items):
        if it["mode"] != 2:
            want = ref[j].astype(np.float32)
            assert np.array_equal(want.astype(np.float64), ref[j]) or it["mode"] == 1
            bad = np.flatnonzero(got[j].view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, f"{what} item {j} (mode {it['mode']}, {tags[j]}): {bad.size} samples differ, first at {bad[0]}: {got[j][bad[0]]!r} != {want[bad[0]]!r}"
            continue
        assert got[j].min() >= -1.0 and got[j].max() <= 1.0 and not np.isnan(got[j]).any(), (what, j)
        err = np.abs(got[j].astype(np.float64) - ref[j])
        bound = spike_bound(ref[j]) if tags[j].startswith("spike") else BOUND * scale[j]
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, (f"{what} item {j} ({tags[j]}, shift {it['shift']}, volume {it['bg_vol']}): {bad.size} samples out of bound, first at {bad[0]}: "
                               f"{got[j][bad[0]]!r} vs {ref[j][bad[0]]!r}, largest error {err.max():.3g} (scale {scale[j]:.3g})")
        worst = max(worst, float(err.max() / scale[j]))
    return worst


# ---------------------------------------------------------------------------------------------------
# augmentation
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", AUGMENT_LENGTHS)
def test_augment_against_the_float64_reference(n):
    bank0, bank1, bg = augment_sources(n)
    items, tags = augment_case(n)
    ref, scale = augment_expected(n)
    got = _augment(n, bank0, bank1, bg, bg_stride_of(n), items)
    worst = _check_augment(got, ref, scale, items, tags, f"n = {n}")
    print(f"n = {n}: {len(items)} items, largest mode 2 |got - ref64| / scale = {worst:.3g}")


@pytest.mark.parametrize("name", CONTRACT_CASES)
def test_augment_launches_the_contract_allows(name):
    """d_bank1 == NULL with every item in bank 0; d_bg == NULL and bg_stride == 0 with every item mode 0; B == 1."""
    n, bank0, bank1, bg, stride, items = contract_case(name)
    ref, scale = ref_augment(bank0, bank1, bg, stride, items, n)
    got = _augment(n, bank0, bank1, bg, stride, items)
    _check_augment(got, ref, scale, items, ["dense"] * len(items), name)


def test_augment_argument_checks():
    L = _lib()
    lib, stream = L.lib(), L.current_stream_ptr()
    n = 257
    bank0, bank1, bg = (_dev(a) for a in augment_sources(n))
    items = augment_case(n)[0][:4]
    d_items = _items_dev(items)
    out = _Guarded(4, n)
    stride = bg_stride_of(n)
    # B == 0: nothing to do, whatever the buffers
    assert lib.mkws_augment_batch(None, None, None, 0, None, 0, n, None, stream) == 0
    refused = [
        (_p(bank0), _p(bank1), _p(bg), stride, _p(d_items), -1, n, _p(out.view)),
        (_p(bank0), _p(bank1), _p(bg), stride, _p(d_items), 4, 0, _p(out.view)),
        (_p(bank0), _p(bank1), _p(bg), stride, _p(d_items), 4, -n, _p(out.view)),
        (_p(bank0), _p(bank1), _p(bg), stride, _p(d_items), 0, 0, _p(out.view)),       # the sample count is checked before B == 0 returns
        (_p(bank0), _p(bank1), _p(bg), stride, None, 4, n, _p(out.view)),
        (_p(bank0), _p(bank1), _p(bg), stride, _p(d_items), 4, n, None),
        (None, _p(bank1), _p(bg), stride, _p(d_items), 4, n, _p(out.view)),
    ]
    for args in refused:
        assert lib.mkws_augment_batch(*args, stream) == INVALID_ARG, args
        assert lib.mkws_last_error()
    torch.cuda.synchronize()
    assert bool((out.flat == CANARY).all().cpu())                                       # a refused call launches nothing


def test_augment_rows_never_interact():
    """The n = 2049 table in a permuted order, and its first 1 and 3 items alone: each row is the row of the whole launch, bit for bit."""
    n = 2049
    src = augment_sources(n)
    d_src = tuple(_dev(a) for a in src)
    items = augment_case(n)[0]
    whole = _augment(n, *src, bg_stride_of(n), items, d_src)
    perm = np.random.default_rng(7).permutation(len(items))
    assert (perm != np.arange(len(items))).sum() > len(items) // 2
    moved = _augment(n, *src, bg_stride_of(n), items[perm], d_src)
    assert np.array_equal(moved.view(np.uint32), whole[perm].view(np.uint32))
    for b in (1, 3):
        alone = _augment(n, *src, bg_stride_of(n), items[:b], d_src)
        assert np.array_equal(alone.view(np.uint32), whole[:b].view(np.uint32)), b
    last = _augment(n, *src, bg_stride_of(n), items[-1:], d_src)
    assert np.array_equal(last.view(np.uint32), whole[-1:].view(np.uint32))


# ---------------------------------------------------------------------------------------------------
# SpecAugment
# ---------------------------------------------------------------------------------------------------
def _specaug(spec, masks, nf, nt, eight=False, times=1):
    """mkws_specaug_apply_n(nf, nt) -- or, with `eight`, mkws_specaug_apply on the [B, 8] table -- in place on a guarded copy of spec,
    `times` times -> the uint32 view of the result on the host."""
    L = _lib()
    B, F, C = spec.shape
    buf = _Guarded(B, F * C, MARGIN + (F * C) % 2)
    buf.load(spec)
    d_masks = _dev(masks)
    for _ in range(times):
        if eight:
            L.check(L.lib().mkws_specaug_apply(_p(buf.view), _p(d_masks), B, F, C, L.current_stream_ptr()))
        else:
            L.check(L.lib().mkws_specaug_apply_n(_p(buf.view), _p(d_masks), nf, nt, B, F, C, L.current_stream_ptr()))
    torch.cuda.synchronize()
    assert buf.margins_intact(), "SpecAugment wrote outside d_spec [B, frames, channels]"
    return buf.view.view(torch.int32).cpu().numpy().view(np.uint32).reshape(B, F, C)


def _check_specaug(got, spec, expected, what):
    """Untouched elements keep their bits (the planted negative, inf and NaN payload among them); zeroed ones are +0.0 or -0.0."""
    zero = expected.view(np.uint32) == 0
    bad = np.argwhere((got & 0x7FFFFFFF != 0) & zero)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} elements the masks cover are not zero, first at (clip, frame, channel) {bad[0].tolist()}"
    bad = np.argwhere((got != spec.view(np.uint32)) & ~zero)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} elements outside the masks changed, first at (clip, frame, channel) {bad[0].tolist()}"


@pytest.mark.parametrize("shape", SPECAUG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_specaug_both_forms_against_the_index_sets(shape):
    F, C = shape
    spec, masks, expected, planted = specaug_case(F, C, 2, 2)
    assert masks.shape == (SPECAUG_ROWS, 8) and np.array_equal(expected, ref_specaug(spec, masks, 2, 2), equal_nan=True)
    got8 = _specaug(spec, masks, 2, 2, eight=True)
    _check_specaug(got8, spec, expected, f"{F} x {C} mkws_specaug_apply")
    got_n = _specaug(spec, masks, 2, 2)
    _check_specaug(got_n, spec, expected, f"{F} x {C} mkws_specaug_apply_n(2, 2)")
    assert np.array_equal(got8, got_n)                                                  # the same table, the same bytes
    assert np.array_equal(_specaug(spec, masks, 2, 2, eight=True, times=2), got8)       # idempotent
    assert np.array_equal(_specaug(spec, masks, 2, 2, times=2), got_n)
    for nf, nt in SPECAUG_COUNTS[1:]:
        spec, masks, expected, planted = specaug_case(F, C, nf, nt)
        assert np.array_equal(masks, specaug_table(F, C, nf, nt))
        got = _specaug(spec, masks, nf, nt)
        _check_specaug(got, spec, expected, f"{F} x {C} mkws_specaug_apply_n({nf}, {nt})")
        assert np.array_equal(_specaug(spec, masks, nf, nt, times=2), got)


def test_specaug_argument_checks():
    L = _lib()
    lib, stream = L.lib(), L.current_stream_ptr()
    spec, masks, _, _ = specaug_case(7, 36, 2, 2)
    buf = _Guarded(SPECAUG_ROWS, 7 * 36)
    buf.load(spec)
    before = buf.flat.clone()
    d_masks = _dev(masks)
    B = SPECAUG_ROWS
    for frames, channels in ((0, 36), (7, 0), (-7, 36), (7, -36)):
        assert lib.mkws_specaug_apply(_p(buf.view), _p(d_masks), B, frames, channels, stream) == INVALID_ARG
        assert lib.mkws_specaug_apply_n(_p(buf.view), _p(d_masks), 2, 2, B, frames, channels, stream) == INVALID_ARG
    assert lib.mkws_specaug_apply(_p(buf.view), _p(d_masks), -1, 7, 36, stream) == INVALID_ARG
    assert lib.mkws_specaug_apply(None, _p(d_masks), B, 7, 36, stream) == INVALID_ARG
    assert lib.mkws_specaug_apply(_p(buf.view), None, B, 7, 36, stream) == INVALID_ARG
    for nf, nt in ((-1, 2), (2, -1), (-1, -1), (-2, 2)):
        assert lib.mkws_specaug_apply_n(_p(buf.view), _p(d_masks), nf, nt, B, 7, 36, stream) == INVALID_ARG
    assert lib.mkws_specaug_apply_n(_p(buf.view), _p(d_masks), 2, 2, -1, 7, 36, stream) == INVALID_ARG
    assert lib.mkws_specaug_apply_n(None, _p(d_masks), 2, 2, B, 7, 36, stream) == INVALID_ARG
    assert lib.mkws_specaug_apply_n(_p(buf.view), None, 2, 2, B, 7, 36, stream) == INVALID_ARG
    # nothing to do: B == 0 with NULL buffers; no masks at all with a NULL table, the spectrogram untouched
    assert lib.mkws_specaug_apply(None, None, 0, 7, 36, stream) == 0
    assert lib.mkws_specaug_apply_n(None, None, 2, 2, 0, 7, 36, stream) == 0
    assert lib.mkws_specaug_apply_n(_p(buf.view), None, 0, 0, B, 7, 36, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf.flat, before)


# ---------------------------------------------------------------------------------------------------
# the three launches as they run in a training step
# ---------------------------------------------------------------------------------------------------
def test_the_assembly_chain_in_one_captured_graph():
    """mkws_augment_batch -> Frontend.forward -> mkws_specaug_apply_n on fixed buffers, captured once and replayed three times with the
    item and mask tables overwritten in place: every replay equals the eager chain on that table, bit for bit.  (One stream, one
    launch after the other: the graph has no parallel branches.)"""
    from multilingual_kws_amd.frontend import Frontend
    L = _lib()
    n, B, F, C = 16000, 8, 49, 40
    bank0, bank1, bg = (_dev(a) for a in augment_sources(n))
    items = augment_case(n)[0]
    masks = specaug_table(F, C, 2, 2)
    # three tables of eight: shifts and mixes in the first, all three modes in the others, the spike items in the last
    first_mode1 = int(np.flatnonzero(items["mode"] == 1)[0])
    picks = [np.arange(k, k + 8 * 6, 6) for k in (0, 1)] + [np.concatenate([[first_mode1 - 1, first_mode1], np.arange(len(items) - 6, len(items))])]
    assert [sorted(set(items[p]["mode"].tolist())) for p in picks] == [[0, 2], [0, 1, 2], [0, 1, 2]]
    tables = [(items[p], masks[8 * k:8 * k + 8]) for k, p in enumerate(picks)]
    fe = Frontend(max_samples=n)

    def chain(d_items, d_masks, audio, spec):
        L.check(L.lib().mkws_augment_batch(_p(bank0), _p(bank1), _p(bg), bg_stride_of(n), _p(d_items), B, n, _p(audio), L.current_stream_ptr()))
        fe.forward(audio, out=spec)
        L.check(L.lib().mkws_specaug_apply_n(_p(spec), _p(d_masks), 2, 2, B, F, C, L.current_stream_ptr()))

    eager = []
    for it, m in tables:
        audio, spec = torch.empty((B, n), dtype=torch.float32, device="cuda"), torch.empty((B, F, C), dtype=torch.float32, device="cuda")
        chain(_items_dev(it), _dev(m), audio, spec)
        eager.append((audio.clone(), spec.clone()))
    assert not torch.equal(eager[0][1], eager[1][1]) and not torch.equal(eager[1][1], eager[2][1])
    assert all(bool((s == 0).any().cpu()) and bool((s != 0).any().cpu()) for _, s in eager)
    s_items, s_masks = _items_dev(tables[0][0]), _dev(tables[0][1])
    s_audio, s_spec = torch.zeros((B, n), dtype=torch.float32, device="cuda"), torch.zeros((B, F, C), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(s_items, s_masks, s_audio, s_spec)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(s_items, s_masks, s_audio, s_spec)
    for k in (1, 2, 0):
        s_items.copy_(_items_dev(tables[k][0]))
        s_masks.copy_(_dev(tables[k][1]))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_audio.view(torch.int32), eager[k][0].view(torch.int32)), k
        assert torch.equal(s_spec.view(torch.int32), eager[k][1].view(torch.int32)), k
    del g
    fe.close()


def test_a_dataset_away_from_16000_samples(tmp_path):
    """600 ms clips, 33 channels (9600 samples, a 29 x 33 image) through AudioDataset: last_audio is ref_augment on the items a second,
    identically seeded dataset draws, and the batch is ref_specaug of the frontend's output on last_audio, bit for bit."""
    from multilingual_kws_amd.embedding import input_data
    from tests.util_data import make_fewshot_dataset
    data = make_fewshot_dataset(str(tmp_path / "fewshot"))
    ms = input_data.prepare_model_settings(3, 16000, 600, 30, 20, 33, "micro")
    n, B = ms["desired_samples"], 64
    assert (n, ms["spectrogram_length"], ms["fingerprint_width"]) == (9600, 29, 33)

    def dataset():
        ds = input_data.AudioDataset(ms, ["target"], data["bg_dir"], data["unknown"], unknown_percentage=50.0, background_volume_range=1.0,
                                     spec_aug_params=input_data.SpecAugParams(percentage=100), seed=9)
        return ds, ds.init_single_target(input_data.AUTOTUNE, data["train"], is_training=True).shuffle(1000).repeat().batch(B)

    ds, train = dataset()
    spec, labels = next(iter(train))
    assert spec.shape == (B, 29, 33, 1) and labels.shape == (B,)
    # the same draws, on the host only
    ds2, train2 = dataset()
    items, labels2, masks = ds2._draw_batch(train2, input_data.BatchGroups(train2)._next_indices(), [])
    assert np.array_equal(labels.cpu().numpy(), labels2) and np.array_equal(ds.last_masks, masks)
    assert set(items["mode"].tolist()) == {0, 1, 2} and set(items["bank"].tolist()) == {0, 1} and (np.abs(items["shift"]) < 1600).all()
    bank0 = np.stack([input_data._read_wav(f, n) for f in data["train"]])
    bank1 = np.stack([input_data._read_wav(f, n) for f in data["unknown"]])
    bg = ds2.background_host
    ref, scale = ref_augment(bank0, bank1, bg, bg.shape[1], items, n)
    got = ds.last_audio.cpu().numpy()
    worst = _check_augment(got, ref, scale, items, ["dense"] * B, "dataset batch")
    print(f"dataset batch at n = {n}: largest mode 2 |got - ref64| / scale = {worst:.3g}")
    # SpecAugment on the 29 x 33 image
    clean = input_data.to_micro_spectrogram(ms, ds.last_audio).cpu().numpy()
    assert masks.shape == (B, 8) and (masks[:, 1::2] > 0).any(axis=1).sum() > B // 2
    want = ref_specaug(clean, masks, 2, 2)
    assert (want == 0).any() and np.array_equal(spec[..., 0].cpu().numpy().view(np.uint32), want.view(np.uint32))
