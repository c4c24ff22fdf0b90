"""Classification ROC on the device (mkws_roc_count / roc.roc_counts_on_device / transfer_learning_analysis.roc_many /
transfer_learning.evaluate_files_many / classification_curves) against the host specification (roc_single_target, roc_sc).
Every comparison is exact: the device counts integers with the comparison the host makes -- (float64)score > threshold -- and the
rates are quotients of those integers formed in Python on both sides.  A rate count / total determines the count (total < 2^24), so
equal rates are equal counts."""
import json
import os

import numpy as np
import pytest

from multilingual_kws_amd.embedding import transfer_learning_analysis as tla

THRESHS = np.arange(0, 1.01, 0.01)
SHAPES = [(1, 1), (3, 63), (3, 257), (65, 64), (2, 5000)]


def near_threshold_scores(rng, shape):
    """float32 scores drawn from {float32(thr), one ulp below, one ulp above} of the 101 default thresholds."""
    thr = THRESHS[rng.integers(0, 101, shape)].astype(np.float32)
    step = rng.integers(-1, 2, shape)
    return np.where(step < 0, np.nextafter(thr, np.float32(-1)), np.where(step > 0, np.nextafter(thr, np.float32(2)), thr)).astype(np.float32)


_CASES = {}


def yardstick_case(K, N):
    """probs [K, N, 3] and per-head row lists: duplicates, head 0's positive list longer than N, lengths that are no multiple of 64, and
    (from two heads on) head 1 without positives and head 0 without negatives.  Built once per shape and left unchanged."""
    if (K, N) not in _CASES:
        rng = np.random.default_rng(1000 * K + N)
        probs = near_threshold_scores(rng, (K, N, 3))
        pos = [[int(r) for r in rng.integers(0, N, int(rng.integers(30, max(31, 2 * N)) | 1))] for _ in range(K)]
        neg = [[int(r) for r in rng.integers(0, N, int(rng.integers(30, max(31, 2 * N)) | 1))] for _ in range(K)]
        pos[0] = [int(r) for r in rng.integers(0, N, N + 7)]
        if K >= 2:
            pos[1], neg[0] = [], []
        _CASES[(K, N)] = (probs, pos, neg)
    return _CASES[(K, N)]


def host_rates(p, pos, neg, multiclass=False, pos_class=2, neg_class=1):
    """(tprs or None, fprs or None) of one head by the host functions, a side at a time so that an empty other side does not matter."""
    one = dict(correct=[1.0], incorrect=[])
    tprs = fprs = None
    if len(pos):
        tprs = tla.roc_sc(tla.split_confidences(p[pos], pos_class), one)[0] if multiclass else tla.roc_single_target(p[pos, pos_class], np.ones(1, np.float32))[0]
    if len(neg):
        fprs = tla.roc_sc(one, tla.split_confidences(p[neg], neg_class))[1] if multiclass else tla.roc_single_target(np.ones(1, np.float32), p[neg, pos_class])[1]
    return tprs, fprs


def assert_counts_are_the_host_rates(counts, probs, pos, neg, **mode):
    """counts int [K, 101, 2] at the default thresholds."""
    counts = np.asarray(counts).tolist()
    for k in range(len(pos)):
        tprs, fprs = host_rates(probs[k], pos[k], neg[k], **mode)
        for side, rates, rows in ((0, tprs, pos[k]), (1, fprs, neg[k])):
            got = [c[side] for c in counts[k]]
            if rates is None:
                assert got == [0] * len(got), (k, side)
            else:
                assert [c / len(rows) for c in got] == rates, (k, side, mode)


def raw_call(torch, probs, pos, neg, thresholds, mode=0, pos_class=2, neg_class=1, n_rows=None):
    """mkws_roc_count on unchecked lists -> (code, counts [K, T, 2], invalid [K]); the outputs start at -9."""
    from multilingual_kws_amd import _lib
    K = len(pos)
    C = probs.shape[2]
    N = probs.shape[1] if n_rows is None else n_rows

    def pack(lists):
        rows = np.asarray([r for l in lists for r in l] + [0], np.int32)       # (one spare word: never an empty allocation)
        off = np.zeros(K + 1, np.int32)
        np.cumsum([len(l) for l in lists], out=off[1:])
        return torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda()
    d_pos, d_pos_off = pack(pos)
    d_neg, d_neg_off = pack(neg)
    thr = np.asarray(thresholds, np.float64)
    d_thr = torch.from_numpy(thr).cuda()
    d_probs = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda() if probs.size else torch.zeros(1, device="cuda")
    d_counts = torch.full((K, thr.size, 2), -9, dtype=torch.int32, device="cuda")
    d_invalid = torch.full((max(K, 1),), -9, dtype=torch.int32, device="cuda")
    code = _lib.lib().mkws_roc_count(d_probs.data_ptr() if N != 0 else None, K, N, C, d_pos.data_ptr(), d_pos_off.data_ptr(),
                                     d_neg.data_ptr(), d_neg_off.data_ptr(), d_thr.data_ptr(), thr.size, mode, pos_class, neg_class,
                                     d_counts.data_ptr(), d_invalid.data_ptr(), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return code, d_counts.cpu().numpy(), d_invalid.cpu().numpy()[:K]


def counts_in_float64(scores_pos, scores_neg, thresholds):
    """The rule itself, for thresholds the host functions do not take: entries with (float64)score > threshold."""
    a, b = np.asarray(scores_pos, np.float64), np.asarray(scores_neg, np.float64)
    return np.asarray([[np.count_nonzero(a > t), np.count_nonzero(b > t)] for t in np.asarray(thresholds, np.float64)], np.int32)


# ------------------------------------------------------------------------------------------------ the cases are worth running

@pytest.mark.parametrize("K,N", SHAPES[1:])
def test_counting_in_float32_would_change_every_head(K, N):
    """Host only.  A kernel that compared in float32 must fail the yardstick on every head of every shape but (1, 1)."""
    probs, pos, neg = yardstick_case(K, N)
    thr32 = THRESHS.astype(np.float32)
    for k in range(K):
        s = np.concatenate([probs[k][pos[k], 2], probs[k][neg[k], 2]])
        in32 = [np.count_nonzero(s > t) for t in thr32]
        in64 = [np.count_nonzero(s.astype(np.float64) > t) for t in THRESHS]
        assert in32 != in64, k


def test_yardstick_lists_have_the_awkward_shapes():
    for K, N in SHAPES:
        probs, pos, neg = yardstick_case(K, N)
        assert len(pos[0]) > N and len(set(pos[0])) < len(pos[0])
        if K >= 2:
            assert pos[1] == [] and neg[0] == [] and len(neg[1]) % 64 and len(pos[0]) % 64
            assert any(o % 64 for o in np.cumsum([len(x) for x in pos]))


# ------------------------------------------------------------------------------------------------ the C call

@pytest.mark.gpu
def test_raw_call_reproduces_the_reference_vectors(golden_dir):
    torch = pytest.importorskip("torch")
    cases = json.load(open(os.path.join(golden_dir, "roc_golden.json")))["cases"]
    assert len(cases) == 12
    for c in cases:
        p = np.asarray(c["probs"], np.float32)[None]
        neg = sum((c["groups"][k] for k in ("oov", "unknown_training", "original_embedding")), []) if "groups" in c else c["negatives"]
        mode = int(c["function"] != "roc_single_target")
        code, counts, invalid = raw_call(torch, p, [c["positives"]], [neg], THRESHS, mode, c["target_id"], c.get("negative_class", 0))
        assert code == 0 and invalid.tolist() == [0]
        got = counts[0].tolist()
        assert [x[0] / len(c["positives"]) for x in got] == c["tprs"] and [x[1] / len(neg) for x in got] == c["fprs"], c["function"]


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", SHAPES)
def test_device_counts_equal_roc_single_target(K, N):
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd.roc import roc_counts_on_device
    probs, pos, neg = yardstick_case(K, N)
    code, counts, invalid = raw_call(torch, probs, pos, neg, THRESHS)
    assert code == 0 and not invalid.any()
    assert_counts_are_the_host_rates(counts, probs, pos, neg)
    wrapped, totals = roc_counts_on_device(torch.from_numpy(probs).cuda(), pos, neg, THRESHS)
    assert np.array_equal(wrapped, counts) and wrapped.dtype == totals.dtype == np.int32
    assert totals.tolist() == [[len(a), len(b)] for a, b in zip(pos, neg)]
    again = raw_call(torch, probs, pos, neg, THRESHS)[1]
    assert np.array_equal(again, counts)                                       # the same on every run


def _multiclass_table(rng, N, C):
    """Near-threshold winners, ties between two winning classes in both orders (rows 0, 4, 8, ...), rows holding a NaN (rows 2, 12, ...)."""
    win = near_threshold_scores(rng, N)
    p = (win[:, None] * rng.uniform(0, 0.9, (N, C))).astype(np.float32)
    p[np.arange(N), rng.integers(0, C, N)] = win
    for r in range(0, N, 4):
        a, b = rng.choice(C, 2, replace=False)
        p[r, a] = p[r, b] = p[r].max()
    for r in range(2, N, 10):
        p[r, int(rng.integers(0, C))] = np.nan
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 3, 8])
def test_argmax_mode_equals_roc_sc(C):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(40 + C)
    K, N = 3, 97
    probs = np.stack([_multiclass_table(rng, N, C) for _ in range(K)])
    assert np.isnan(probs).any(axis=2).sum() >= 3 * K
    pos = [[int(r) for r in rng.integers(0, N, n)] for n in (131, 50, 77)]
    neg = [[int(r) for r in rng.integers(0, N, n)] for n in (45, 201, 99)]
    pairs = [(a, b) for a in range(C) for b in range(C)] if C == 3 else [(C - 1, 0), (0, C - 1), (1, 1)]
    for pc, nc in pairs:
        code, counts, invalid = raw_call(torch, probs, pos, neg, THRESHS, 1, pc, nc)
        assert code == 0 and not invalid.any()
        assert_counts_are_the_host_rates(counts, probs, pos, neg, multiclass=True, pos_class=pc, neg_class=nc)
    assert counts.sum() > 0


@pytest.mark.gpu
def test_argmax_ties_go_to_the_lower_index_and_nan_rows_are_never_counted():
    torch = pytest.importorskip("torch")
    nan = np.nan
    p = np.asarray([[[0.5, 0.5, 0.25], [0.25, 0.5, 0.5], [0.5, 0.25, 0.5], [nan, 0.9, 0.1], [0.1, 0.9, nan], [0.75, 0.75, 0.75]]], np.float32)
    rows = [list(range(6))]
    for pc, want in ((0, 3), (1, 1), (2, 0)):                                  # argmax: 0, 1, 0, -, -, 0
        code, counts, _ = raw_call(torch, p, rows, rows, [0.0], 1, pc, pc)
        assert code == 0 and counts[0, 0].tolist() == [want, 4 - want], pc
    code, counts, _ = raw_call(torch, p, rows, rows, [0.0, 0.5, 0.75], 0, 0, 0)  # mode 0: a NaN score is above no threshold
    assert counts[0, :, 0].tolist() == [5, 1, 0]


# ------------------------------------------------------------------------------------------------ thresholds

@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 101, 1000, 1024, 4100])
def test_wrapper_threshold_counts(T):
    """4100 is past MKWS_ROC_MAX_THRESHOLDS: the wrapper runs the list in pieces."""
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd.roc import roc_counts_on_device
    probs, pos, neg = yardstick_case(3, 63)
    thresholds = [0.37] if T == 1 else THRESHS if T == 101 else np.linspace(0, 1, T)
    counts, _ = roc_counts_on_device(probs, pos, neg, thresholds)
    for k in range(3):
        assert np.array_equal(counts[k], counts_in_float64(probs[k][pos[k], 2], probs[k][neg[k], 2], thresholds)), k


@pytest.mark.gpu
def test_wrapper_takes_thresholds_in_any_order():
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd.roc import roc_counts_on_device
    probs, pos, neg = yardstick_case(3, 257)
    thresholds = [0.7, float(np.float32(0.1)), np.inf, 0.7, -np.inf, np.nan, 0.29, 0.0, -0.0, 0.29, np.nan]
    counts, totals = roc_counts_on_device(probs, pos, neg, thresholds)
    for k in range(3):
        assert np.array_equal(counts[k], counts_in_float64(probs[k][pos[k], 2], probs[k][neg[k], 2], thresholds)), k
        assert counts[k, 4].tolist() == totals[k].tolist() and not counts[k, [2, 5, 10]].any()
    out = tla.roc_many(probs, [pos[0], pos[0], pos[2]], [neg[1]] * 3, thresholds=thresholds)              # no empty side: rates divide
    assert out[1][0] == [int(c) / len(pos[0]) for c in counts_in_float64(probs[1][pos[0], 2], [], thresholds)[:, 0]]


@pytest.mark.gpu
def test_raw_call_takes_equal_neighbours():
    torch = pytest.importorskip("torch")
    probs, pos, neg = yardstick_case(3, 63)
    thresholds = [0.0, 0.25, 0.25, 0.25, 0.5, 0.5, 1.0]
    code, counts, invalid = raw_call(torch, probs, pos, neg, thresholds)
    assert code == 0 and not invalid.any()
    for k in range(3):
        assert np.array_equal(counts[k], counts_in_float64(probs[k][pos[k], 2], probs[k][neg[k], 2], thresholds)), k


# ------------------------------------------------------------------------------------------------ edges of the interface

@pytest.mark.gpu
def test_out_of_range_rows_are_skipped_and_reported():
    """By design, not a fault: the entry is never dereferenced."""
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd.roc import roc_counts_on_device
    probs, pos, neg = yardstick_case(3, 63)
    bad_pos = [list(pos[0]), [63, -1], list(pos[2])]
    bad_pos[0][5:5] = [63, 2 ** 31 - 1]
    bad_neg = [list(neg[0]), list(neg[1]), list(neg[2]) + [-2 ** 31]]
    bad_neg[1].append(-7)
    code, counts, invalid = raw_call(torch, probs, bad_pos, bad_neg, THRESHS)
    clean = raw_call(torch, probs, pos, neg, THRESHS)[1]
    assert code == 0 and invalid.tolist() == [2, 3, 1] and np.array_equal(counts, clean)
    with pytest.raises(ValueError, match="outside"):
        roc_counts_on_device(torch.from_numpy(probs).cuda(), bad_pos, neg, THRESHS)


@pytest.mark.gpu
def test_no_heads_no_rows_and_refused_arguments():
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.roc import MAX_THRESHOLDS, roc_counts_on_device
    probs = yardstick_case(3, 63)[0]
    code, counts, _ = raw_call(torch, probs[:0], [], [], [0.5])
    assert code == 0 and counts.shape == (0, 1, 2)
    code, counts, invalid = raw_call(torch, np.zeros((2, 0, 3), np.float32), [[], []], [[], []], [0.25, 0.5])
    assert code == 0 and not counts.any() and not invalid.any()                # written: the buffers started at -9
    code, counts, invalid = raw_call(torch, np.zeros((1, 0, 3), np.float32), [[0]], [[]], [0.5])
    assert code == 0 and not counts.any() and invalid.tolist() == [1]          # no rows at all: every entry is out of range
    counts, totals = roc_counts_on_device(np.zeros((0, 5, 3), np.float32), [], [], [0.5, 0.6])
    assert counts.shape == (0, 2, 2) and totals.shape == (0, 2)
    one = ([[0]], [[0]])
    assert raw_call(torch, probs[:1], *one, np.zeros(0))[0] == -1              # n_thr < 1
    assert raw_call(torch, probs[:1], *one, [0.5], 2)[0] == -1                 # mode
    assert raw_call(torch, probs[:1], *one, [0.5], 0, 3)[0] == -1              # pos_class
    assert raw_call(torch, probs[:1], *one, [0.5], 1, 2, -1)[0] == -1          # neg_class counts in mode 1 ...
    assert raw_call(torch, probs[:1], *one, [0.5], 0, 2, -1)[0] == 0           # ... and is ignored in mode 0
    assert raw_call(torch, probs[:1], *one, [0.5], n_rows=-1)[0] == -1
    assert raw_call(torch, probs[:1], *one, np.linspace(0, 1, MAX_THRESHOLDS))[0] == 0
    assert raw_call(torch, probs[:1], *one, np.linspace(0, 1, MAX_THRESHOLDS + 1))[0] == -2
    L, s = _lib.lib(), _lib.current_stream_ptr()
    d = torch.zeros(16, dtype=torch.int64, device="cuda")
    for hole in range(8):                                                      # probs, 2 x (rows, offsets), thresholds, counts, invalid
        a = [d.data_ptr()] * 8
        a[hole] = None
        assert L.mkws_roc_count(a[0], 1, 1, 3, a[1], a[2], a[3], a[4], a[5], 1, 0, 2, 1, a[6], a[7], s) == -1, hole
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end

@pytest.mark.gpu
def test_shared_embedding_pass_end_to_end(tmp_path):
    """Three synthetic heads, 40 one-second clips, overlapping per-keyword lists: evaluate_files_many has the bits of
    evaluate_files_single_target per model, classification_curves is roc_single_target on those predictions gathered by row."""
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd.embedding import input_data, transfer_learning as tl
    from multilingual_kws_amd.head import Head, glorot_uniform_params
    from util_data import tone_clip, write_wav
    rng = np.random.default_rng(3)
    files = []
    for i in range(40):
        files.append(str(tmp_path / "clips" / f"c{i}.wav"))
        write_wav(files[-1], tone_clip(250 + 95 * (i % 13), rng, burst=(1000 + 150 * i, 8000 + 150 * i)))
    settings = input_data.standard_microspeech_model_settings(3)
    emb, blob = tl.load_base_model("synthetic", max_batch=16)                   # 40 clips: batches of 16, 16 and 8
    models = [tl.TransferLearnedModel(emb, Head(emb.output_dim, 18, 3, max_batch=16, params=8 * glorot_uniform_params(emb.output_dim, 18, 3, s),
                                                device=emb.device), blob, "synthetic") for s in (1, 2, 3)]
    many = tl.evaluate_files_many(files, models, settings)
    assert many.shape == (3, 40, 3) and many.dtype == np.float32
    single = [tl.evaluate_files_single_target(files, 2, m, settings)[1] for m in models]
    for k in range(3):
        assert np.array_equal(many[k], single[k]), k
    on_device = tl.evaluate_files_many(files, models, settings, as_device=True)
    assert on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), many)
    # per-keyword lists: own targets (one clip twice), one shared pool plus the other keywords' targets
    targets = [files[0:6] + files[2:3], files[6:11], files[11:19]]
    pool = files[19:40]
    unknown = [pool + targets[1], pool + pool[:5] + targets[0], pool[::-1]]
    curves = tl.classification_curves(models, targets, unknown, settings)
    index = {f: i for i, f in enumerate(files)}
    for k, c in enumerate(curves):
        t_rows, u_rows = [index[f] for f in targets[k]], [index[f] for f in unknown[k]]
        tprs, fprs, threshs = tla.roc_single_target(single[k][t_rows, 2], single[k][u_rows, 2])
        assert c["tprs"] == tprs and c["fprs"] == fprs and np.array_equal(c["threshs"], threshs)
        assert (c["n_target"], c["n_unknown"]) == (len(t_rows), len(u_rows))
    with pytest.raises(ValueError, match="share one embedding"):
        other, _ = tl.load_base_model("synthetic", max_batch=16)
        tl.evaluate_files_many(files[:1], [models[0], tl.TransferLearnedModel(other, models[1].head, blob, "synthetic")], settings)


@pytest.mark.gpu
def test_captured_behind_the_heads_forward():
    """mkws_heads_forward -> mkws_roc_count recorded in a torch.cuda.graph and replayed twice on changed embeddings: the eager counts."""
    import ctypes
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.head import Head, glorot_uniform_params
    from multilingual_kws_amd.roc import pack_rows, roc_counts_on_device
    rng = np.random.default_rng(9)
    K, B, F = 4, 150, 1024
    heads = [Head(F, 18, 3, max_batch=B, params=4 * glorot_uniform_params(F, 18, 3, s)) for s in range(K)]
    pos = [[int(r) for r in rng.integers(0, B, n)] for n in (33, 70, 1, 129)]
    neg = [[int(r) for r in rng.integers(0, B, n)] for n in (200, 5, 64, 65)]
    (p_rows, p_off), (n_rows, n_off) = pack_rows(pos, K, B, "positives"), pack_rows(neg, K, B, "negatives")
    d_p, d_po, d_n, d_no = (torch.from_numpy(x).cuda() for x in (p_rows, p_off, n_rows, n_off))
    d_thr = torch.from_numpy(THRESHS).cuda()
    first, second = (rng.standard_normal((B, F)).astype(np.float32) for _ in range(2))
    d_emb = torch.from_numpy(first).cuda()
    d_probs = torch.zeros((K, B, 3), dtype=torch.float32, device="cuda")
    d_counts = torch.zeros((K, 101, 2), dtype=torch.int32, device="cuda")
    d_invalid = torch.zeros(K, dtype=torch.int32, device="cuda")
    table = (ctypes.c_void_p * K)(*[h.h.value for h in heads])
    L = _lib.lib()

    def chain():
        s = _lib.current_stream_ptr()
        assert L.mkws_heads_forward(table, K, d_emb.data_ptr(), B, d_probs.data_ptr(), s) == 0
        assert L.mkws_roc_count(d_probs.data_ptr(), K, B, 3, d_p.data_ptr(), d_po.data_ptr(), d_n.data_ptr(), d_no.data_ptr(), d_thr.data_ptr(), 101,
                                0, 2, 1, d_counts.data_ptr(), d_invalid.data_ptr(), s) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    seen = []
    for emb in (second, first):
        d_emb.copy_(torch.from_numpy(emb))
        d_counts.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        eager, _ = roc_counts_on_device(Head.forward_many(heads, torch.from_numpy(emb).cuda()), pos, neg, THRESHS)
        assert np.array_equal(d_counts.cpu().numpy(), eager) and not d_invalid.cpu().numpy().any()
        seen.append(eager)
    assert not np.array_equal(seen[0], seen[1]) and seen[0][:, 0].min() > 0
