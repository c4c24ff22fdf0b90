"""The point scorer without a GPU: scoring.score_host (the specification the kernel is held to) against sklearn and torch, against the
three scoring loops the package already has, the wrapper's refusals, the C entry's refusals (all decided on the host), the two small
pure functions that came with it, and the case table's claims about itself (tests/score_cases.py)."""
import ctypes
import hashlib
import math
import os

import numpy as np
import pytest
import torch

from multilingual_kws_amd import _lib, scoring
from tests import score_cases as sc

CPU, META = torch.device("cpu"), torch.device("meta")


def _probs(rng, n, c):
    z = rng.standard_normal((n, c)) * 3
    p = np.exp(z - z.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def test_score_host_against_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(0)
    p, y = _probs(rng, 400, 7), rng.integers(0, 7, 400)
    p[::9, 0] = 0.0                                                  # some probabilities at the clip
    got = scoring.score_host(p, y, mode=0)
    pred = p.argmax(1)
    assert np.array_equal(got.pred[0], pred)
    assert np.array_equal(got.confusion[0], metrics.confusion_matrix(y, pred, labels=list(range(7))))
    # log_loss on the clipped probabilities of the true class: one-hot rows make it the mean of -log(p[y])
    clipped = np.clip(p[np.arange(400), y].astype(np.float64), scoring.PROB_LO, scoring.PROB_HI)
    two = np.stack([1 - clipped, clipped], axis=1)
    want = metrics.log_loss(np.ones(400, int), two, labels=[0, 1], normalize=False)
    assert abs(got.loss_sum[0] - want) <= 1e-12 * want
    assert got.tally[0].tolist() == [400, int((pred == y).sum()), 0, 0]
    pr, rc, f1 = scoring.precision_recall_f1(got.confusion[0])
    wp, wr, wf, _ = metrics.precision_recall_fscore_support(y, pred, labels=list(range(7)), zero_division=0)
    assert np.allclose(pr, wp, rtol=1e-15, atol=0) and np.allclose(rc, wr, rtol=1e-15, atol=0) and np.allclose(f1, wf, rtol=1e-14, atol=0)
    # a class never predicted and a class never present: zero_division=0
    cm = np.asarray([[3, 0, 0], [1, 0, 0], [0, 0, 0]])
    pr, rc, f1 = scoring.precision_recall_f1(cm)
    wp, wr, wf, _ = metrics.precision_recall_fscore_support([0, 0, 0, 1], [0, 0, 0, 0], labels=[0, 1, 2], zero_division=0)
    assert pr.tolist() == wp.tolist() and rc.tolist() == wr.tolist() and np.allclose(f1, wf, rtol=1e-15)


def test_score_host_against_torch_cross_entropy():
    rng = np.random.default_rng(1)
    for c in (3, 33, 761):
        z, y = (rng.standard_normal((50, c)) * 6).astype(np.float32), rng.integers(0, c, 50)
        got = scoring.score_host(z, y, mode=1)
        want = torch.nn.functional.cross_entropy(torch.from_numpy(z).double(), torch.from_numpy(y), reduction="none").numpy()
        assert np.abs(got.row_loss[0] - want).max() <= 64 * sc.EPS * (1 + np.abs(z).max())
        assert abs(got.loss_sum[0] - want.sum()) <= 1e-13 * want.sum()


def test_score_host_against_the_three_existing_loops():
    """Where the package's three scoring loops agree with the specification and where they do not: they differ only in how they clip."""
    rng = np.random.default_rng(2)
    p, y = _probs(rng, 64, 3), rng.integers(0, 3, 64)
    p[0, y[0]], p[1, y[1]], p[2, y[2]] = 1.0, 0.0, 3e-8
    rows = np.arange(64)
    spec = scoring.score_host(p, y, mode=0).row_loss[0]
    tp, ty = torch.from_numpy(p), torch.from_numpy(y)
    # transfer_learning._validate: float32, clamped from below only
    validate = -torch.log(torch.clamp(tp[torch.arange(64), ty], min=1e-7))
    assert validate[0] == 0.0 and spec[0] == -math.log(1 - 2.0 ** -23) > 1e-7          # p[y] = 1: the one-sided clamp reports 0
    assert np.abs(validate.numpy()[1:] - spec[1:]).max() <= 2e-6                          # float32 everywhere else, the low clip included
    # dscnn_comparison: float64, clipped to [1e-7, 1 - 1e-7] with float64 constants
    picked = tp.double().gather(1, ty.view(-1, 1)).clamp(1e-7, 1 - 1e-7)
    dscnn_loop = -picked.log().view(-1).numpy()
    inside = (p[rows, y] > 1.1e-7) & (p[rows, y] < 1 - 2e-7)
    assert np.abs(dscnn_loop[inside] - spec[inside]).max() <= 4 * sc.EPS * spec[inside].max()
    assert abs(dscnn_loop[1] - spec[1]) < 2e-8 and dscnn_loop[1] != spec[1]               # float64 1e-7 against the widened float32 1e-7
    assert abs(dscnn_loop[0] - 1e-7) < 1e-13 and abs(spec[0] - 2.0 ** -23) < 1e-13        # 1 - 1e-7 against the float32 1 - 2^-23
    # train_multilingual_embedding: float32 cross_entropy on logits
    z = (rng.standard_normal((64, 761)) * 4).astype(np.float32)
    zy = rng.integers(0, 761, 64)
    ce = torch.nn.functional.cross_entropy(torch.from_numpy(z), torch.from_numpy(zy), reduction="none").numpy()
    got = scoring.score_host(z, zy, mode=1)
    assert np.abs(ce - got.row_loss[0]).max() <= 2e-5 * np.abs(got.row_loss[0]).max()
    assert np.array_equal(got.pred[0], torch.from_numpy(z).argmax(1).numpy())


def test_score_host_label_rules_and_groups():
    p = np.asarray([[0.2, 0.8], [0.6, 0.4], [0.5, 0.5], [0.1, 0.9], [0.3, 0.7]], np.float32)
    got = scoring.score_host(p, [1, 1, -1, 2, 0], groups=[0, 1, 5, 0, 2], mode=0, n_groups=2)
    assert got.pred[0].tolist() == [1, 0, 0, 1, 1] and got.kind[0].tolist() == [0, 0, 1, 2, 2]
    assert got.tally[0].tolist() == [2, 1, 1, 2] and got.confusion[0].tolist() == [[0, 0], [1, 1]]
    assert got.group_tally[0].tolist() == [[1, 1], [1, 0]] and np.isnan(got.row_loss[0][2:]).all()
    assert got.loss_sum[0] == math.fsum([-math.log(float(np.float32(0.8))), -math.log(float(np.float32(0.4)))])
    nan_row = scoring.score_host(np.asarray([[1.0, np.nan, np.nan]], np.float32), [0], mode=1)
    assert nan_row.pred[0].tolist() == [1] and np.isnan(nan_row.loss_sum[0])
    res = scoring.summarise(got.loss_sum, got.tally, got.confusion, got.group_tally)
    assert res.accuracy.tolist() == [0.5] and res.rows.tolist() == [2] and res.ignored.tolist() == [1] and res.group_accuracy.tolist() == [[1.0, 0.0]]


def _ok(dev=CPU, K=3, N=5, C=4):
    return dict(scores=torch.zeros((K, N, C), device=dev), labels=torch.zeros(N, dtype=torch.int32, device=dev), groups=torch.zeros(N, dtype=torch.int64, device=dev))


def test_check_add_accepts_and_normalises():
    a = _ok()
    assert scoring.check_add(CPU, 3, 4, 2, **a) == (5, 0)
    assert scoring.check_add(CPU, 3, 4, 0, a["scores"], torch.zeros((3, 5), dtype=torch.int64)) == (5, 1)
    assert scoring.check_add(CPU, 1, 4, 0, torch.zeros((5, 4)), torch.zeros(5, dtype=torch.uint8)) == (5, 0)
    assert scoring.check_add(CPU, 1, 4, 0, torch.zeros((1, 0, 4)), torch.zeros(0, dtype=torch.int32)) == (0, 0)
    strided = torch.zeros((3, 5, 8))[:, :, ::2]
    assert not strided.is_contiguous() and scoring.check_add(CPU, 3, 4, 0, strided, a["labels"]) == (5, 0)
    assert scoring.check_add(META, 3, 4, 2, **_ok(META)) == (5, 0)


@pytest.mark.parametrize("dev,bad_dev", [(CPU, META), (META, CPU)])
def test_check_add_refusals(dev, bad_dev):
    a = _ok(dev)
    cases = [
        ("scores", dict(scores=a["scores"].double())), ("scores", dict(scores=a["scores"].half())), ("scores", dict(scores=a["scores"].int())),
        ("scores", dict(scores=torch.zeros((3, 5, 4), device=bad_dev))), ("scores", dict(scores=a["scores"][0])), ("scores", dict(scores=a["scores"][None])),
        ("scores", dict(scores=torch.zeros((3, 5, 5), device=dev))), ("scores", dict(scores=torch.zeros((2, 5, 4), device=dev))), ("scores", dict(scores=[[0.0] * 4] * 5)),
        ("labels", dict(labels=a["labels"].float())), ("labels", dict(labels=a["labels"].bool())), ("labels", dict(labels=torch.zeros(5, dtype=torch.int32, device=bad_dev))),
        ("labels", dict(labels=a["labels"][:4])), ("labels", dict(labels=torch.zeros((2, 5), dtype=torch.int32, device=dev))),
        ("labels", dict(labels=torch.zeros((3, 5, 1), dtype=torch.int32, device=dev))), ("labels", dict(labels=[0] * 5)),
        ("groups", dict(groups=None)), ("groups", dict(groups=a["groups"].float())), ("groups", dict(groups=torch.zeros(5, dtype=torch.int32, device=bad_dev))),
        ("groups", dict(groups=a["groups"][:4])), ("groups", dict(groups=torch.zeros((3, 5), dtype=torch.int32, device=dev))),
    ]
    for name, change in cases:
        with pytest.raises(ValueError, match=rf"\b{name}\b"):
            scoring.check_add(dev, 3, 4, 2, **dict(a, **change))
    with pytest.raises(ValueError, match=r"\bgroups\b"):
        scoring.check_add(dev, 3, 4, 0, **a)                          # groups for a scorer without groups
    with pytest.raises(ValueError, match=r"\bdevice\b"):
        scoring.Scorer(1, 3, 0, device="cpu")
    for bad in (dict(n_models=0), dict(classes=1), dict(classes=4097), dict(mode=2), dict(n_groups=-1)):
        with pytest.raises(ValueError):
            scoring.Scorer(**dict(dict(n_models=1, classes=3, mode=0, device="cuda:0"), **bad))


def test_c_entry_refusals_are_decided_on_the_host():
    L = _lib.lib()
    one = ctypes.c_void_p(8)                                         # a non-NULL pointer nothing reads: every call below returns before a launch
    ok = dict(d_scores=one, n_models=1, n_rows=4, classes=3, mode=0, d_labels=one, labels_per_model=0, d_groups=None, n_groups=0, d_loss=one,
              d_tally=one, d_confusion=None, d_group_tally=None, d_row_loss=None, d_pred=None, d_work=one, stream=None)

    def call(**change):
        return L.mkws_score_accumulate(*dict(ok, **change).values())

    for change in (dict(n_models=-1), dict(n_rows=-1), dict(classes=1), dict(classes=0), dict(mode=2), dict(mode=-1), dict(n_groups=-1),
                   dict(d_groups=one, n_groups=0), dict(labels_per_model=2), dict(d_scores=None), dict(d_labels=None), dict(d_loss=None),
                   dict(d_tally=None), dict(d_work=None)):
        assert call(**change) == -1, change                          # MKWS_ERR_INVALID_ARG
        assert L.mkws_last_error()
    assert call(classes=4097) == -2 and call(classes=4097, n_rows=0) == -2     # MKWS_ERR_UNSUPPORTED
    assert call(n_models=0) == 0 and call(n_rows=0) == 0 and call(n_rows=0, d_scores=None, d_loss=None) == 0
    assert L.mkws_score_work_bytes(3, 513) == 3 * 513 * 8 and L.mkws_score_work_bytes(0, 5) == 0 and L.mkws_score_work_bytes(2, -1) == 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mkws.h")).read()
    assert "#define MKWS_SCORE_MAX_CLASSES 4096" in header and scoring.MAX_CLASSES == 4096
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert len(bound["mkws_score_accumulate"]) == 17 and len(bound["mkws_score_work_bytes"]) == 2


def test_which_set_known_answers():
    from multilingual_kws_amd.gsc_comparisons import which_set

    def by_hand(name, val, test):
        pct = (int(hashlib.sha1(name.encode()).hexdigest(), 16) % 2 ** 27) * (100.0 / (2 ** 27 - 1))
        return "validation" if pct < val else "testing" if pct < val + test else "training"

    names = ["bed/0a7c2a8d_nohash_0.wav", "/data/left/0a7c2a8d_nohash_3.wav", "c50f55b8_nohash_1.wav", "right/ffd2ba2f_nohash_0.wav", "3cfc6b3a.wav",
             "yes/b5cf6ea8_nohash_12.wav", "common_voice_en_123.wav"]
    speakers = ["0a7c2a8d", "0a7c2a8d", "c50f55b8", "ffd2ba2f", "3cfc6b3a.wav", "b5cf6ea8", "common_voice_en_123.wav"]
    got = [which_set(n, 10, 10) for n in names]
    assert got == [by_hand(s, 10, 10) for s in speakers]
    assert got[0] == got[1]                                          # one speaker, one set, whatever the word and the take
    assert [which_set(n, 0, 0) for n in names] == ["training"] * 7 and [which_set(n, 100.1, 0) for n in names] == ["validation"] * 7
    assert [which_set(n, 0, 100.1) for n in names] == ["testing"] * 7
    many = [which_set(f"{i:08x}_nohash_0.wav", 10, 10) for i in range(2000)]
    assert 120 < many.count("validation") < 280 and 120 < many.count("testing") < 280


def test_keyword_labels():
    from multilingual_kws_amd.embedding.transfer_learning import keyword_labels
    got = keyword_labels([0, -1, 2, 5, 1, 2], 3)
    assert got.dtype == np.int32 and got.tolist() == [[2, 0, 1, 1, 1, 1], [1, 0, 1, 1, 2, 1], [1, 0, 2, 1, 1, 2]]
    assert keyword_labels([], 2).shape == (2, 0) and keyword_labels(np.asarray([1], np.int8), 1).tolist() == [[1]]
    for bad in ([[0, 1]], [0.5], [-2]):
        with pytest.raises(ValueError):
            keyword_labels(bad, 2)
    with pytest.raises(ValueError):
        keyword_labels([0], 0)


def test_dscnn_l2_helper_names_the_trainers_kernels():
    from multilingual_kws_amd import dscnn, dscnn_trainer
    assert dscnn.conv_kernel_names() == dscnn_trainer.CONV_KERNELS and dscnn.WEIGHT_DECAY == 1e-4
    ws = [torch.full((3, 3), 2.0), torch.full((2,), 0.5, dtype=torch.float32)]
    assert dscnn.l2_penalty(ws, 0.25) == 0.25 * (9 * 4.0 + 2 * 0.25)
    params = dscnn.synthetic_params(5)
    host = dscnn.unpack(params)
    want = 1e-4 * sum(float(np.square(host[k].astype(np.float64)).sum()) for k in dscnn.conv_kernel_names())
    got = dscnn.l2_penalty([torch.from_numpy(np.ascontiguousarray(host[k])) for k in dscnn.conv_kernel_names()], 1e-4)
    assert abs(got - want) <= 1e-12 * want


# ---- the case table's own claims ----------------------------------------------------------------------------------------------------------

def test_the_grid_covers_what_it_says():
    cases = sc.grid_cases()
    assert len(cases) == len(sc.CLASSES) * len(sc.ROWS) * 2 and len({c["name"] for c in sc.all_cases()}) == len(sc.all_cases())
    assert scoring.SMALL_CLASSES in sc.CLASSES and scoring.SMALL_CLASSES + 1 in sc.CLASSES and {64, 65, 761, 2, 3, 7} <= set(sc.CLASSES)
    assert {0, 1, 63, 64, 65, 257} <= set(sc.ROWS) and max(sc.ROWS) > 2 * sc.SMALL_TILE > 2 * sc.LARGE_TILE and 65 > 2 * sc.LARGE_TILE
    for key, values in (("classes", sc.CLASSES), ("rows", sc.ROWS)):
        for v in values:
            mine = [c for c in cases if c[key] == v]
            assert {c["mode"] for c in mine} == {0, 1} and {c["models"] for c in mine} == set(sc.MODELS), (key, v)
            assert {c["per_model"] for c in mine} == {0, 1} and {c["n_groups"] for c in mine} == set(sc.GROUPS), (key, v)
    ties = ignored = 0
    for case in cases:
        scores, labels, groups, _ = sc.build(case)
        assert scores.dtype == np.float32 and scores.shape == (case["models"], case["rows"], case["classes"])
        assert labels.shape == ((case["models"], case["rows"]) if case["per_model"] else (case["rows"],)) and (groups is None) == (case["n_groups"] == 0)
        if case["rows"]:
            ties += int(((scores == scores.max(axis=2, keepdims=True)).sum(axis=2) > 1).sum())
            ignored += int((labels == -1).sum())
            assert labels.max() < case["classes"] and labels.min() >= -1
    assert ties > 500 and ignored > 500


@pytest.mark.parametrize("case", sc.named_cases(), ids=lambda c: c["name"])
def test_named_rows_are_what_they_claim(case):
    scores, labels, groups, named = sc.build(case)
    C, mode = case["classes"], case["mode"]
    want = sc.host(case, scores, labels, groups)
    names = [n for n, *_ in named]
    assert len(set(names)) == len(names)
    for must in ("two-way tie", "three-way tie", "last lane's stride", "one NaN", "two NaNs", "label -1", "label = classes", "group = n_groups"):
        assert any(must in n for n in names), must
    for must in (("+inf", "magnitude 80", "magnitude 100") if mode else ("p[y] = 0", "p[y] = 1", "below 1e-7")):
        assert any(must in n for n in names), must
    for r, (name, row, label, group, claims) in enumerate(named):
        bits = scores[0, r].view(np.uint32)
        assert np.array_equal(bits, row.view(np.uint32)) and labels[0, r] == np.int32(label) and groups[r] == group, name
        for k in range(3):
            assert want.pred[k, r] == claims["pred"] and want.kind[k, r] == claims["kind"], (name, k)
        if "tie" in claims:
            idx = list(claims["tie"])
            vals = row[idx]
            assert len(idx) >= 2 and claims["pred"] == min(idx), name
            assert np.all(vals == vals[0]) and vals.dtype == np.float32, name        # a float32 tie (== : -0.0 and +0.0 are one)
            with np.errstate(invalid="ignore"):
                assert not np.any(row[~np.isnan(row)] > vals[0]), name
        loss = claims.get("loss")
        if claims["kind"] != 0:
            assert np.isnan(want.row_loss[0, r]), name
        elif loss == "nan":
            assert np.isnan(want.row_loss[0, r]), name
        elif loss == "finite":
            assert np.isfinite(want.row_loss[0, r]), name
        elif loss is not None:
            assert want.row_loss[0, r] == loss or abs(want.row_loss[0, r] - loss) <= 1e-6 * abs(loss), (name, want.row_loss[0, r], loss)
        if claims.get("clipped") == "lo":
            assert float(row[label]) < scoring.PROB_LO, name
        if claims.get("clipped") == "at lo":
            assert float(row[label]) == scoring.PROB_LO and row[label] == np.float32(1e-7), name
        if claims.get("clipped") == "hi":
            assert float(row[label]) > scoring.PROB_HI == 1 - 2.0 ** -23, name
        if claims.get("f32_overflow"):
            with np.errstate(over="ignore"):
                assert np.isinf(np.exp(row).sum(dtype=np.float32)), name             # the naive float32 logsumexp overflows here
    if mode == 1:
        r = names.index("logits of magnitude 80, label the minimum")
        assert np.abs(scores[0, r]).max() == 80.0 and want.row_loss[0, r] == pytest.approx(160.0, abs=1e-9)
        with np.errstate(over="ignore", divide="ignore"):
            naive32 = np.log(np.exp(scores[0, r]).sum(dtype=np.float32)) - scores[0, r, C - 1]
            naive64 = np.log(np.exp(scores[0, r].astype(np.float64) * 10).sum())       # and in double at ten times the magnitude
        assert abs(float(naive32) - 160.0) < 1e-3 and np.isinf(naive64)
    if C > 64:
        r = names.index("two NaNs: the first wins")
        a, b = np.nonzero(np.isnan(scores[0, r]))[0]
        assert a < b and a % 64 > b % 64                               # the later NaN sits in a lower lane
        r = names.index("the maximum in the last lane's stride")
        assert want.pred[0, r] % 64 == 63 and want.pred[0, r] + 64 >= C


def test_bound_constants_follow_from_the_table():
    """The measured route: four times the kernel-order twin's largest distance from exact arithmetic, per mode and for the sum; the
    constants in score_cases.py are those figures rounded up (and at least one unit for the single log of mode 0)."""
    worst_row, worst_sum = sc.measure_bounds()
    print("twin against exact, largest distance in units: rows", worst_row, "sum", worst_sum)
    assert 4 * worst_row[1] <= sc.ROW_BOUND_UNITS[1] <= 8 * worst_row[1]
    assert 4 * worst_sum <= sc.SUM_BOUND_UNITS <= 8 * worst_sum
    assert sc.ROW_BOUND_UNITS[0] == max(1.0, math.ceil(40 * worst_row[0]) / 10)
    assert sc.n_adds(32) == 31 and sc.n_adds(33) == 6 and sc.n_adds(761) == 17
    # the twin is the specification up to rounding: the same integers by construction, losses within the bound it defines
    for case in sc.all_cases()[::7]:
        scores, labels, groups, _ = sc.build(case)
        want = sc.host(case, scores, labels, groups)
        twin = scoring.score_kernel_order(scores, labels, groups, case["mode"], case["n_groups"])
        row, total = sc.loss_bounds(case, scores, want)
        finite = np.isfinite(want.row_loss)
        assert np.array_equal(np.isnan(twin.row_loss), np.isnan(want.row_loss))
        assert np.all(np.abs(twin.row_loss[finite] - want.row_loss[finite]) <= row[finite] / 4), case["name"]
        for k in range(scores.shape[0]):
            if np.isfinite(want.loss_sum[k]):
                assert abs(twin.loss_sum[k] - want.loss_sum[k]) <= total[k] / 4, case["name"]
