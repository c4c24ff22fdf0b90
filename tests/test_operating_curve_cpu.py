"""batch_streaming_analysis.operating_curves on a host without a GPU (numpy input, CUDA reported unavailable): equal to an explicit
detect() + tpr_fpr composition, dict for dict with ==, on a stream and a ground truth built so that true positives, false positives,
false negatives, a threshold without a fire and the cap of the true-positive count all occur -- asserted on the host yardstick itself."""
import contextlib
import dataclasses
import io

import numpy as np
import pytest

from multilingual_kws_amd.embedding import batch_streaming_analysis as sa
from multilingual_kws_amd.embedding.tpr_fpr import tpr_fpr

THRESHOLDS = [0.1, 0.3, 0.5, 0.7, 0.9, 0.99]
W = 600


def _bursts(seed, centres, width=8, low=0.02, high=0.97):
    rng = np.random.default_rng(seed)
    tgt = np.full(W, low)
    for i, c in enumerate(centres):
        tgt[max(0, c - width):c + width] = high if i % 3 else 0.6        # every third burst reaches 0.6 only
    other = rng.uniform(0, 1, W) * (1 - tgt)
    return np.stack([1 - tgt - other, other, tgt], axis=1).astype(np.float32)


@pytest.fixture
def no_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def _compose(inferences, flags, thresholds, gt, keywords, duration_s, nontarget=None, **kw):
    """The parent's route, spelled out; the warning lines of tpr_fpr are collected, not printed."""
    out, said = [], io.StringIO()
    for n, word in enumerate(keywords):
        f = dataclasses.replace(flags, target_keyword=word)
        curve = []
        for thr in thresholds:
            found = sa.detect(inferences[n], f, thr, **kw)[0]
            with contextlib.redirect_stdout(said):
                curve.append(tpr_fpr(word, thr, found, gt[word], duration_s, flags.time_tolerance_ms, nontarget))
        out.append(curve)
    return out, said.getvalue().count("WARNING: weird timing issue")


def _recipe():
    centres = [30, 75, 120, 170, 215, 260, 310, 355, 400, 450, 500, 560]          # a dozen bursts
    inf = np.stack([_bursts(1, centres), _bursts(2, centres[::2])])
    keywords = ["alpha", "beta"]
    flags = sa.StreamFlags(wav="unused.wav", ground_truth="", target_keyword="mask", detection_thresholds=THRESHOLDS, time_tolerance_ms=750)
    tol = flags.time_tolerance_ms
    gt = {}
    for n, word in enumerate(keywords):
        fires = [t for _, t in sa.detect(inf[n], dataclasses.replace(flags, target_keyword=word), 0.5)[0]]
        assert len(fires) >= 5
        times = []
        for i, t in enumerate(fires):
            times.append(float(t + (tol, -tol, tol + 1)[i % 3]))            # on the upper edge, on the lower edge, one past the edge
        times.append(times[0] + 100.5)                                        # a second entry next to an occurrence
        times.append(float(W * 20 + 5000))                                    # a decoy nothing fires near
        times.append(times[1] - 0.5)                                          # out of order: behind the decoy, in some windows
        gt[word] = times
    return inf, keywords, flags, gt


def test_operating_curves_on_the_host_equal_detect_plus_tpr_fpr(no_gpu, capsys):
    inf, keywords, flags, gt = _recipe()
    duration_s = ((W - 1) * 320 + 16000) / 16000
    want, n_warn = _compose(inf, flags, THRESHOLDS, gt, keywords, duration_s)
    # the recipe does what it was written for, on the yardstick
    flat = [d for curve in want for d in curve]
    assert any(d["true_positives"] > 0 and d["false_positives"] > 0 and d["false_negatives"] > 0 for d in flat)
    assert any(d["true_positives"] == 0 and d["false_positives"] == 0 and d["false_negatives"] == d["groundtruth_positives"] for d in flat)   # no fire at all
    assert all(sorted(g) != g for g in gt.values())
    capsys.readouterr()
    got = sa.operating_curves(inf, flags, THRESHOLDS, gt, keywords=keywords)
    assert got == want
    for a, b in zip([d for c in got for d in c], flat):
        assert list(a) == list(b) and all(type(a[k]) is type(b[k]) for k in a)
    assert ("WARNING: weird timing issue" in capsys.readouterr().out) == (n_warn > 0)
    # rows (keyword, time) as read from the CSV, a list of arrays, one keyword as [W, 3], data_samples, duration and fpr
    rows = [(k, t) for k in keywords for t in gt[k]] + [("gamma", 1.0)]
    assert sa.operating_curves([inf[0], inf[1]], flags, THRESHOLDS, rows, keywords=keywords) == want
    one = sa.operating_curves(inf[1], dataclasses.replace(flags, target_keyword="beta"), THRESHOLDS, gt)
    assert one == want[1]
    data_samples = 16000 + 320 * 400
    cut, _ = _compose(inf, flags, THRESHOLDS, gt, keywords, data_samples / 16000, 40, data_samples=data_samples)
    assert sa.operating_curves(inf, flags, THRESHOLDS, gt, keywords=keywords, data_samples=data_samples, num_nontarget_words=40) == cut
    assert cut != want and all("fpr" in d for c in cut for d in c)
    fixed, _ = _compose(inf, flags, THRESHOLDS, gt, keywords, 12.5)
    assert sa.operating_curves(inf, flags, THRESHOLDS, gt, keywords=keywords, duration_s=12.5) == fixed
    assert sa.operating_curves(inf, flags, [], gt, keywords=keywords) == [[], []]


def test_the_cap_of_the_true_positive_count_is_hit_and_reported_once(no_gpu, capsys):
    inf, keywords, flags, _ = _recipe()
    flags = dataclasses.replace(flags, suppression_ms=100, time_tolerance_ms=1500)
    first = sa.detect(inf[0], dataclasses.replace(flags, target_keyword="alpha"), 0.5)[0][0][1]
    gt = {"alpha": [float(first)], "beta": [float(first)]}
    duration_s = ((W - 1) * 320 + 16000) / 16000
    want, n_warn = _compose(inf, flags, THRESHOLDS, gt, keywords, duration_s)
    assert n_warn >= 1
    # raw 2 > 1: two detections of a lane inside the one occurrence's window
    found = [t for _, t in sa.detect(inf[0], dataclasses.replace(flags, target_keyword="alpha"), 0.5)[0]]
    assert sum(abs(t - first) <= 1500 for t in found) >= 2 and want[0][THRESHOLDS.index(0.5)]["true_positives"] == 1
    capsys.readouterr()
    assert sa.operating_curves(inf, flags, THRESHOLDS, gt, keywords=keywords) == want
    out = capsys.readouterr().out
    assert out.count("WARNING: weird timing issue") == 1 and f"({n_warn} of {2 * len(THRESHOLDS)} " in out


def test_argument_errors(no_gpu):
    inf, keywords, flags, gt = _recipe()
    with pytest.raises(ValueError, match="keywords"):
        sa.operating_curves(inf, flags, THRESHOLDS, gt, keywords=["alpha"])
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            sa.operating_curves(inf, flags, THRESHOLDS, dict(gt, beta=[1000.0, bad]), keywords=keywords)
    with pytest.raises(ValueError, match="time_tolerance_ms"):
        sa.operating_curves(inf, dataclasses.replace(flags, time_tolerance_ms=-1), THRESHOLDS, gt, keywords=keywords)
    with pytest.raises(ZeroDivisionError):
        sa.operating_curves(inf, flags, THRESHOLDS, dict(alpha=gt["alpha"]), keywords=keywords)       # beta has no ground truth
    with pytest.raises(ValueError):
        sa.operating_curves(inf[0, 0], flags, THRESHOLDS, gt)


def test_score_wrapper_checks_its_arguments_before_touching_the_device():
    from multilingual_kws_amd import _lib, detector
    assert detector.SCORE_GT_TILE == 2048 and any(n == "mkws_detect_score" for n, _, _ in _lib.SYMBOLS)
    probs = np.zeros((2, 3, 3), np.float32)
    args = (100, 500, 4)
    with pytest.raises(ValueError, match="2\\*\\*53"):
        detector.score_on_device(probs, [0, 20, 2 ** 53 + 2], [0.5], [[], []], 750, *args)
    with pytest.raises(ValueError, match="finite"):
        detector.score_on_device(probs, [0, 20, 40], [0.5], [[1.0], [float("inf")]], 750, *args)
    with pytest.raises(ValueError, match="time_tolerance_ms"):
        detector.score_on_device(probs, [0, 20, 40], [0.5], [[], []], float("nan"), *args)
    with pytest.raises(ValueError, match="ground-truth lists"):
        detector.score_on_device(probs, [0, 20, 40], [0.5], [[]], 750, *args)
    values, offsets = detector.pack_groundtruth([[3.5, 1.0], [], [2.0]], 3)
    assert values.tolist() == [3.5, 1.0, 2.0] and offsets.tolist() == [0, 2, 2, 3] and offsets.dtype == np.int32
