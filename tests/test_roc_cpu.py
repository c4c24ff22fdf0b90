"""The host specification of the classification ROC (embedding/transfer_learning_analysis.py) against vectors of the reference's own
functions (tests/golden/roc_golden.json, written by make_roc_golden.py), roc_many on numpy input, and the argument checks that come
before any device call.  Every comparison is exact: the rates are quotients of the same integers.  No GPU is needed (on a host with
one, roc_many counts numpy input on the device and must return the same lists)."""
import json
import os
import types

import numpy as np
import pytest

from multilingual_kws_amd.embedding import transfer_learning as tl
from multilingual_kws_amd.embedding import transfer_learning_analysis as tla

THRESHS = np.arange(0, 1.01, 0.01)


@pytest.fixture(scope="module")
def golden(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "roc_golden.json")))["cases"]
    assert len(cases) == 12 and {c["function"] for c in cases} == {"roc_single_target", "roc_sc", "calc_roc"}
    return cases


def _table(case):
    return np.asarray(case["probs"], dtype=np.float32)


def _negatives(case):
    return sum((case["groups"][k] for k in ("oov", "unknown_training", "original_embedding")), []) if "groups" in case else case["negatives"]


def test_host_functions_reproduce_the_reference_vectors(golden):
    for c in golden:
        p = _table(c)
        if c["function"] == "roc_single_target":
            tprs, fprs, threshs = tla.roc_single_target(p[c["positives"], c["target_id"]], p[c["negatives"], c["target_id"]])
        elif c["function"] == "roc_sc":
            tprs, fprs, threshs = tla.roc_sc(tla.split_confidences(p[c["positives"]], c["target_id"]),
                                             tla.split_confidences(p[c["negatives"]], c["negative_class"]))
        else:
            res = {"target_keywords": tla.split_confidences(p[c["positives"]], c["target_id"])}
            res.update({k: tla.split_confidences(p[v], c["negative_class"]) for k, v in c["groups"].items()})
            (tprs, fprs), threshs = tla.calc_roc(res), THRESHS
        assert tprs == c["tprs"] and fprs == c["fprs"], c["function"]
        assert all(type(x) is float for x in tprs + fprs) and len(tprs) == len(fprs) == 101
        assert isinstance(threshs, np.ndarray) and threshs.dtype == np.float64 and np.array_equal(threshs, THRESHS)


def test_golden_vectors_tell_the_float32_comparison_apart(golden):
    """The vectors are worth having only if comparing in float32 would not reproduce them."""
    differ = 0
    for c in golden:
        if c["function"] == "roc_single_target":
            s = _table(c)[c["positives"], c["target_id"]]
            differ += [int(np.count_nonzero(s > np.float32(t))) / len(s) for t in THRESHS] != c["tprs"]
    assert differ >= 2


def test_host_functions_take_lists_and_float64(golden):
    """np.array(list) in the reference: plain lists of Python floats are compared as they are."""
    tprs, fprs, _ = tla.roc_sc(dict(correct=[0.5, 0.75, 1.0], incorrect=[0.2]), dict(correct=[0.9] * 3, incorrect=[0.5]))
    assert tprs[0] == 0.75 and tprs[50] == 0.5 and tprs[75] == 0.25 and tprs[100] == 0.0
    assert fprs[49] == 0.25 and fprs[50] == 0.0


def test_roc_many_equals_the_host_functions(golden):
    for c in golden:
        p = _table(c)
        many = c["function"] != "roc_single_target"
        out = tla.roc_many(p[None], [c["positives"]], [_negatives(c)], multiclass=many, target_id=c["target_id"],
                           negative_class=c.get("negative_class", 0))
        assert len(out) == 1
        tprs, fprs, threshs = out[0]
        assert tprs == c["tprs"] and fprs == c["fprs"] and np.array_equal(threshs, THRESHS)
        assert all(type(x) is float for x in tprs + fprs)


def test_roc_many_several_heads_and_own_thresholds():
    """Three heads with different planes and lists; thresholds unsorted, with a duplicate, both infinities and a NaN."""
    rng = np.random.default_rng(5)
    K, N = 3, 37
    thr32 = THRESHS[rng.integers(0, 101, (K, N, 3))].astype(np.float32)
    probs = np.where(rng.integers(0, 2, thr32.shape) > 0, np.nextafter(thr32, np.float32(2)), thr32).astype(np.float32)
    pos = [[int(r) for r in rng.integers(0, N, n)] for n in (5, 60, 1)]
    neg = [[int(r) for r in rng.integers(0, N, n)] for n in (44, 3, 9)]
    thresholds = [0.7, 0.1, np.inf, 0.7, -np.inf, np.nan, 0.30000000000000004]
    for multiclass in (False, True):
        out = tla.roc_many(probs, pos, neg, thresholds=thresholds, multiclass=multiclass)
        for k in range(K):
            tprs, fprs, threshs = out[k]
            assert np.array_equal(threshs, np.asarray(thresholds), equal_nan=True)
            for j, t in enumerate(thresholds):
                if multiclass:
                    a, b = tla.split_confidences(probs[k][pos[k]], 2)["correct"], tla.split_confidences(probs[k][neg[k]], 1)["incorrect"]
                else:
                    a, b = probs[k][pos[k], 2], probs[k][neg[k], 2]
                want = (sum(float(x) > t for x in a) / len(pos[k]), sum(float(x) > t for x in b) / len(neg[k]))
                assert (tprs[j], fprs[j]) == want, (multiclass, k, j)
            assert tprs[2] == fprs[2] == tprs[5] == fprs[5] == 0.0 and tprs[0] == tprs[3]


def _args(**over):
    kw = dict(probs=np.full((2, 4, 3), 0.5, np.float32), positives=[[0, 1], [2]], negatives=[[3], [0, 0]])
    kw.update(over)
    return kw


@pytest.mark.parametrize("over", [
    dict(positives=[[0, 1]]),                              # one list for two heads
    dict(negatives=[[3], [0], [1]]),
    dict(positives=[[0, 4], [2]]),                         # row 4 of 4
    dict(negatives=[[3], [-1]]),
    dict(positives=[[0.5], [2]]),
    dict(probs=np.zeros((4, 3), np.float32)),
    dict(probs=np.zeros((2, 4, 3), np.float64)),
    dict(target_id=3),
    dict(multiclass=True, negative_class=-1),
    dict(thresholds=[]),
], ids=["pos_short", "neg_long", "row_high", "row_negative", "row_float", "probs_2d", "probs_f64", "target_id", "negative_class", "no_threshold"])
def test_roc_many_refuses(over):
    with pytest.raises(ValueError):
        tla.roc_many(**_args(**over))


def test_wrapper_refuses_rows_before_any_upload():
    from multilingual_kws_amd.roc import pack_rows, roc_counts_on_device
    with pytest.raises(ValueError, match="outside"):
        roc_counts_on_device(np.zeros((1, 4, 3), np.float32), [[4]], [[0]], [0.5])          # raised before torch.cuda is touched
    rows, offsets = pack_rows([[1, 1, 0], [], [3]], 3, 4, "positives")
    assert rows.dtype == offsets.dtype == np.int32 and rows.tolist() == [1, 1, 0, 3] and offsets.tolist() == [0, 3, 3, 4]


def test_empty_side_divides_by_zero():
    with pytest.raises(ZeroDivisionError):
        tla.roc_single_target(np.zeros(0, np.float32), np.ones(3, np.float32))
    with pytest.raises(ZeroDivisionError):
        tla.roc_sc(dict(correct=[0.5], incorrect=[]), dict(correct=[], incorrect=[]))
    with pytest.raises(ZeroDivisionError):
        tla.calc_roc({k: dict(correct=[], incorrect=[]) for k in ("target_keywords", "oov", "unknown_training", "original_embedding")})
    with pytest.raises(ZeroDivisionError):
        tla.roc_many(**_args(negatives=[[3], []]))


def test_models_must_share_one_embedding_handle():
    head = types.SimpleNamespace(in_dim=1024, hidden=18, classes=3)
    a, b = types.SimpleNamespace(embedding=object(), head=head), types.SimpleNamespace(embedding=object(), head=head)
    settings = tl.input_data.standard_microspeech_model_settings(3)
    with pytest.raises(ValueError, match="share one embedding"):
        tl.evaluate_files_many(["x.wav"], [a, b], settings)
    with pytest.raises(ValueError, match="share one embedding"):
        tl.classification_curves([a, b], [["x.wav"], ["y.wav"]], [["z.wav"], ["z.wav"]])
    with pytest.raises(ValueError, match="at least one model"):
        tl.evaluate_files_many(["x.wav"], [], settings)
    with pytest.raises(ValueError, match="lists of target files"):
        tl.classification_curves([a, a], [["x.wav"]], [["z.wav"], ["z.wav"]])


def test_reference_import_path_is_the_same_module():
    import multilingual_kws.embedding.transfer_learning_analysis as under_reference_path
    from multilingual_kws import embedding
    assert under_reference_path is tla and embedding.transfer_learning_analysis is tla
