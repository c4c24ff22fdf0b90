"""The selection harness with the SVC classifiers ("svc", "svc_scaled") through the host path (no GPU): contract, the first-argmax tie
rule, and one experiment against a literal transcription of the reference's loop with sklearn.svm.SVC() and the StandardScaler
pipeline.  The stub vectors are those of tests/test_selection_eval_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_selection_eval_cpu import N_DEV, N_TRAIN, N_UNKNOWN, WORDS, experiment, splits_for, stub_bank  # noqa: E402

from multilingual_kws_amd.embedding import selection_eval as se  # noqa: E402


def test_contract_and_determinism():
    bank, word_rows, ut, ue = stub_bank(spread=2.5)
    exps = [experiment(word_rows, WORDS[:3]), experiment(word_rows, WORDS[4:7]), experiment(word_rows, [WORDS[6], WORDS[0], WORDS[3]])]
    splits = [splits_for(e, 3, 10 + i) for i, e in enumerate(exps)]
    assert se.CLASSIFIERS["svc"] is False and se.CLASSIFIERS["svc_scaled"] is True and "svm" not in se.CLASSIFIERS
    out = se.experiment_run_many(bank, exps, ut, ue, splits, classifier="svc", on_device=False)
    assert len(out) == 3
    for e, sp, r in zip(exps, splits, out):
        assert set(r) == {"words", "score", "crossfold_scores", "best_split"} and r["words"] == e["words"]
        assert len(r["crossfold_scores"]) == 3 and r["best_split"] == int(np.argmax(r["crossfold_scores"]))
        n_val = len(sp[0][1]) + N_UNKNOWN
        assert all(0.0 <= s <= 1.0 and abs(s * n_val - round(s * n_val)) < 1e-9 for s in r["crossfold_scores"])
        assert 0.5 < r["score"] <= 1.0 and abs(r["score"] * (3 * N_DEV + N_UNKNOWN) - round(r["score"] * (3 * N_DEV + N_UNKNOWN))) < 1e-9
    assert any(s < 1.0 for r in out for s in r["crossfold_scores"])                 # (this family is hard enough to tell splits apart)
    assert se.experiment_run_many(bank, exps, ut, ue, splits, classifier="svc", on_device=False) == out
    # an experiment's answer does not depend on its neighbours; the scaled classifier and the logistic regression are different ones
    assert se.experiment_run_many(bank, exps[1:2], ut, ue, splits[1:2], classifier="svc", on_device=False) == out[1:2]
    scaled = se.experiment_run_many(bank, exps, ut, ue, splits, classifier="svc_scaled", on_device=False)
    assert [r["words"] for r in scaled] == [r["words"] for r in out]
    assert se.experiment_run_many(bank, [], ut, ue, [], classifier="svc") == []
    with pytest.raises(ValueError, match="probability"):
        se.experiment_run_many(bank, exps, ut, ue, splits, classifier="svc_probability")


@pytest.mark.parametrize("classifier", ["svc", "svc_scaled"])
def test_best_split_is_the_first_argmax(classifier):
    """Well separated: every split scores 1.0 and the tie goes to split 0, as np.argmax does in the reference; with the first split
    spoiled (a word held out of its training rows: a class with no row is never predicted) the best is the next one."""
    bank, word_rows, ut, ue = stub_bank(spread=0.3)
    e = experiment(word_rows, WORDS[:3])
    sp = splits_for(e, 3, 5)
    (r,) = se.experiment_run_many(bank, [e], ut, ue, [sp], classifier=classifier, on_device=False)
    assert r["crossfold_scores"] == [1.0, 1.0, 1.0] and r["best_split"] == 0 and r["score"] == 1.0
    first = (np.arange(N_TRAIN, 3 * N_TRAIN), np.arange(N_TRAIN))       # word 0 held out entirely
    (r2,) = se.experiment_run_many(bank, [e], ut, ue, [[first] + sp[1:]], classifier=classifier, on_device=False)
    assert r2["crossfold_scores"] == [N_UNKNOWN / (N_TRAIN + N_UNKNOWN), 1.0, 1.0] and r2["best_split"] == 1 and r2["score"] == 1.0


@pytest.mark.parametrize("classifier", ["svc", "svc_scaled"])
def test_one_experiment_is_the_reference_loop(classifier):
    """dataperf_test_harness.py:318-408 transcribed with its `simplest_svm` / `svm_with_scaling` classifier functions (:224-239) on a
    well-separated family, splits drawn by sklearn's StratifiedShuffleSplit as there: every route scores 1.0 on every fold, so scores and
    the chosen split compare with ==."""
    svm = pytest.importorskip("sklearn.svm")
    model_selection = pytest.importorskip("sklearn.model_selection")
    pipeline = pytest.importorskip("sklearn.pipeline")
    preprocessing = pytest.importorskip("sklearn.preprocessing")

    def classifier_fn(train_Xs, train_ys):
        if classifier == "svc":
            clf = svm.SVC()
        else:
            clf = pipeline.make_pipeline(preprocessing.StandardScaler(), svm.SVC())
        clf.fit(train_Xs, train_ys)
        return clf

    bank, word_rows, ut, ue = stub_bank(spread=0.3)
    e = WORDS[:5]
    unknown_fvs = dict(train=bank[ut], eval=bank[ue])
    # ---- the reference's loop
    word2classid = {word: ix + 1 for ix, word in enumerate(e)}
    word2splits_fvs = {word: dict(train=bank[word_rows[word][:N_TRAIN]], dev=bank[word_rows[word][N_TRAIN:]]) for word in e}
    training_samples, training_labels, eval_samples, eval_labels = [], [], [], []
    for word, splits2fvs in word2splits_fvs.items():
        training_samples.append(splits2fvs["train"])
        training_labels.extend([word2classid[word] for _ in range(splits2fvs["train"].shape[0])])
        eval_samples.append(splits2fvs["dev"])
        eval_labels.extend([word2classid[word] for _ in range(splits2fvs["dev"].shape[0])])
    training_samples, eval_samples = np.vstack(training_samples), np.vstack(eval_samples)
    training_labels, eval_labels = np.array(training_labels), np.array(eval_labels)
    eval_samples = np.vstack([eval_samples, unknown_fvs["eval"]])
    eval_labels = np.concatenate([eval_labels, [0] * unknown_fvs["eval"].shape[0]])
    selector = model_selection.StratifiedShuffleSplit(n_splits=4, train_size=40, random_state=0)
    drawn = list(selector.split(training_samples, training_labels))
    classifiers, crossfold_scores = [], []
    for train_ixs, val_ixs in drawn:
        train_Xs = np.vstack([training_samples[train_ixs], unknown_fvs["train"]])
        train_ys = np.concatenate([training_labels[train_ixs], [0] * unknown_fvs["train"].shape[0]])
        val_Xs = np.vstack([training_samples[val_ixs], unknown_fvs["eval"]])
        val_ys = np.concatenate([training_labels[val_ixs], [0] * unknown_fvs["eval"].shape[0]])
        clf = classifier_fn(train_Xs, train_ys)
        classifiers.append(clf)
        crossfold_scores.append(clf.score(val_Xs, val_ys))
    best_clf = classifiers[np.argmax(crossfold_scores)]
    experiment_results = dict(words=e, score=best_clf.score(eval_samples, eval_labels))
    # ---- this module
    (r,) = se.experiment_run_many(bank, [experiment(word_rows, e)], ut, ue, [drawn], classifier=classifier, on_device=False)
    assert crossfold_scores == [1.0] * 4 and experiment_results["score"] == 1.0
    assert r == dict(words=e, score=experiment_results["score"], crossfold_scores=crossfold_scores, best_split=int(np.argmax(crossfold_scores)))
