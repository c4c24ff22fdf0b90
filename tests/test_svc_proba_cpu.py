"""The specification of SVC(probability=True) given the folds (multilingual_kws_amd/svc.py: cv_folds, cv_decision_host, platt_host,
couple_host, proba_host), the two transcriptions of libsvm's routines that tests/svc_proba_cases.py measures the reference's slack with,
the fixture tests/golden/svc_proba_golden.npz, the fold rule in distribution, and the "vote" classifier of the selection harness through
the host path.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import svc_proba_cases as cases  # noqa: E402
from test_selection_eval_cpu import N_TRAIN, N_UNKNOWN, WORDS, experiment, splits_for, stub_bank  # noqa: E402

from multilingual_kws_amd import svc  # noqa: E402
from multilingual_kws_amd.embedding import selection_eval as se  # noqa: E402


def clusters(seed, K=4, n=120, n_eval=60, dim=16, shift=1.8):
    """X = N(0, 1) + shift * onehot(y): -> (x float32 [n + n_eval, dim], y, training rows, evaluation rows)."""
    rng = np.random.RandomState(seed)
    y = np.arange(n + n_eval) % K
    x = (rng.randn(n + n_eval, dim) + shift * np.eye(K, dim)[y]).astype(np.float32)
    return x, y, np.arange(n), np.arange(n, n + n_eval)


# ------------------------------------------------------------------------------------------------ the yardstick

@pytest.mark.parametrize("K", [2, 4])
def test_the_transcriptions_reproduce_sklearn(K):
    """sigmoid_predict and multiclass_probability, given sklearn's own probA_, probB_ and decision values: predict_proba to 1e-10."""
    svm = pytest.importorskip("sklearn.svm")
    x, y, tr, ev = clusters(3, K)
    X = x.astype(np.float64)
    clf = svm.SVC(probability=True, random_state=0, decision_function_shape="ovo").fit(X[tr], y[tr])
    dec = clf.decision_function(X[ev])
    dec = -dec[:, None] if K == 2 else dec                               # libsvm's sign: class i of the pair positive
    got = cases.libsvm_proba(dec, clf.probA_, clf.probB_, np.arange(K), K)
    assert np.abs(got - clf.predict_proba(X[ev])).max() <= 1e-10
    # the exact solve differs from it by what the iteration's stopping rule (0.005 / K on the residual) leaves: the same argmax
    exact = svc.couple_host(dec, clf.probA_, clf.probB_, np.ones(K, bool))
    print(f"K {K}: the exact solve is {np.abs(exact - got).max():.2e} from libsvm's iteration")
    assert np.array_equal(exact.argmax(axis=1), got.argmax(axis=1))


def test_sigmoid_train_stops_where_libsvm_does():
    rng = np.random.default_rng(0)
    y = np.where(rng.random(200) < 0.4, 1.0, -1.0)
    dec = y * 0.8 + rng.normal(0, 1.0, 200)
    A, B = cases.sigmoid_train(dec, y)
    g = svc.platt_objective(dec, y, A, B)[1]
    assert np.abs(g).max() < 1e-5 and A < 0


# ------------------------------------------------------------------------------------------------ platt

@pytest.mark.parametrize("kind", ["overlap", "separable", "equal", "one_each", "large"])
def test_platt_host_against_scipy(kind):
    optimize = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(7)
    if kind == "equal":
        y, dec = np.asarray([1.0] * 9 + [-1.0] * 4), np.full(13, 0.75)
    elif kind == "one_each":
        y, dec = np.asarray([-1.0, 1.0]), np.asarray([-1.25, 2.0])
    else:
        y = np.where(rng.random(300) < 0.5, 1.0, -1.0)
        dec = y * {"overlap": 0.7, "separable": 6.0, "large": 25.0}[kind] + rng.normal(0, {"large": 12.0}.get(kind, 1.0), 300)
    A, B = svc.platt_host(dec, y)
    f, g, _ = svc.platt_objective(dec, y, A, B)
    assert np.abs(g).max() <= 1e-11
    fun = lambda v: svc.platt_objective(dec, y, v[0], v[1])[0]
    jac = lambda v: svc.platt_objective(dec, y, v[0], v[1])[1]
    res = optimize.minimize(fun, [0.0, 0.0], jac=jac, method="BFGS", options=dict(gtol=1e-9))
    # compared on A dec + B, which is unique also where (A, B) is not.  scipy stops at a gradient g_s: to first order it sits H^-1 g_s
    # from the minimiser, so the values differ by at most |g_s| |(dec, 1)| / lambda_min(H) (where all dec are equal the problem has one
    # unknown, the common value, with curvature H_BB); twice that is allowed for the higher orders
    _, g_s, H = svc.platt_objective(dec, y, res.x[0], res.x[1])
    if np.ptp(dec) == 0:
        bound = 2 * abs(g_s[1]) / H[1, 1] + 1e-12
    else:
        bound = 2 * np.linalg.norm(g_s) * np.sqrt((dec * dec).max() + 1.0) / np.linalg.eigvalsh(H)[0] + 1e-12
    err = np.abs((A * dec + B) - (res.x[0] * dec + res.x[1])).max()
    print(f"{kind}: max |z - z_scipy| {err:.3e}, bound {bound:.3e}, |g_scipy| {np.abs(g_s).max():.3e}")
    assert err <= bound and f <= res.fun + 1e-12 * max(1.0, abs(f))


# ------------------------------------------------------------------------------------------------ couple

def random_r(rng, k, extreme=False):
    r = np.zeros((k, k))
    for a in range(k):
        for b in range(a + 1, k):
            r[a, b] = rng.choice([svc.R_CLIP, 1 - svc.R_CLIP, rng.uniform(0.05, 0.95)]) if extreme else rng.uniform(0.02, 0.98)
            r[b, a] = 1.0 - r[a, b]
    return r


def decision_for(r, K):
    """decision values and sigmoids (A = -1, B = 0) whose pairwise probabilities are r."""
    dec = np.asarray([np.log(r[i, j] / r[j, i]) for i, j in svc.pairs(K)])
    return dec[None], -np.ones(len(dec)), np.zeros(len(dec))


@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_couple_host_solves_the_kkt_system(K):
    rng = np.random.default_rng(K)
    for trial in range(6):
        r = random_r(rng, K, extreme=trial >= 3)
        p = svc.couple_host(*decision_for(r, K), np.ones(K, bool))[0]
        Q = svc.couple_matrix(r)
        Qp = Q @ p
        assert abs(p.sum() - 1.0) <= 1e-12 and np.ptp(Qp) <= 1e-12 and p.min() >= -1e-12      # Q p = -b e on the plane sum p = 1
        if K == 2:
            assert np.abs(p - [r[0, 1], r[1, 0]]).max() <= 1e-12
        else:
            # the fixed-point iteration run to 1e-14 (or its bounded count): it solves the same linear system M [p; b] = [0; 1], so it
            # is at most |M^-1| |its residual| from the direct solve
            it, sweeps = svc.couple_iterative(r, eps=1e-14)
            M = np.block([[Q, np.ones((K, 1))], [np.ones((1, K)), np.zeros((1, 1))]])
            resid = np.concatenate([Q @ it - (it @ Q @ it), [it.sum() - 1.0]])
            bound = np.linalg.norm(np.linalg.inv(M), 2) * np.linalg.norm(resid) + 1e-12
            assert np.abs(it - p).max() <= bound, (trial, sweeps, np.abs(it - p).max(), bound)


def test_couple_host_absent_classes_and_nan():
    rng = np.random.default_rng(1)
    present = np.asarray([True, False, True, True, False])
    r = random_r(rng, 3)
    dec, A, B = np.zeros((2, 10)), np.zeros(10), np.zeros(10)
    cls = [0, 2, 3]
    for q, (i, j) in enumerate(svc.pairs(5)):
        if present[i] and present[j]:
            dec[:, q], A[q] = np.log(r[cls.index(i), cls.index(j)] / r[cls.index(j), cls.index(i)]), -1.0
    dec[1, 1] = np.nan
    out = svc.couple_host(dec, A, B, present)
    assert np.abs(out[0, cls] - svc.couple_host(*decision_for(r, 3), np.ones(3, bool))[0]).max() <= 1e-12 and not out[0, [1, 4]].any()
    assert np.isnan(out[1]).all()


# ------------------------------------------------------------------------------------------------ the folds and the cross-validated values

def test_cv_folds_are_balanced_and_deterministic():
    rng = np.random.default_rng(2)
    labels = rng.integers(0, 4, 300)
    offsets = [3, 120, 120, 290]
    for F in (2, 5, 16):
        folds = svc.cv_folds(labels, offsets, F, 1)
        assert folds.dtype == np.int32 and folds.min() == 0 and folds.max() == F - 1
        assert np.array_equal(folds, svc.cv_folds(labels, offsets, F, 1)) and not np.array_equal(folds, svc.cv_folds(labels, offsets, F, 2))
        for a, b in ((3, 120), (120, 290)):
            for k in range(4):
                counts = np.bincount(folds[a:b][labels[a:b] == k], minlength=F)
                assert counts.max() - counts.min() <= 1
    # a problem's folds depend on its index and its own list alone
    assert np.array_equal(svc.cv_folds(labels[:120], [3, 120], 5, 1)[3:], svc.cv_folds(labels, offsets, 5, 1)[3:120])
    # the key formula of the docstring, by hand, for one class of one problem
    from multilingual_kws_amd.synth import splitmix64
    with np.errstate(over="ignore"):
        base = splitmix64(np.asarray([1], np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        key = splitmix64(splitmix64(base + np.uint64(2)) + np.arange(170, dtype=np.uint64))
    t = np.nonzero(labels[120:290] == 3)[0]
    assert np.array_equal(svc.cv_folds(labels, offsets, 5, 1)[120 + t[np.argsort(key[t], kind="stable")]], np.arange(len(t)) % 5)
    with pytest.raises(ValueError):
        svc.cv_folds(labels, offsets, 17)


def test_cv_decision_host_against_tight_sklearn_sub_fits():
    """Per-fold SVC(tol=1e-9) fits with the whole problem's gamma: within 1.7e-6, libsvm's own distance from the float64 optimum
    (its kernel cache is float32)."""
    pytest.importorskip("sklearn.svm")
    for name in ("n12_k3_dim37_f3", "same_vector_both_labels", "degenerate_1_2_1_10"):
        c = cases.case(name)
        for rows, y, C, _, _, folds, _, _ in cases.problems(c):
            mine = svc.cv_decision_host(c["x"], rows, y, c["n_classes"], folds, c["n_folds"], C, c["standardize"])
            theirs = cases.sklearn_cv_decision(c["x"], rows, y, c["n_classes"], folds, c["n_folds"], C, c["standardize"], tol=1e-9)
            assert np.abs(mine - theirs).max() <= 1.7e-6, (name, np.abs(mine - theirs).max())


def test_the_three_rules_for_a_sub_fit_without_a_class():
    x, y, tr, _ = clusters(0, K=3, n=9, n_eval=0)
    y = np.asarray([0, 0, 1, 2, 2, 2, 2, 2, 2])
    folds = np.asarray([1, 2, 0, 0, 1, 1, 2, 2, 0])
    cv = svc.cv_decision_host(x, tr, y, 3, folds, 3)
    # pair (0, 1), fold 0 held out (entry 2, the whole of class 1): class 0 alone is left -> +1; folds 1 and 2 leave one of each: a machine
    assert cv[2, svc._slot(1, 0)] == 1.0 and abs(cv[0, svc._slot(0, 1)]) not in (0.0, 1.0)
    # pair (1, 2), fold 0 held out (entries 2, 3, 8): class 2 alone is left -> -1 for all three
    assert cv[2, svc._slot(1, 2)] == -1.0 and cv[3, svc._slot(2, 1)] == -1.0 and cv[8, svc._slot(2, 1)] == -1.0
    # a pair whose every entry sits in one fold: nothing is left -> 0
    cv = svc.cv_decision_host(x, tr[:3], y[:3], 3, [0, 0, 1], 2)
    assert cv[0, svc._slot(0, 1)] == -1.0 and cv[2, svc._slot(1, 0)] == 1.0          # pair (0, 1): each fold leaves the other class alone
    cv = svc.cv_decision_host(x, tr[:4], np.asarray([0, 1, 2, 2]), 3, [0, 0, 0, 1], 2)
    assert cv[0, 0] == 0.0 and cv[1, 0] == 0.0                                       # pair (0, 1): both in fold 0
    cv = svc.cv_decision_host(x, tr[:4], np.asarray([0, 0, 2, 2]), 3, [0, 1, 0, 1], 2)                      # class 1 absent: its slots are 0
    assert not cv[:2, svc._slot(0, 1)].any() and not cv[2:, svc._slot(2, 1)].any() and cv[:2, svc._slot(0, 2)].all() and cv[2:, svc._slot(2, 0)].all()
    with pytest.raises(ValueError):
        svc.cv_decision_host(x, tr, y, 3, folds, 2)


@pytest.mark.parametrize("name", cases.SMALL)
def test_the_fixture_equals_a_fresh_run(name, golden_dir):
    pytest.importorskip("sklearn.svm")
    stored = dict(np.load(os.path.join(golden_dir, "svc_proba_golden.npz")))
    assert {k.split("/")[0] for k in stored} == set(cases.CASES)
    fresh = cases.reference(name)
    for key, value in fresh.items():
        assert np.allclose(stored[f"{name}/{key}"], value, rtol=0, atol=1e-12), (name, key)
    assert fresh["clear"].min() >= 0.9
    if name == "degenerate_1_2_1_10":
        assert (fresh["rules"] > 0).all()


# ------------------------------------------------------------------------------------------------ the fold rule in distribution

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_fold_rule_is_within_sklearns_own_spread(seed):
    """D(P) = max |P - the mean of sklearn's eight seeds| (leave-one-out for sklearn's own runs): the median D of proba_host under fold
    seeds 0..7 is at most the largest D among sklearn's eight.  No margin: a failure is a finding about the fold rule."""
    svm = pytest.importorskip("sklearn.svm")
    x, y, tr, ev = clusters(seed)
    X = x.astype(np.float64)
    sk = np.stack([svm.SVC(probability=True, random_state=k).fit(X[tr], y[tr]).predict_proba(X[ev]) for k in range(8)])
    d_sk = [np.abs(sk[k] - np.delete(sk, k, axis=0).mean(axis=0)).max() for k in range(8)]
    mean = sk.mean(axis=0)
    d_ours = [np.abs(svc.proba_host(x, ev, tr, y[tr], 4, svc.cv_folds(y[tr], [0, len(tr)], 5, k), 5) - mean).max() for k in range(8)]
    print(f"generator seed {seed}: median D of the fold rule {np.median(d_ours):.3f}, sklearn's largest {max(d_sk):.3f}")
    assert np.median(d_ours) <= max(d_sk)


# ------------------------------------------------------------------------------------------------ the harness

def test_vote_contract_and_refusals():
    bank, word_rows, ut, ue = stub_bank(spread=2.5)
    exps = [experiment(word_rows, WORDS[:3]), experiment(word_rows, WORDS[4:7])]
    splits = [splits_for(e, 2, 10 + i) for i, e in enumerate(exps)]
    assert se.CLASSIFIERS["vote"] is False and "svm" not in se.CLASSIFIERS and "svc_probability" not in se.CLASSIFIERS
    out = se.experiment_run_many(bank, exps, ut, ue, splits, classifier="vote", on_device=False)
    assert [r["words"] for r in out] == [e["words"] for e in exps] and all(len(r["crossfold_scores"]) == 2 and 0.5 < r["score"] <= 1.0 for r in out)
    assert se.experiment_run_many(bank, exps, ut, ue, splits, classifier="vote", on_device=False) == out
    assert se.experiment_run_many(bank, exps[1:], ut, ue, splits[1:], classifier="vote", on_device=False, folds=None) != []
    K, fit_l, _, _, _ = se._lists(exps, ut, ue, splits)
    folds = svc.cv_folds(fit_l[1], fit_l[2], 5, 0)
    assert se.experiment_run_many(bank, exps, ut, ue, splits, classifier="vote", on_device=False, folds=folds) == out
    with pytest.raises(ValueError, match="folds"):
        se.experiment_run_many(bank, exps, ut, ue, splits, classifier="vote", on_device=False, folds=folds[:-1])
    for name in ("svm", "svc_probability", "random_forest"):
        with pytest.raises(ValueError, match="classifier.*probability"):
            se.experiment_run_many(bank, exps, ut, ue, splits, classifier=name)


def test_vote_best_split_is_the_first_argmax():
    bank, word_rows, ut, ue = stub_bank(spread=0.3)
    e = experiment(word_rows, WORDS[:3])
    sp = splits_for(e, 3, 5)
    (r,) = se.experiment_run_many(bank, [e], ut, ue, [sp], classifier="vote", on_device=False)
    assert r["crossfold_scores"] == [1.0, 1.0, 1.0] and r["best_split"] == 0 and r["score"] == 1.0
    first = (np.arange(N_TRAIN, 3 * N_TRAIN), np.arange(N_TRAIN))       # word 0 held out entirely: its class is never predicted by the SVC half
    (r2,) = se.experiment_run_many(bank, [e], ut, ue, [[first] + sp[1:]], classifier="vote", on_device=False)
    assert r2["crossfold_scores"][0] < 1.0 and r2["crossfold_scores"][1:] == [1.0, 1.0] and r2["best_split"] == 1 and r2["score"] == 1.0


def test_vote_is_the_reference_loop():
    """dataperf_test_harness.py:386-406 transcribed (the VotingClassifier of SVC(probability=True) and LogisticRegression, voting="soft",
    weights=None, per split; the best split by validation score on the dev rows) on the well-separated family: every route scores 1.0 on
    every fold, whatever folds libsvm draws, so scores and the chosen split compare with ==."""
    svm = pytest.importorskip("sklearn.svm")
    ensemble = pytest.importorskip("sklearn.ensemble")
    linear_model = pytest.importorskip("sklearn.linear_model")
    model_selection = pytest.importorskip("sklearn.model_selection")
    bank, word_rows, ut, ue = stub_bank(spread=0.3)
    e = WORDS[:5]
    training_samples = np.vstack([bank[word_rows[w][:N_TRAIN]] for w in e])
    training_labels = np.concatenate([[ix + 1] * N_TRAIN for ix, _ in enumerate(e)])
    eval_samples = np.vstack([bank[word_rows[w][N_TRAIN:]] for w in e] + [bank[ue]])
    eval_labels = np.concatenate([[ix + 1] * (len(word_rows[w]) - N_TRAIN) for ix, w in enumerate(e)] + [[0] * len(ue)])
    drawn = list(model_selection.StratifiedShuffleSplit(n_splits=4, train_size=40, random_state=0).split(training_samples, training_labels))
    clfs, crossfold_scores = [], []
    for train_ixs, val_ixs in drawn:
        train_Xs = np.vstack([training_samples[train_ixs], bank[ut]])
        train_ys = np.concatenate([training_labels[train_ixs], [0] * len(ut)])
        val_Xs = np.vstack([training_samples[val_ixs], bank[ue]])
        val_ys = np.concatenate([training_labels[val_ixs], [0] * len(ue)])
        clf = ensemble.VotingClassifier(estimators=[("svm", svm.SVC(probability=True)), ("lr", linear_model.LogisticRegression())], voting="soft", weights=None)
        clf.fit(train_Xs, train_ys)
        clfs.append(clf)
        crossfold_scores.append(clf.score(val_Xs, val_ys))
    best_clf = clfs[np.argmax(crossfold_scores)]
    score = best_clf.score(eval_samples, eval_labels)
    (r,) = se.experiment_run_many(bank, [experiment(word_rows, e)], ut, ue, [drawn], classifier="vote", on_device=False)
    assert crossfold_scores == [1.0] * 4 and score == 1.0
    assert r == dict(words=e, score=score, crossfold_scores=crossfold_scores, best_split=int(np.argmax(crossfold_scores)))
