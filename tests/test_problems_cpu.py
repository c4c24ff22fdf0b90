"""The layer under kmeans.py, logreg.py, svc.py and embedding/selection_eval.py (multilingual_kws_amd/problems.py, _lib.word_layout) without
a GPU: the two check_problems are one, check_groups and check_lists refuse the same offsets, the scaler statistics are one, the output
layouts are the ones the fits used to spell out, and experiment_run_many is one flow that does not know which classifier it carries."""
import numpy as np
import pytest

from multilingual_kws_amd import _lib, kmeans, logreg, problems, svc
from multilingual_kws_amd.embedding import selection_eval as se

ROWS, LABELS = np.arange(40) % 40, np.arange(40) % 3
# (rows, labels, offsets, n_rows, dim, n_classes, C): the refusal cases of tests/test_logreg_cpu.py and tests/test_svc_cpu.py, and what passes there
PROBLEM_TABLE = (
    [(ROWS, LABELS, offsets, 40, 8, 3, 1.0) for offsets in ([0, 20, 10, 40], [-1, 40], [0, 41], [[0, 40]], [0.0, 40.0], [], [0, 40], [5, 3], [0])] +
    [(ROWS, LABELS, [0, 40], 40, 8, K, 1.0) for K in (1, 0, 9, 2, 8)] +
    [(ROWS, LABELS, [0, 40], 40, dim, 3, 1.0) for dim in (0, 1, 1024, 1025)] +
    [(ROWS, LABELS, [0, 40], 40, 8, 3, C) for C in (0.0, -1.0, np.inf, np.nan, 2.0, [1.0, 1.0], [3.0])] +
    [(np.zeros(1025, np.int64), np.zeros(1025, np.int64), [0, 1025], 40, 8, 3, 1.0), (np.zeros(1024, np.int32), np.zeros(1024, np.int32), [0, 1024], 40, 8, 3, 1.0),
     (ROWS, LABELS[:39], [0, 40], 40, 8, 3, 1.0), (ROWS.astype(np.float64), LABELS, [0, 40], 40, 8, 3, 1.0), (ROWS, LABELS.astype(np.float32), [0, 40], 40, 8, 3, 1.0),
     (ROWS.reshape(4, 10), LABELS.reshape(4, 10), [0, 40], 40, 8, 3, 1.0), (ROWS, LABELS, [0, 20, 40], 40, 8, 3, [1.0, 2.0, 3.0]),
     (ROWS, LABELS, [3, 20, 20, 37], 40, 8, 3, [1, 2, 3]), ([2 ** 40, -2 ** 40], [0, 1], [0, 2], 40, 8, 3, 1.0), ([], [], [0, 0], 40, 8, 3, 1.0),
     (ROWS, LABELS, [0, 40], -1, 8, 3, 1.0)])


def _outcome(check, args):
    try:
        return check(*args[:6], C=args[6])
    except ValueError as e:
        return str(e)


def test_the_two_check_problems_are_one():
    refused = 0
    for args in PROBLEM_TABLE:
        a, b = _outcome(logreg.check_problems, args), _outcome(svc.check_problems, args)
        assert type(a) is type(b), args
        if isinstance(a, str):
            assert a == b and a
            refused += 1
        else:
            assert len(a) == len(b) == 4
            for u, v, dtype in zip(a, b, (np.int32, np.int32, np.int32, np.float64)):
                assert u.dtype == v.dtype == dtype and np.array_equal(u, v)
    assert refused == 7 + 3 + 2 + 5 + 7 and len(PROBLEM_TABLE) == 9 + 5 + 4 + 7 + 11     # (per line of the table: bad offsets, K, dim, C, the rest)
    r, y, off, Cs = logreg.check_problems([2 ** 40, -2 ** 40], [0, 1], [0, 2], 40, 8, 3)        # out of int32 stays out of every bank
    assert r.tolist() == [2 ** 31 - 1, -2 ** 31] and y.tolist() == [0, 1] and off.tolist() == [0, 2] and Cs.tolist() == [1.0]
    assert (logreg.MAX_ROWS, logreg.MAX_CLASSES, logreg.MAX_DIM) == (svc.MAX_ROWS, svc.MAX_CLASSES, svc.MAX_DIM) == (1024, 8, 1024)


def test_check_groups_and_check_lists_refuse_the_same_offsets():
    for offsets in ([0, 20, 10, 40], [-1, 40], [0, 41], [0.0, 40.0], [[0, 40]]):        # decreasing, negative, beyond the total, float, 2-D
        with pytest.raises(ValueError, match="offsets"):
            kmeans.check_groups(offsets, 40, 8, 2)
        with pytest.raises(ValueError, match="offsets"):
            problems.check_lists(ROWS, LABELS, offsets, 1024)
        with pytest.raises(ValueError, match="offsets"):
            problems.check_offsets(offsets, 40, "group")
    assert kmeans.check_groups([0, 20, 40], 40, 8, 2).tolist() == problems.check_lists(ROWS, LABELS, [0, 20, 40], 1024)[2].tolist() == [0, 20, 40]
    with pytest.raises(ValueError, match="group 1 has 1 points for 2 clusters"):         # check_groups keeps its own refusals and its word
        kmeans.check_groups([0, 20, 21, 40], 40, 8, 2)
    with pytest.raises(ValueError, match="problem 1 has 21 rows: at most 20"):
        problems.check_lists(ROWS, LABELS, [0, 19, 40], 20)


def test_standard_scaler_is_the_one_of_both_modules():
    X = np.random.default_rng(3).normal(size=(7, 5)) * [1.0, 10.0, 0.1, 1.0, 3.0] + [0.0, 5.0, -2.0, 0.0, 100.0]
    X[:, 3] = 3.0                                                                        # a constant column: sigma 0 -> 1
    mu, sigma = problems.standard_scaler(X)
    assert mu.dtype == sigma.dtype == np.float64 and sigma[3] == 1.0 and mu[3] == 3.0
    live = np.arange(5) != 3
    assert (np.abs(mu - X.mean(0)) <= 1e-15 * np.abs(X.mean(0))).all()
    assert (np.abs(sigma[live] - X.std(0)[live]) <= 1e-15 * X.std(0)[live]).all() and X.std(0)[3] == 0.0
    mu_lr, sigma_lr = logreg._scaler(X, True)
    centre, inv, _ = svc.scaling(X, np.arange(7), standardize=True)
    assert mu_lr.tobytes() == mu.tobytes() == centre.tobytes() and sigma_lr.tobytes() == sigma.tobytes() and inv.tobytes() == (1.0 / sigma).tobytes()
    assert [a.tolist() for a in logreg._scaler(X, False)] == [[0.0] * 5, [1.0] * 5]
    centre, inv, _ = svc.scaling(X, np.arange(7))                                        # svc always centres
    assert centre.tobytes() == mu.tobytes() and inv.tolist() == [1.0] * 5


def test_output_layouts_are_the_ones_the_fits_spelled_out():
    f32, f64, i32 = np.float32, np.float64, np.int32
    P, K, dim = 3, 4, 5
    assert _lib.word_layout([("stats", f64, (P, 2)), ("coef", f32, (P, K, dim)), ("intercept", f32, (P, K)), ("info", i32, (P, 4))]) == \
        np.cumsum([0, 4 * P, P * K * dim, P * K, 4 * P]).tolist()
    P, K, dim, n_list = 2, 3, 4, 11
    npairs = K * (K - 1) // 2
    assert _lib.word_layout([("coef", f32, (n_list, K - 1)), ("rho", f32, (P, npairs)), ("gamma", f32, (P,)), ("centre", f32, (P, dim)),
                             ("inv_scale", f32, (P, dim)), ("info", i32, (P, 4)), ("gap", f32, (P,))]) == \
        np.cumsum([0, n_list * (K - 1), P * npairs, P, P * dim, P * dim, 4 * P, P]).tolist()
    G, k, rows = 2, 3, 7                                                                  # kmeans, with and without its float64 centres
    tail = [("centers", f32, (G, k, dim)), ("labels", i32, (rows,)), ("init", i32, (G, k)), ("info", i32, (G, 4))]
    assert _lib.word_layout([("centers_f64", f64, (G, k, dim))] + tail) == np.cumsum([0, 2 * G * k * dim, G * k * dim, rows, G * k, G * 4]).tolist()
    assert _lib.word_layout(tail) == np.cumsum([0, G * k * dim, rows, G * k, G * 4]).tolist()
    assert _lib.word_layout([]) == [0] and _lib.word_layout([("empty", f64, (0, 2)), ("one", i32, ())]) == [0, 0, 1]
    with pytest.raises(ValueError, match="8-byte"):
        _lib.word_layout([("odd", i32, (3,)), ("stats", f64, (1, 2))])
    assert _lib.word_layout([("even", i32, (4,)), ("stats", f64, (1, 2))]) == [0, 4, 8]
    with pytest.raises(TypeError):
        _lib.word_layout([("short", np.int16, (4,))])


# ---- experiment_run_many against a classifier it has never seen: nearest class mean, in NumPy
N_WORDS, N_PER_WORD, N_TRAIN, DIM = 3, 6, 4, 8


def class_means(bank, rows, labels, K):
    """[K, dim]: the mean vector of every class, +inf for a class without a row (never the nearest)."""
    return np.stack([bank[rows[labels == c]].astype(np.float64).mean(axis=0) if (labels == c).any() else np.full(bank.shape[1], np.inf) for c in range(K)])


def n_correct(bank, means, rows, true):
    d = ((bank[rows].astype(np.float64)[:, None, :] - means[None]) ** 2).sum(axis=2)
    return int((d.argmin(axis=1) == true).sum())


def _stub_fit(bank, fit_lists, K, C, standardize, max_iter, gtol, tol):
    assert isinstance(bank, np.ndarray) and max_iter == 7                                # the host route, and the description's own default
    return [class_means(bank, rows, labels, K) for rows, labels in se._each(fit_lists)]


def _stub_count_correct(bank, models, which, fit_lists, eval_lists, K):
    models = models if which is None else [models[c] for c in which]
    return [n_correct(bank, m, rows, true) for m, (rows, true) in zip(models, se._each(eval_lists))]


def _stub_refused(models):
    bad = [p for p, m in enumerate(models) if np.isinf(m[1:]).all()]                     # (no word has a row)
    return bad[0] if bad else None


def by_plain_loop(bank, experiments, splits):
    """What the reference's loop gives for the stub classifier, with no unknown rows: -> [(crossfold scores, best split, dev score)]."""
    out = []
    for e, sp in zip(experiments, splits):
        K = len(e["words"]) + 1
        rows = np.concatenate(e["train_rows"])
        labels = np.concatenate([np.full(len(r), ix + 1) for ix, r in enumerate(e["train_rows"])])
        dev_rows = np.concatenate(e["dev_rows"])
        dev_true = np.concatenate([np.full(len(r), ix + 1) for ix, r in enumerate(e["dev_rows"])])
        models, scores = [], []
        for train_ixs, val_ixs in sp:
            models.append(class_means(bank, rows[train_ixs], labels[train_ixs], K))
            scores.append(n_correct(bank, models[-1], rows[val_ixs], labels[val_ixs]) / len(val_ixs))
        best = 0
        for s in range(1, len(sp)):
            if scores[s] > scores[best]:
                best = s
        out.append((scores, best, n_correct(bank, models[best], dev_rows, dev_true) / len(dev_rows)))
    return out


def test_experiment_run_many_is_one_flow_for_any_classifier(monkeypatch):
    monkeypatch.setitem(se.CLASSIFIERS, "stub", False)
    monkeypatch.setitem(se.IMPLEMENTATIONS, "stub", se.Classifier(_stub_fit, _stub_refused, _stub_count_correct, "no word has a row", 7))
    rng = np.random.default_rng(11)
    word_of_row = np.repeat(np.arange(N_WORDS), N_PER_WORD)
    word_rows = [np.nonzero(word_of_row == w)[0] for w in range(N_WORDS)]
    centres = rng.normal(size=(N_WORDS, DIM))
    exps = [dict(words=[f"w{w}" for w in order], train_rows=[word_rows[w][:N_TRAIN] for w in order], dev_rows=[word_rows[w][N_TRAIN:] for w in order])
            for order in ([0, 1, 2], [2, 0, 1])]
    stacked = np.arange(N_WORDS * N_TRAIN).reshape(N_WORDS, N_TRAIN)                      # positions in an experiment's stacked train rows
    splits = [[(np.delete(stacked, s + shift, axis=1).reshape(-1), stacked[:, s + shift]) for s in range(3)] for shift in (0, 1)]
    for spread, some_wrong in ((0.05, False), (1.2, True)):
        bank = (centres[word_of_row] + spread * rng.normal(size=(N_WORDS * N_PER_WORD, DIM))).astype(np.float32)
        out = se.experiment_run_many(bank, exps, [], [], splits, classifier="stub", on_device=False)
        want = by_plain_loop(bank, exps, splits)
        assert [(r["crossfold_scores"], r["best_split"], r["score"]) for r in out] == want and [r["words"] for r in out] == [e["words"] for e in exps]
        assert some_wrong == any(s < 1.0 for scores, _, _ in want for s in scores)
    # `bank` is now the noisy one; on the clean one every split scores 1.0 and the tie goes to split 0 ...
    bank = (centres[word_of_row] + 0.05 * rng.normal(size=(N_WORDS * N_PER_WORD, DIM))).astype(np.float32)
    out = se.experiment_run_many(bank, exps, [], [], splits, classifier="stub", on_device=False)
    assert [(r["crossfold_scores"], r["best_split"], r["score"]) for r in out] == [([1.0, 1.0, 1.0], 0, 1.0)] * 2
    # ... and with the first split's training rows emptied of experiment 0's first word the best moves to the next split
    spoiled = [[(splits[0][0][0][N_TRAIN - 1:], splits[0][0][1])] + splits[0][1:], splits[1]]
    out = se.experiment_run_many(bank, exps, [], [], spoiled, classifier="stub", on_device=False)
    want = by_plain_loop(bank, exps, spoiled)
    assert [(r["crossfold_scores"], r["best_split"], r["score"]) for r in out] == want
    assert want[0][0][0] == 2 / 3 and want[0][1] == 1 and want[1][1] == 0
    # what the description refuses, the flow reports with the description's text
    nothing = [[(np.zeros(0, np.int64), stacked[:, 0])] * 3, splits[1]]
    with pytest.raises(ValueError, match="problem 0 was refused by the device: no word has a row"):
        se.experiment_run_many(bank, exps, [], [], nothing, classifier="stub", on_device=False)
    assert sorted(se.IMPLEMENTATIONS) == sorted(se.CLASSIFIERS)
