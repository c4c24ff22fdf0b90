"""The L1 logistic-regression specification and the host side of the device solver (multilingual_kws_amd/lr_l1.py) without a GPU:
lr_l1_host against sklearn's liblinear run at tol=1e-10, the golden fixture, the mirror, the closed forms, the refusals, the C symbols,
and the "lr_l1" / "lr_l2" classifiers of the selection harness through the host path."""
import ctypes
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from lr_l1_cases import CASES, case, dense_star, problems, x_hash  # noqa: E402
from test_selection_eval_cpu import N_DEV, N_UNKNOWN, WORDS, experiment, splits_for, stub_bank  # noqa: E402

from multilingual_kws_amd import _lib, logreg, lr_l1  # noqa: E402
from multilingual_kws_amd.embedding import selection_eval as se  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRESH = [n for n in CASES if not n.startswith("caps")]      # lr_l1_host runs on these here (their first three problems); the caps case
_HOST = {}                                                   # takes 40 s on the host and is held to the fixture instead


def host(name):
    """lr_l1_host on the first three problems of a case; computed once and left unchanged."""
    if name not in _HOST:
        c = case(name)
        _HOST[name] = [lr_l1.lr_l1_host(c["x"], rows, y, c["n_classes"], C) for rows, y, C, _, _ in problems(c)[:3]]
    return _HOST[name]


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "lr_l1_golden.npz"))


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_is_the_optimum(name, golden_dir):
    """Every case, the caps case included: the stored weights reproduce the stored f_star under objective() with a violation of at most
    1e-8, sklearn's tight run (stored) has the same objective within 1e-8 f, and sklearn's default run is not below the optimum."""
    g, c = golden(golden_dir), case(name)
    assert str(g[name + "/x_sha1"]) == x_hash(c)
    K, dim = c["n_classes"], c["x"].shape[1]
    P = len(c["offsets"]) - 1
    coef, intercept = dense_star(g, name, P, K, dim)
    assert g[name + "/f_star"].shape == (P, K) and g[name + "/z_star"].shape == (len(c["eval_rows"]), K)
    for p, (rows, y, C, ev_rows, _) in enumerate(problems(c)):
        f, v = lr_l1.objective(c["x"], rows, y, K, C, coef[p], intercept[p])
        assert np.all(np.abs(f - g[name + "/f_star"][p]) <= 1e-12 * f) and np.all(v <= 1e-8), (name, p, f, v)
        assert np.all(np.abs(g[name + "/f_sklearn_tight"][p] - f) <= 1e-8 * f)
        assert np.all(g[name + "/f_sklearn"][p] >= f - 1e-9 * f)
        lo, hi = c["eval_offsets"][p], c["eval_offsets"][p + 1]
        assert np.abs(g[name + "/z_star"][lo:hi] - (c["x"][ev_rows].astype(np.float64) @ coef[p].T + intercept[p])).max() <= 1e-12
    if name in FRESH:
        for p, h in enumerate(host(name)):
            assert np.all(np.abs(h.f - g[name + "/f_star"][p]) <= 1e-12 * h.f)
            assert np.array_equal(h.coef != 0, coef[p] != 0) and np.array_equal(h.intercept != 0, intercept[p] != 0)


@pytest.mark.parametrize("name", FRESH)
def test_host_reaches_sklearns_tight_optimum(name):
    """f within 1e-8 f of liblinear's at tol=1e-10 per class, the same non-zero pattern, and objective() at sklearn's point reproduces the
    value computed directly from the formula."""
    linear_model = pytest.importorskip("sklearn.linear_model")
    c = case(name)
    K = c["n_classes"]
    for (rows, y, C, _, _), h in zip(problems(c), host(name)):
        X = c["x"][rows].astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            clf = linear_model.LogisticRegression(penalty="l1", solver="liblinear", C=C, tol=1e-10, max_iter=200000, random_state=0).fit(X, y)
        assert h.coef.shape == (K, X.shape[1]) and h.intercept.shape == h.f.shape == h.violation.shape == h.n_iter.shape == (K,)
        assert (h.violation <= 1e-8).all()
        models = [(1, clf.coef_[0], clf.intercept_[0])] if K == 2 else [(k, clf.coef_[i], clf.intercept_[i]) for i, k in enumerate(clf.classes_)]
        for k, w, b in models:
            s = np.where(np.asarray(y) == k, 1.0, -1.0)
            direct = np.abs(w).sum() + abs(b) + C * np.logaddexp(0.0, -s * (X @ w + b)).sum()
            W, B = h.coef.copy(), h.intercept.copy()
            W[k], B[k] = w, b
            f_at, _ = lr_l1.objective(c["x"], rows, y, K, C, W, B)
            assert f_at[k] == pytest.approx(direct, rel=1e-13)
            assert abs(h.f[k] - direct) <= 1e-8 * direct, (name, k, h.f[k], direct)
            assert np.array_equal(h.coef[k] != 0, w != 0) and (h.intercept[k] != 0) == (b != 0), (name, k)


def test_two_classes_are_exact_negations():
    c = case("n10_k2_dim1024")
    (h,) = host("n10_k2_dim1024")
    assert np.array_equal(h.coef[0], -h.coef[1]) and h.intercept[0] == -h.intercept[1] and h.f[0] == h.f[1]
    assert not np.signbit(h.coef).all() and (h.coef[1] != 0).sum() >= 1
    rows, y, C, _, _ = problems(c)[0]
    f, v = lr_l1.objective(c["x"], rows, y, 2, C, h.coef, h.intercept)
    assert f[0] == pytest.approx(f[1], rel=1e-14) and (v <= 1e-8).all()            # the mirror is the optimum of the class-0 problem


def test_absent_class_takes_its_closed_form():
    c = case("absent_class")
    rows, y, C, _, _ = problems(c)[0]
    (h,) = host("absent_class")
    assert 2 not in set(np.asarray(y).tolist()) and C * len(rows) > 1
    assert not h.coef[2].any() and abs(h.intercept[2] + np.log(C * len(rows) - 1)) <= 1e-7 and h.violation[2] <= 1e-8
    # every sample in the class: the mirror image (a two-class problem whose labels are all 1)
    one = lr_l1.lr_l1_host(c["x"], rows, np.ones(len(rows), np.int64), 3, C)
    assert not one.coef.any() and abs(one.intercept[1] - np.log(C * len(rows) - 1)) <= 1e-7 and abs(one.intercept[0] + np.log(C * len(rows) - 1)) <= 1e-7


def test_small_c_gives_exact_zeros():
    c = case("c_0p01_1_100")
    rows, y, C, _, _ = problems(c)[0]
    h = host("c_0p01_1_100")[0]
    assert C == 0.01 and not h.coef.any() and not h.intercept.any()
    assert np.allclose(h.f, C * len(rows) * np.log(2.0), rtol=1e-14, atol=0)


def test_host_raises_above_vtol_and_refuses_bad_problems():
    c = case("k6_n200_raw")
    rows, y, C, _, _ = problems(c)[0]
    with pytest.raises(RuntimeError, match="violation"):
        lr_l1.lr_l1_host(c["x"], rows, y, 6, C, max_iter=16)
    x = np.zeros((40, 8), np.float32)
    for bad_rows, bad_labels in (([0, 1], [0, 3]), ([0, 40], [0, 1]), ([], [])):
        with pytest.raises(ValueError):
            lr_l1.lr_l1_host(x, bad_rows, bad_labels, 3)


def test_check_problems_refusals_come_before_any_upload():
    """numpy input: a refused call never reaches torch.cuda (this test runs without a GPU)."""
    x = np.zeros((40, 8), np.float32)
    rows, labels = np.arange(40) % 40, np.arange(40) % 3
    fit = lr_l1.fit_on_device
    for offsets in ([0, 20, 10, 40], [-1, 40], [0, 41], []):
        with pytest.raises(ValueError, match="offsets"):
            fit(x, rows, labels, offsets, 3)
    for K in (1, 9):
        with pytest.raises(ValueError, match="n_classes"):
            fit(x, rows, labels, [0, 40], K)
    with pytest.raises(ValueError, match="at most 1024"):
        fit(x, np.zeros(1025, np.int64), np.zeros(1025, np.int64), [0, 1025], 3)
    with pytest.raises(ValueError, match="dim"):
        fit(np.zeros((4, 1025), np.float32), rows[:4], labels[:4], [0, 4], 3)
    for C in (0.0, np.nan):
        with pytest.raises(ValueError, match="positive"):
            fit(x, rows, labels, [0, 40], 3, C=C)
    with pytest.raises(ValueError, match="max_iter"):
        fit(x, rows, labels, [0, 40], 3, max_iter=0)
    with pytest.raises(ValueError, match="vtol"):
        fit(x, rows, labels, [0, 40], 3, vtol=float("nan"))
    assert (lr_l1.MAX_ROWS, lr_l1.MAX_CLASSES, lr_l1.MAX_DIM) == (logreg.MAX_ROWS, logreg.MAX_CLASSES, logreg.MAX_DIM) == (1024, 8, 1024)
    assert lr_l1.predict_host is logreg.predict_host and not hasattr(lr_l1, "standardize")


def test_module_imports_neither_scipy_nor_sklearn():
    src = open(os.path.join(ROOT, "multilingual_kws_amd", "lr_l1.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", src, flags=re.M)


def test_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mkws.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, ret, res, n_args in (("mkws_lr_l1_fit", "int", ctypes.c_int, 18), ("mkws_lr_l1_work_floats", "size_t", ctypes.c_size_t, 3)):
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", src), name
        assert hasattr(L, name), name
        assert bound[name][0] is res and len(bound[name][1]) == n_args
        assert getattr(_lib.lib(), name).argtypes == bound[name][1]
    assert bound["mkws_lr_l1_fit"][1][10] is ctypes.c_double           # vtol
    lib = _lib.lib()
    assert lib.mkws_lr_l1_work_floats(1024, 200, 6) == 0               # the iterates live in registers and LDS
    # refused arguments are refused before any device is touched
    call = lambda dim, P, K, max_iter, vtol: lib.mkws_lr_l1_fit(None, 4, dim, None, None, None, P, K, None, max_iter, vtol, None, None, None, None, None, 0, None)
    assert call(8, 1, 9, 10, 1e-3) == -2 and call(1025, 1, 3, 10, 1e-3) == -2          # MKWS_ERR_UNSUPPORTED: above a cap
    assert call(8, 1, 1, 10, 1e-3) == -1 and call(0, 1, 3, 10, 1e-3) == -1 and call(8, -1, 3, 10, 1e-3) == -1      # MKWS_ERR_INVALID_ARG
    assert call(8, 1, 3, 0, 1e-3) == -1                                                 # max_iter = 0
    assert call(8, 1, 3, 10, float("nan")) == -1 and call(8, 1, 3, 10, -1.0) == -1
    assert call(8, 1, 3, 10, 1e-3) == -1                                                # NULL buffers
    assert call(8, 0, 3, 10, 1e-3) == 0                                                 # P = 0


def test_harness_lr_l1_on_the_host_path():
    """The contract's dicts, repeatable, and equal to a plain loop over lr_l1_host + predict_host."""
    bank, word_rows, ut, ue = stub_bank(spread=2.5)
    exps = [experiment(word_rows, WORDS[:3]), experiment(word_rows, WORDS[4:7])]
    splits = [splits_for(e, 2, 10 + i) for i, e in enumerate(exps)]
    out = se.experiment_run_many(bank, exps, ut, ue, splits, classifier="lr_l1", on_device=False)
    assert out == se.experiment_run_many(bank, exps, ut, ue, splits, classifier="lr_l1", on_device=False)
    assert len(out) == 2
    for e, sp, r in zip(exps, splits, out):
        assert set(r) == {"words", "score", "crossfold_scores", "best_split"} and r["words"] == e["words"]
        train_rows = np.concatenate(e["train_rows"])
        train_y = np.concatenate([np.full(len(t), i + 1) for i, t in enumerate(e["train_rows"])])
        dev_rows = np.concatenate(list(e["dev_rows"]) + [ue])
        dev_y = np.concatenate([np.full(len(t), i + 1) for i, t in enumerate(e["dev_rows"])] + [np.zeros(len(ue), np.int64)])
        scores, models = [], []
        for tr, va in sp:
            m = lr_l1.lr_l1_host(bank, np.concatenate([train_rows[tr], ut]), np.concatenate([train_y[tr], np.zeros(len(ut), np.int64)]), 4, 1.0)
            pred = logreg.predict_host(bank, np.concatenate([train_rows[va], ue]), m.coef, m.intercept)[0]
            scores.append(float((pred == np.concatenate([train_y[va], np.zeros(len(ue), np.int64)])).mean()))
            models.append(m)
        best = int(np.argmax(scores))
        final = float((logreg.predict_host(bank, dev_rows, models[best].coef, models[best].intercept)[0] == dev_y).mean())
        assert r["crossfold_scores"] == pytest.approx(scores, abs=1e-12) and r["best_split"] == best and r["score"] == pytest.approx(final, abs=1e-12)
        assert len(dev_y) == 3 * N_DEV + N_UNKNOWN


def test_harness_names():
    bank, word_rows, ut, ue = stub_bank(spread=2.5)
    exps = [experiment(word_rows, WORDS[:3])]
    splits = [splits_for(exps[0], 2, 10)]
    assert se.experiment_run_many(bank, exps, ut, ue, splits, classifier="lr_l2", on_device=False) == \
        se.experiment_run_many(bank, exps, ut, ue, splits, classifier="lr", on_device=False)
    assert sorted(se.IMPLEMENTATIONS) == sorted(se.CLASSIFIERS) and se.CLASSIFIERS["lr_l1"] is False and se.CLASSIFIERS["lr_l2"] is False
    assert se.IMPLEMENTATIONS["lr_l2"] is se.IMPLEMENTATIONS["lr"] and se.IMPLEMENTATIONS["lr_l1"].max_iter == lr_l1.MAX_ITER
    for name in ("random_forest", "gradient_boosting"):
        with pytest.raises(ValueError, match="classifier.*probability"):
            se.experiment_run_many(bank, exps, ut, ue, splits, classifier=name)
