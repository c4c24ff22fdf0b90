"""The logistic-regression specification and the host side of the device solver (multilingual_kws_amd/logreg.py) without a GPU:
logreg_host against scipy's L-BFGS-B and against sklearn's own run, the binary penalty, the golden fixture, the refusals, the C symbols."""
import ctypes
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from logreg_cases import CASES, case, problems, x_hash  # noqa: E402

from multilingual_kws_amd import _lib, logreg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HOST = {}


def host(name):
    """logreg_host on every problem of a case; computed once and left unchanged."""
    if name not in _HOST:
        c = case(name)
        _HOST[name] = [logreg.logreg_host(c["x"], rows, y, c["n_classes"], C, c["standardize"]) for rows, y, C, _, _ in problems(c)]
    return _HOST[name]


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "logreg_golden.npz"))


@pytest.mark.parametrize("name", CASES)
def test_fixture_equals_a_fresh_host_run(name, golden_dir):
    g, c = golden(golden_dir), case(name)
    assert str(g[name + "/x_sha1"]) == x_hash(c)
    want = host(name)
    assert g[name + "/theta_star"].shape == (len(want), c["n_classes"] * (c["x"].shape[1] + 1))
    for p, h in enumerate(want):
        assert h.gnorm <= 1e-8 and abs(h.intercept.sum() + (h.coef @ _mu(c, p)).sum()) <= 1e-9 * max(1.0, np.abs(h.intercept).max())
        assert abs(g[name + "/f_star"][p] - h.f) <= 1e-12 * max(1.0, h.f)
        # the optimum is unique in W; to the solver's gradient tolerance two runs agree far below the figures the GPU tests compare
        assert np.abs(g[name + "/theta_star"][p] - np.concatenate([h.coef.ravel(), h.intercept])).max() <= 1e-9
        assert g[name + "/f_sklearn"][p] >= g[name + "/f_star"][p] and g[name + "/bound_ok"][p] >= 0.9


def _mu(c, p):
    """The mean the problem was centred by (zero for the raw cases): sum_k b~_k = sum_k (b_k + W_k . mu) = 0."""
    rows = problems(c)[p][0]
    return c["x"][rows].astype(np.float64).mean(axis=0) if c["standardize"] else np.zeros(c["x"].shape[1])


@pytest.mark.parametrize("name", CASES)
def test_host_reaches_the_optimum_scipy_finds(name):
    """|f - f_scipy| <= 1e-9 * max(1, f) against L-BFGS-B with gtol 1e-10 on the same float64 objective (the first three problems of a
    case; the 65-problem case adds nothing after that)."""
    optimize = pytest.importorskip("scipy.optimize")
    c = case(name)
    K, dim = c["n_classes"], c["x"].shape[1]
    for (rows, y, C, _, _), h in list(zip(problems(c), host(name)))[:3]:
        Xs, yy, _, _ = logreg._problem(c["x"], rows, y, K, c["standardize"])

        def fun(theta):
            f, gW, gb, _ = logreg._value_grad(Xs, yy, K, C, theta[:K * dim].reshape(K, dim), theta[K * dim:])
            return f, np.concatenate([gW.ravel(), gb])

        res = optimize.minimize(fun, np.zeros(K * dim + K), jac=True, method="L-BFGS-B", options=dict(gtol=1e-10, ftol=0.0, maxiter=20000, maxfun=40000, maxcor=30))
        print(f"{name}: f_host {h.f:.12f}, f_scipy {res.fun:.12f}, scipy iterations {res.nit}")
        assert abs(h.f - res.fun) <= 1e-9 * max(1.0, h.f)
        assert objective_at(c, rows, y, C, h) == pytest.approx(h.f, rel=1e-13, abs=1e-13)


def objective_at(c, rows, y, C, h):
    return logreg.objective(c["x"], rows, y, c["n_classes"], C, h.coef, h.intercept, c["standardize"])[0]


@pytest.mark.parametrize("name", CASES)
def test_host_is_at_or_below_sklearn(name):
    linear_model = pytest.importorskip("sklearn.linear_model")
    preprocessing = pytest.importorskip("sklearn.preprocessing")
    c = case(name)
    K = c["n_classes"]
    for (rows, y, C, _, _), h in list(zip(problems(c), host(name)))[:3]:
        X = c["x"][rows].astype(np.float64)
        if c["standardize"]:
            X = preprocessing.StandardScaler().fit_transform(X)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            clf = linear_model.LogisticRegression(C=C).fit(X, y)
        W, b = np.zeros((K, X.shape[1])), np.full(K, -50.0)          # (a class sklearn did not see: probability 0, as it predicts)
        if K == 2:
            W[1], W[0], b[1], b[0] = clf.coef_[0] / 2, -clf.coef_[0] / 2, clf.intercept_[0] / 2, -clf.intercept_[0] / 2
        else:
            W[clf.classes_], b[clf.classes_] = clf.coef_, clf.intercept_
        f_sk = logreg._value_grad(X, np.asarray(y, np.int64), K, C, W, b)[0]
        assert h.f <= f_sk + 1e-12 * max(1.0, h.f), (name, h.f, f_sk)


def test_two_classes_take_the_binary_penalty():
    """kappa = 2 at K = 2: W[1] - W[0] is sklearn's coef_.  With kappa = 1 the two-row problem is regularised half as strongly -- it is
    the kappa = 2 problem at C doubled -- and its W[1] - W[0] is further from sklearn's."""
    linear_model = pytest.importorskip("sklearn.linear_model")
    c = case("n10_k2_dim1024")
    rows, y, C, ev_rows, _ = problems(c)[0]
    clf = linear_model.LogisticRegression(C=C, tol=1e-10, max_iter=10000).fit(c["x"][rows].astype(np.float64), y)
    ours = logreg.logreg_host(c["x"], rows, y, 2, C)
    half = logreg.logreg_host(c["x"], rows, y, 2, 2 * C)              # what kappa = 1 would solve
    assert logreg.kappa(2) == 2.0 and logreg.kappa(3) == 1.0 == logreg.kappa(8)
    d_ours = np.abs((ours.coef[1] - ours.coef[0]) - clf.coef_[0]).max()
    d_half = np.abs((half.coef[1] - half.coef[0]) - clf.coef_[0]).max()
    scale = np.abs(clf.coef_[0]).max()
    assert d_ours <= 1e-6 * scale and d_half >= 1e-2 * scale, (d_ours, d_half, scale)
    assert abs((ours.intercept[1] - ours.intercept[0]) - clf.intercept_[0]) <= 1e-6 * max(1.0, abs(clf.intercept_[0]))
    p_ours = logreg.predict_host(c["x"], ev_rows, ours.coef, ours.intercept)[1]
    assert np.abs(p_ours - clf.predict_proba(c["x"][ev_rows].astype(np.float64))).max() <= 1e-6


def test_objective_gradient_and_scaled_space():
    c = case("constant_column_scaled")
    rows, y, C, _, _ = problems(c)[0]
    K, dim = 3, c["x"].shape[1]
    rng = np.random.default_rng(0)
    W, b = 0.1 * rng.standard_normal((K, dim)), rng.standard_normal(K)
    for std in (False, True):
        f, g = logreg.objective(c["x"], rows, y, K, C, W, b, std)
        assert g.shape == (K * dim + K,) and abs(g[K * dim:].sum()) <= 1e-9      # sum_k (P - Y) = 0
        Xs, yy, mu, sigma = logreg._problem(c["x"], rows, y, K, std)
        Wt, bt = W * sigma, b + W @ mu
        for _ in range(5):                                           # central differences in the space the problem is posed in
            dW, db = rng.standard_normal((K, dim)), rng.standard_normal(K)
            h = 1e-6
            fp = logreg._value_grad(Xs, yy, K, C, Wt + h * dW, bt + h * db)[0]
            fm = logreg._value_grad(Xs, yy, K, C, Wt - h * dW, bt - h * db)[0]
            assert (fp - fm) / (2 * h) == pytest.approx(g[:K * dim] @ dW.ravel() + g[K * dim:] @ db, rel=1e-5)
    h = logreg.logreg_host(c["x"], rows, y, K, C, True)
    assert h.coef[:, 5].tolist() == [0.0] * K and h.coef[:, 9].tolist() == [0.0] * K        # a constant column carries no weight
    f0, _ = logreg.objective(c["x"], rows, y, K, C, np.zeros((K, dim)), np.zeros(K), True)
    assert f0 == pytest.approx(C * len(rows) * np.log(K), rel=1e-12)


def test_predict_host():
    c = case("n7_k3_dim37")
    rows, y, C, ev_rows, _ = problems(c)[0]
    h = host("n7_k3_dim37")[0]
    pred, probs = logreg.predict_host(c["x"], ev_rows, h.coef, h.intercept)
    assert pred.dtype == np.int32 and probs.shape == (len(ev_rows), 3) and np.allclose(probs.sum(1), 1.0, atol=1e-12)
    assert pred.tolist() == probs.argmax(1).tolist()
    assert logreg.predict_host(c["x"], [], h.coef, h.intercept)[0].shape == (0,)


def test_check_problems_refusals_come_before_any_upload():
    """numpy input: a refused call never reaches torch.cuda (this test runs without a GPU)."""
    x = np.zeros((40, 8), np.float32)
    rows, labels = np.arange(40) % 40, np.arange(40) % 3
    fit = logreg.fit_on_device
    for offsets in ([0, 20, 10, 40], [-1, 40], [0, 41], [[0, 40]], [0.0, 40.0], []):
        with pytest.raises(ValueError, match="offsets"):
            fit(x, rows, labels, offsets, 3)
    for K in (1, 0, 9):
        with pytest.raises(ValueError, match="n_classes"):
            fit(x, rows, labels, [0, 40], K)
    with pytest.raises(ValueError, match="at most 1024"):
        fit(x, np.zeros(1025, np.int64), np.zeros(1025, np.int64), [0, 1025], 3)
    with pytest.raises(ValueError, match="dim"):
        fit(np.zeros((4, 1025), np.float32), rows[:4], labels[:4], [0, 4], 3)
    with pytest.raises(ValueError, match="labels"):
        fit(x, rows, labels[:39], [0, 40], 3)
    with pytest.raises(ValueError, match="integers"):
        fit(x, rows.astype(np.float64), labels, [0, 40], 3)
    with pytest.raises(ValueError, match="values of C"):
        fit(x, rows, labels, [0, 20, 40], 3, C=[1.0, 2.0, 3.0])
    for C in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="positive"):
            fit(x, rows, labels, [0, 40], 3, C=C)
    with pytest.raises(ValueError, match="float32"):
        fit(x.astype(np.float64), rows, labels, [0, 40], 3)
    with pytest.raises(ValueError, match="max_iter"):
        fit(x, rows, labels, [0, 40], 3, max_iter=0)
    r, y, off, Cs = logreg.check_problems(rows, labels, [3, 20, 20, 37], 40, 8, 3, C=[1, 2, 3])      # an empty problem is the device's to report
    assert (r.dtype, y.dtype, off.dtype, Cs.dtype) == (np.int32, np.int32, np.int32, np.float64) and off.tolist() == [3, 20, 20, 37]
    r, _, _, _ = logreg.check_problems([2 ** 40, -2 ** 40], [0, 1], [0, 2], 40, 8, 3)              # out of int32 stays out of every bank
    assert r.tolist() == [2 ** 31 - 1, -2 ** 31]
    assert (logreg.MAX_ROWS, logreg.MAX_CLASSES, logreg.MAX_DIM) == (1024, 8, 1024)
    for bad_rows, bad_labels in (([0, 1], [0, 3]), ([0, 40], [0, 1]), ([], [])):       # the host solver refuses what the device reports
        with pytest.raises(ValueError):
            logreg.logreg_host(x, bad_rows, bad_labels, 3)


def test_module_imports_neither_scipy_nor_sklearn():
    src = open(os.path.join(ROOT, "multilingual_kws_amd", "logreg.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", src, flags=re.M)


def test_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mkws.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, ret, res, n_args in (("mkws_logreg_fit", "int", ctypes.c_int, 19), ("mkws_logreg_score", "int", ctypes.c_int, 16),
                                   ("mkws_logreg_work_floats", "size_t", ctypes.c_size_t, 3)):
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", src), name
        assert hasattr(L, name), name
        assert bound[name][0] is res and len(bound[name][1]) == n_args
        assert getattr(_lib.lib(), name).argtypes == bound[name][1]
    assert bound["mkws_logreg_fit"][1][11] is ctypes.c_double          # gtol
    for macro, value in (("MKWS_LOGREG_MAX_ROWS", 1024), ("MKWS_LOGREG_MAX_CLASSES", 8), ("MKWS_LOGREG_MAX_DIM", 1024)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", src), macro
    lib = _lib.lib()
    assert lib.mkws_abi_version() == 5
    assert lib.mkws_logreg_work_floats(1024, 200, 6) == 3 * 200 * 6 * 1024 and lib.mkws_logreg_work_floats(0, 1, 2) == 0
    # refused arguments are refused before any device is touched
    assert lib.mkws_logreg_fit(None, 4, 8, None, None, None, 1, 9, None, 0, 10, 1e-5, None, None, None, None, None, 0, None) == -2      # MKWS_ERR_UNSUPPORTED
    assert lib.mkws_logreg_fit(None, 4, 8, None, None, None, 1, 1, None, 0, 10, 1e-5, None, None, None, None, None, 0, None) == -1      # MKWS_ERR_INVALID_ARG
    assert lib.mkws_logreg_fit(None, 4, 8, None, None, None, 1, 3, None, 0, 0, 1e-5, None, None, None, None, None, 0, None) == -1
    assert lib.mkws_logreg_fit(None, 4, 8, None, None, None, 1, 3, None, 0, 10, float("nan"), None, None, None, None, None, 0, None) == -1
    assert lib.mkws_logreg_fit(None, 4, 8, None, None, None, 1, 3, None, 0, 10, 1e-5, None, None, None, None, None, 0, None) == -1      # NULL buffers
    assert lib.mkws_logreg_fit(None, 4, 8, None, None, None, 0, 3, None, 0, 10, 1e-5, None, None, None, None, None, 0, None) == 0       # P = 0
    assert lib.mkws_logreg_score(None, 4, 1025, None, None, None, 0, 3, None, None, 0, None, None, None, None, None) == -2
