"""Generates tests/golden/logreg_golden.npz on the CPU (scipy-free; sklearn is needed here and only here): for every case of
tests/logreg_cases.py and every problem of it

  theta_star  float64 [K * dim + K] = logreg_host's (coef.ravel(), intercept) in raw space, and f_star its objective;
  f_sklearn   the float64 objective at what sklearn.linear_model.LogisticRegression(C=C) returns with its defaults (lbfgs, tol 1e-4,
              max_iter 100) -- the two-row form W = (-w / 2, w / 2) for K = 2, fitted after a StandardScaler for the scaled cases, a class
              sklearn did not see given a zero row and an intercept of -50 (probability 0, as sklearn predicts it);
  p_sklearn   max |P_sklearn - P*| over the problem's evaluation rows;
  bound_ok    the share of the evaluation rows whose float64 top-two logit gap at theta_star exceeds twice the float32 dot-product bound
              (asserted >= 0.9 here: tests/test_logreg_gpu.py compares predictions with == on such rows);

and a hash of each bank.  The GPU tests read only this file plus NumPy."""
import os
import sys
import warnings

import numpy as np
import sklearn.linear_model
import sklearn.preprocessing

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from logreg_cases import CASES, case, problems, x_hash  # noqa: E402
from multilingual_kws_amd import logreg  # noqa: E402

U = 2.0 ** -24


def dot_bound(x_rows, coef, dim):
    """gamma_{dim+1} * sum_j |w_j x_j| (+ |b|): the rounding bound of a float32 dot product of dim terms and the bias, in any order."""
    g = (dim + 1) * U / (1 - (dim + 1) * U)
    return g * (np.abs(x_rows.astype(np.float64))[:, None, :] * np.abs(coef.astype(np.float64))[None]).sum(-1)


def sklearn_point(x, rows, y, K, C, standardize):
    """(coef, intercept) of sklearn's default run in this module's raw-space K-row form."""
    X = x[rows].astype(np.float64)
    mu, sigma = np.zeros(X.shape[1]), np.ones(X.shape[1])
    if standardize:
        sc = sklearn.preprocessing.StandardScaler().fit(X)
        mu, sigma = sc.mean_, sc.scale_
        X = sc.transform(X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = sklearn.linear_model.LogisticRegression(C=C).fit(X, y)
    W, b = np.zeros((K, X.shape[1])), np.full(K, -50.0)
    if K == 2:
        assert clf.classes_.tolist() == [0, 1]
        W[1], W[0], b[1], b[0] = clf.coef_[0] / 2, -clf.coef_[0] / 2, clf.intercept_[0] / 2, -clf.intercept_[0] / 2
    else:
        assert len(clf.classes_) >= 3
        W[clf.classes_], b[clf.classes_] = clf.coef_, clf.intercept_
    coef = W / sigma
    return coef, b - coef @ mu, clf


if __name__ == "__main__":
    out = {}
    for name in CASES:
        c = case(name)
        K, dim, std = c["n_classes"], c["x"].shape[1], c["standardize"]
        theta, f_star, f_sk, p_sk, ok = [], [], [], [], []
        for rows, y, C, ev_rows, _ in problems(c):
            h = logreg.logreg_host(c["x"], rows, y, K, C, std)
            coef, intercept, clf = sklearn_point(c["x"], rows, y, K, C, std)
            fs, _ = logreg.objective(c["x"], rows, y, K, C, coef, intercept, std)
            _, p_star = logreg.predict_host(c["x"], ev_rows, h.coef, h.intercept)
            _, p_skl = logreg.predict_host(c["x"], ev_rows, coef, intercept)
            z = c["x"][ev_rows].astype(np.float64) @ h.coef.T + h.intercept
            top = np.sort(z, axis=1)
            bound = dot_bound(c["x"][ev_rows], h.coef.astype(np.float32), dim).max(axis=1)
            theta.append(np.concatenate([h.coef.ravel(), h.intercept]))
            f_star.append(h.f)
            f_sk.append(fs)
            p_sk.append(np.abs(p_skl - p_star).max())
            ok.append(float(np.mean(top[:, -1] - top[:, -2] > 2 * bound)))
            assert fs >= h.f and ok[-1] >= 0.9, (name, fs, h.f, ok[-1])
        print(f"{name}: P = {len(f_star)}, f_sklearn - f_star in [{min(np.subtract(f_sk, f_star)):.3e}, {max(np.subtract(f_sk, f_star)):.3e}], "
              f"p_sklearn in [{min(p_sk):.3e}, {max(p_sk):.3e}], rows with a clear argmax >= {min(ok):.3f}", flush=True)
        out[name + "/theta_star"] = np.stack(theta)
        out[name + "/f_star"] = np.asarray(f_star)
        out[name + "/f_sklearn"] = np.asarray(f_sk)
        out[name + "/p_sklearn"] = np.asarray(p_sk)
        out[name + "/bound_ok"] = np.asarray(ok)
        out[name + "/x_sha1"] = np.asarray(x_hash(c))
    np.savez_compressed(os.path.join(HERE, "logreg_golden.npz"), **out)
