"""Generates tests/golden/lr_l1_golden.npz on the CPU (sklearn is needed here): for every case of tests/lr_l1_cases.py

  f_star [P, K], viol_star [P, K]     lr_l1_host's objective and violation (<= 1e-8) per class;
  w_index, w_value                     the optimum's non-zero weights: flat indices into [P, K, dim + 1] (the bias last) and float64 values;
  z_star [eval rows, K]                the optimum's float64 logits on the case's evaluation rows, problem after problem;
  f_sklearn, viol_sklearn [P, K]       objective and violation at what LogisticRegression(penalty="l1", solver="liblinear", C=C,
                                       random_state=0) returns with its defaults (tol 1e-4); a class sklearn never saw has no model of
                                       its own there and is given the optimum (gap 0), K = 2 is its one model and the mirror;
  f_sklearn_tight [P, K]               the same at tol=1e-10, max_iter=200000 (asserted here: |f_star - it| <= 1e-8 f_star, and the same
                                       non-zero pattern);
  x_sha1                               a hash of the bank.

The GPU tests read only this file plus NumPy."""
import os
import sys
import warnings

import numpy as np
import sklearn.linear_model

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from lr_l1_cases import CASES, case, problems, x_hash  # noqa: E402
from multilingual_kws_amd import lr_l1  # noqa: E402


def sklearn_point(x, rows, y, K, C, star=None, **kw):
    """-> (W [K, dim + 1] with the bias last, seen bool [K]) of sklearn's run; a class it never saw takes the row of `star`."""
    X = x[rows].astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = sklearn.linear_model.LogisticRegression(penalty="l1", solver="liblinear", C=C, random_state=0, **kw).fit(X, y)
    W = np.zeros((K, X.shape[1] + 1)) if star is None else np.array(star, dtype=np.float64)
    seen = np.zeros(K, bool)
    got = np.hstack([clf.coef_, clf.intercept_[:, None]])
    if K == 2:
        assert clf.classes_.tolist() == [0, 1]
        W[1], W[0] = got[0], np.where(got[0] == 0.0, 0.0, -got[0])
        seen[:] = True
    else:
        W[clf.classes_] = got
        seen[clf.classes_] = True
    return W, seen


if __name__ == "__main__":
    out = {}
    for name in CASES:
        c = case(name)
        K, dim = c["n_classes"], c["x"].shape[1]
        f_star, v_star, f_sk, v_sk, f_tight, W_star, z_star = [], [], [], [], [], [], []
        for rows, y, C, ev_rows, _ in problems(c):
            h = lr_l1.lr_l1_host(c["x"], rows, y, K, C)
            star = np.hstack([h.coef, h.intercept[:, None]])
            sk, _ = sklearn_point(c["x"], rows, y, K, C, star)
            tight, seen = sklearn_point(c["x"], rows, y, K, C, star, tol=1e-10, max_iter=200000)
            fs, vs = lr_l1.objective(c["x"], rows, y, K, C, sk[:, :dim], sk[:, dim])
            ft, _ = lr_l1.objective(c["x"], rows, y, K, C, tight[:, :dim], tight[:, dim])
            assert (h.violation <= 1e-8).all() and (np.abs(h.f - ft) <= 1e-8 * h.f).all(), (name, h.f, ft)
            assert np.array_equal(star != 0.0, tight != 0.0), name
            assert (fs >= h.f - 1e-9 * h.f).all(), (name, fs, h.f)
            f_star.append(h.f)
            v_star.append(h.violation)
            f_sk.append(fs)
            v_sk.append(vs)
            f_tight.append(ft)
            W_star.append(star)
            z_star.append(c["x"][ev_rows].astype(np.float64) @ h.coef.T + h.intercept)
        W_star = np.stack(W_star)
        gap = (np.sum(f_sk) - np.sum(f_star)) / np.sum(f_star)
        print(f"{name}: P = {len(f_star)}, non-zeros per class <= {int((W_star != 0).sum(axis=2).max())} of {dim + 1}, sklearn's default run: "
              f"relative gap {gap:.2e}, violation in [{np.min(v_sk):.1e}, {np.max(v_sk):.1e}]; max |f_star - f_tight| / f_star "
              f"{np.max(np.abs(np.subtract(f_star, f_tight)) / np.asarray(f_star)):.1e}", flush=True)
        at = np.flatnonzero(W_star)
        out[name + "/f_star"] = np.asarray(f_star)
        out[name + "/viol_star"] = np.asarray(v_star)
        out[name + "/w_index"] = at.astype(np.int32)
        out[name + "/w_value"] = W_star.reshape(-1)[at]
        out[name + "/z_star"] = np.concatenate(z_star)
        out[name + "/f_sklearn"] = np.asarray(f_sk)
        out[name + "/viol_sklearn"] = np.asarray(v_sk)
        out[name + "/f_sklearn_tight"] = np.asarray(f_tight)
        out[name + "/x_sha1"] = np.asarray(x_hash(c))
    np.savez_compressed(os.path.join(HERE, "lr_l1_golden.npz"), **out)
