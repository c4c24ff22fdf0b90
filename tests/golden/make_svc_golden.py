"""Generates tests/golden/svc_golden.npz on the CPU (sklearn is needed here and only here): for every case of tests/svc_cases.py

  x_sha1      a hash of the bank;
  gamma_star  float64 [P];
  coef_star   float64 [list entries, K - 1] and rho_star float64 [P, K (K - 1) / 2]: svc_host at tol 1e-10, aligned with the flat lists;
  f_star      float64 [evaluation entries, K (K - 1) / 2]: decision_host of that model on the case's evaluation lists;
  f_sk        the decision values of sklearn.svm.SVC(C=C) with its defaults (tol 1e-3), fitted after a StandardScaler for the scaled
              cases, in the libsvm convention (class i of pair (i, j) positive: for two classes sklearn returns the negated value), 0 in
              the columns of pairs with an absent class;
  e_sk        float64 [P] = max |f_sk - f_star| over the problem's evaluation rows;
  clear       float64 [P] = the share of evaluation rows whose every pairwise |f_star| exceeds 2 e_sk (asserted >= 0.9 here), and
  clear_votes the share that also clears twice the sum of the fit bound and the float32 scorer's bound of tests/svc_cases.py, formed at
              the optimum (asserted >= 0.9: tests/test_svc_gpu.py compares predictions with == on such rows and asks for 0.9 with the
              bound formed at the device's own coefficients);
  tight_sk    float64 [P] = max |f(SVC(tol=1e-9)) - f_star|: how far libsvm (float32 kernel cache) itself sits from the float64 optimum.

The GPU tests read only this file plus NumPy."""
import os
import sys
import time

import numpy as np
import sklearn.preprocessing
import sklearn.svm

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from svc_cases import CASES, case, fit_bound, problems, score_bound, x_hash  # noqa: E402
from multilingual_kws_amd import svc  # noqa: E402


def sklearn_decision(x, rows, y, K, C, standardize, ev_rows, tol=None):
    """sklearn's decision values on ev_rows in this module's layout and sign -> (float64 [len(ev_rows), K (K - 1) / 2], the classifier)."""
    X, E = x[rows].astype(np.float64), x[ev_rows].astype(np.float64)
    if standardize:
        sc = sklearn.preprocessing.StandardScaler().fit(X)
        X, E = sc.transform(X), sc.transform(E)
    clf = sklearn.svm.SVC(C=C, decision_function_shape="ovo", **({} if tol is None else dict(tol=tol))).fit(X, y)
    d = clf.decision_function(E)
    present = clf.classes_.tolist()
    d = -d[:, None] if len(present) == 2 else d
    out, col = np.zeros((len(ev_rows), K * (K - 1) // 2)), 0
    for q, (i, j) in enumerate(svc.pairs(K)):
        if i in present and j in present:
            out[:, q] = d[:, col]
            col += 1
    assert col == d.shape[1]
    return out, clf


if __name__ == "__main__":
    out = {}
    for name in CASES:
        c = case(name)
        K, std = c["n_classes"], c["standardize"]
        coef = np.zeros((len(c["rows"]), K - 1))
        rho, gam, f_star, f_sk, e_sk, clear, tight, its, votes = [], [], [], [], [], [], [], [], []
        t0 = time.time()
        for p, (rows, y, C, ev_rows, _) in enumerate(problems(c)):
            h = svc.svc_host(c["x"], rows, y, K, C, std)
            lo = int(c["offsets"][p])
            coef[lo:lo + len(rows)] = h.coef
            fs = svc.decision_host(c["x"], ev_rows, rows, y, K, h.coef, h.rho, h.gamma, h.centre, h.inv_scale)
            fk, clf = sklearn_decision(c["x"], rows, y, K, C, std, ev_rows)
            ft, _ = sklearn_decision(c["x"], rows, y, K, C, std, ev_rows, tol=1e-9)
            assert abs(clf._gamma - h.gamma) <= 1e-12 * h.gamma, (name, clf._gamma, h.gamma)
            present = np.bincount(y, minlength=K) > 0
            cols = [q for q, (i, j) in enumerate(svc.pairs(K)) if present[i] and present[j]]
            e = float(np.abs(fk - fs).max())
            share = float(np.mean((np.abs(fs[:, cols]) > 2 * e).all(axis=1)))
            assert share >= 0.9, (name, p, share)
            both = fit_bound(c["x"], rows, y, K, h.coef, h.rho, ev_rows, e, std) + score_bound(c["x"], rows, y, K, h.coef, h.rho, ev_rows, h.centre, h.inv_scale, h.gamma)
            votes.append(float(np.mean((np.abs(fs[:, cols]) > 2 * both[:, cols]).all(axis=1))))
            assert votes[-1] >= 0.9, (name, p, votes[-1])
            rho.append(h.rho), gam.append(h.gamma), f_star.append(fs), f_sk.append(fk), e_sk.append(e), clear.append(share)
            tight.append(float(np.abs(ft - fs).max())), its.append(h.n_iter)
        print(f"{name}: P = {len(rho)}, e_sk in [{min(e_sk):.3e}, {max(e_sk):.3e}], SVC(tol=1e-9) within {max(tight):.3e}, clear rows >= {min(clear):.3f} (votes {min(votes):.3f}), "
              f"iterations <= {max(its)}, {time.time() - t0:.1f} s", flush=True)
        out[name + "/x_sha1"] = np.asarray(x_hash(c))
        out[name + "/gamma_star"] = np.asarray(gam)
        out[name + "/coef_star"] = coef
        out[name + "/rho_star"] = np.stack(rho)
        out[name + "/f_star"] = np.concatenate(f_star)
        out[name + "/f_sk"] = np.concatenate(f_sk)
        out[name + "/e_sk"] = np.asarray(e_sk)
        out[name + "/clear"] = np.asarray(clear)
        out[name + "/clear_votes"] = np.asarray(votes)
        out[name + "/tight_sk"] = np.asarray(tight)
    np.savez_compressed(os.path.join(HERE, "svc_golden.npz"), **out)
