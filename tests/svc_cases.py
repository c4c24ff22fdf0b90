"""Inputs shared by tests/test_svc_cpu.py, tests/test_svc_gpu.py and tests/golden/make_svc_golden.py: embedding-like banks and row
lists, regenerated from seeds (the generators of tests/logreg_cases.py), built once and left unchanged.

case(name) -> dict(x float32 [bank rows, dim], rows / labels int32 (one flat list), offsets int32 [P + 1] into those lists, n_classes,
C float64 [P], standardize, eval_rows / eval_true / eval_offsets: the rows every problem is evaluated on = training rows, then held-out
rows of the same classes)."""
import hashlib

import numpy as np

import logreg_cases

from multilingual_kws_amd import svc

U = 2.0 ** -24

CASES = ["n5_k2_dim1024", "n12_k3_dim37", "ragged_50_20_64", "same_vector_both_labels", "65_problems_of_8_dim16", "k6_n200_raw",
         "k6_n200_scaled", "constant_column_scaled", "c_0p01_1_100", "absent_class", "caps_n1024_k8_dim1024"]

# these are the banks and lists of tests/logreg_cases.py under the same names (poisoned lead and tail rows, shuffled lists, a row shared by
# two problems and a duplicated row in the ragged case)
_SHARED = {"ragged_50_20_64", "65_problems_of_8_dim16", "k6_n200_raw", "k6_n200_scaled", "constant_column_scaled", "c_0p01_1_100", "absent_class"}

_CACHE = {}


def _make(name):
    if name in _SHARED:
        return dict(logreg_cases._make(name))
    if name == "n5_k2_dim1024":
        return logreg_cases._build([5], 1024, 2, 201)
    if name == "n12_k3_dim37":
        return logreg_cases._build([12], 37, 3, 202)
    if name == "same_vector_both_labels":
        # list entries 3 and 17 name one bank row, once as class 0 and once as class 1; entry 9 names it a third time as class 2
        c = logreg_cases._build([30], 48, 3, 203)
        rows, labels = c["rows"].copy(), c["labels"].copy()
        labels[3], labels[17], labels[9] = 0, 1, 2
        rows[17] = rows[9] = rows[3]
        c["rows"], c["labels"] = rows, labels
        return c
    if name == "caps_n1024_k8_dim1024":
        # evaluated on 128 of its training rows and the 64 held-out ones (the fixture stays small)
        c = logreg_cases._build([1024], 1024, 8, 109, n_eval=64)
        keep = np.concatenate([np.arange(0, 1024, 8), 1024 + np.arange(64)])
        c["eval_rows"], c["eval_true"] = c["eval_rows"][keep], c["eval_true"][keep]
        c["eval_offsets"] = np.asarray([0, len(keep)], np.int32)
        return c
    raise KeyError(name)


def case(name):
    if name not in _CACHE:
        c = _make(name)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


def problems(c):
    """-> [(rows, labels, C, eval rows, eval labels)] of a case, problem by problem."""
    return logreg_cases.problems(c)


def x_hash(c):
    return hashlib.sha1(np.ascontiguousarray(c["x"]).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ the bounds the tests hold the device to

def present_columns(y, K):
    present = np.bincount(y, minlength=K) > 0
    return [q for q, (i, j) in enumerate(svc.pairs(K)) if present[i] and present[j]]


def weighted(coef, rho, y, K, kv):
    """[eval rows, pairs]: sum_t |c_t| kv[t, e] + |rho| per pair, the magnitude the storage and dot-product bounds scale with."""
    out = np.zeros((kv.shape[1], K * (K - 1) // 2))
    coef = np.abs(np.asarray(coef, np.float64))
    for q, (i, j) in enumerate(svc.pairs(K)):
        ti, tj = y == i, y == j
        if ti.any() and tj.any():
            out[:, q] = coef[ti, svc._slot(i, j)] @ kv[ti] + coef[tj, svc._slot(j, i)] @ kv[tj] + abs(float(rho[q]))
    return out


def kernel_bound(x, rows_a, rows_b, centre, inv_scale, gamma):
    """k * gamma * 2 gamma_n (s_a + s_b) + 4 u per entry, gamma_n = n u / (1 - n u), n = dim + 8, u = 2^-24: the eight covers centring,
    scaling, the three-term sum, the product with gamma and the exponential's documented error (here the device library's float64 exp
    rounded once to float32, well inside the 4 u)."""
    n = x.shape[1] + 8
    g_n = n * U / (1 - n * U)
    c, s = np.asarray(centre, np.float64), np.asarray(inv_scale, np.float64)
    sa = (((x[rows_a].astype(np.float64) - c) * s) ** 2).sum(axis=1)
    sb = (((x[rows_b].astype(np.float64) - c) * s) ** 2).sum(axis=1)
    k = svc.kernel_host(x, rows_a, rows_b, centre, inv_scale, gamma)
    return k, k * float(gamma) * 2 * g_n * (sa[:, None] + sb[None, :]) + 4 * U


def score_bound(x, rows, y, K, coef, rho, ev_rows, centre, inv_scale, gamma):
    """[eval rows, pairs]: what float32 decision values may differ by from the float64 value of the same model: the kernel bound summed
    over |c_t|, plus the float32 dot-product bound gamma_n (sum_t |c_t| k_t + |rho|), n = rows + 3 (the products, the sum of the two class
    sums and the subtraction of rho)."""
    kv, kb = kernel_bound(x, rows, ev_rows, centre, inv_scale, gamma)
    n = len(rows) + 3
    return weighted(coef, np.zeros_like(np.asarray(rho, np.float64)), y, K, kb) + n * U / (1 - n * U) * weighted(coef, rho, y, K, kv)


def fit_bound(x, rows, y, K, coef_star, rho_star, ev_rows, e_sk, standardize):
    """[eval rows, pairs]: max(e_sk, 2^-23 (sum_t |c*_t| k_t + |rho*|)): sklearn's own distance from the optimum, or the float32 storage of
    the optimum where sklearn is exact."""
    mu, inv, gamma = svc.scaling(x, rows, standardize)
    return np.maximum(e_sk, 2.0 ** -23 * weighted(coef_star, rho_star, y, K, svc.kernel_host(x, rows, ev_rows, mu, inv, gamma)))
