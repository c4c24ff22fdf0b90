"""K L1-regularised logistic regressions on embeddings: the specification (objective, lr_l1_host) and the host wrapper over
mkws_lr_l1_fit (include/mkws.h).

What the DataPerf selection harness of the reference lists as `logistic_regression_with_l1_regularization`
(notebooks/dataperf_test_harness.py:277-280) is sklearn.linear_model.LogisticRegression(penalty="l1", solver="liblinear"): liblinear's
L1R_LR, one independent binary problem per class k (one-vs-rest), the bias an extra feature of value 1 (intercept_scaling = 1) that is
penalised like every other weight:

    f_k(w, b) = ||w||_1 + |b| + C * sum_{i in R_p} log(1 + exp(-s_ik (w . x_i + b))),      s_ik = +1 if y_i == k else -1

Prediction is the first argmax over k of w_k . x + b_k: what logreg.predict_host and mkws_logreg_score evaluate on coef [K, dim],
intercept [K].  For K = 2 sklearn fits one model; the class-0 problem is the mirror of the class-1 problem (s -> -s, w -> -w), so row 1
is solved and row 0 is its exact negation, and the argmax reproduces sklearn's sign test.  Every one of the K problems is posed even when
a class has no sample (or every sample): this module follows the objective, not sklearn's class discovery.  There w = 0 and
b = -+log(C n - 1) when C n > 1, else 0, wherever that point is optimal (it is whenever no column's mean exceeds 1 in magnitude).

The optimality measure is the minimum-norm subgradient over the dim weights and the bias: with g_j = -C sum_i s_i x_ij sigma(-s_i z_i),
v_j = g_j + sign(w_j) where w_j != 0 and sign(g_j) max(|g_j| - 1, 0) where w_j = 0; "violation" is max_j |v_j|.  The penalty weight is 1,
so the violation is already relative to it.  The solver is a proximal gradient iteration (FISTA with gradient restart) with the step
1 / L, L = STEP_SAFETY * C / 4 * lambda_max(Xa^T Xa) from a power iteration, Xa = [X, 1].
Host part: pure NumPy float64 on widened float32 inputs; neither scipy nor sklearn is imported.  No standardize: the reference has no
scaled L1 variant."""
from collections import namedtuple

import numpy as np

from . import _lib, problems
from .logreg import MAX_CLASSES, MAX_DIM, MAX_ROWS, predict_host  # noqa: F401  (the caps and the scorer are logreg's)

# What max_iter=None stands for in fit_on_device.  Seen on an MI355X at vtol 1e-3: 2128 to 2712 iterations for the six classes of the
# harness shape (k6_n200_raw of tests/logreg_cases.py, C = 1), 1352 to 3000 over 200 random subsets of it, 480 to 632 at the caps; C = 100
# does not get there in 8000 and ends with stop reason 1
MAX_ITER = 8000
POWER_ITERATIONS = 50         # of the power iteration for lambda_max (kPower of mkws_lr_l1.hip)
STEP_SAFETY = 1.02            # L = STEP_SAFETY * C / 4 * lambda_max
CHECK_EVERY = 8               # iterations between two evaluations of the violation (kCheck of mkws_lr_l1.hip)

LrL1Host = namedtuple("LrL1Host", "coef intercept f violation n_iter")
LrL1Fit = namedtuple("LrL1Fit", "coef intercept info stats d_coef d_intercept")


def _value_violation(Xa, s, C, w):
    """(f, violation) of one binary problem at w [dim + 1] (the bias last); Xa has the column of ones."""
    m = s * (Xa @ w)
    f = np.abs(w).sum() + C * np.logaddexp(0.0, -m).sum()
    g = C * (Xa.T @ (-s * np.exp(-np.logaddexp(0.0, m))))            # sigma(-m) = exp(-log(1 + exp(m)))
    v = np.where(w != 0.0, g + np.sign(w), np.sign(g) * np.maximum(np.abs(g) - 1.0, 0.0))
    return float(f), float(np.abs(v).max())


def _signs(y, K):
    return np.where(y[None, :] == np.arange(K)[:, None], 1.0, -1.0)


def objective(x, rows, labels, n_classes, C, coef, intercept):
    """-> (f [K], violation [K]) in float64 of the K one-vs-rest problems at (coef [K, dim], intercept [K])."""
    x, rows, y, K = problems.check_one_problem(x, rows, labels, n_classes)
    Xa = np.hstack([x[rows].astype(np.float64), np.ones((rows.size, 1))])
    W = np.hstack([np.asarray(coef, dtype=np.float64).reshape(K, Xa.shape[1] - 1), np.asarray(intercept, dtype=np.float64).reshape(K, 1)])
    out = [_value_violation(Xa, s, float(C), w) for s, w in zip(_signs(y, K), W)]
    return np.asarray([o[0] for o in out]), np.asarray([o[1] for o in out])


def lipschitz(Xa, C):
    """STEP_SAFETY * C / 4 * lambda_max(Xa^T Xa), lambda_max by POWER_ITERATIONS steps from the constant vector."""
    v = np.full(Xa.shape[1], 1.0 / np.sqrt(Xa.shape[1]))
    lam = 1.0
    for _ in range(POWER_ITERATIONS):
        v = Xa.T @ (Xa @ v)
        lam = np.linalg.norm(v)
        v /= lam
    return STEP_SAFETY * 0.25 * C * lam


def _solve(Xa, s, C, L, vtol, max_iter, w):
    """FISTA with gradient restart from w until the violation (looked at every CHECK_EVERY iterations) is at most vtol."""
    y, t, n_iter = w.copy(), 1.0, 0
    f, viol = _value_violation(Xa, s, C, w)
    while viol > vtol and n_iter < max_iter:
        for _ in range(CHECK_EVERY):
            g = C * (Xa.T @ (-s * np.exp(-np.logaddexp(0.0, s * (Xa @ y)))))
            u = y - g / L
            wn = np.sign(u) * np.maximum(np.abs(u) - 1.0 / L, 0.0)
            if (y - wn) @ (wn - w) > 0.0:
                t, y = 1.0, wn.copy()
            else:
                tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
                y = wn + ((t - 1.0) / tn) * (wn - w)
                t = tn
            w = wn
        n_iter += CHECK_EVERY
        f, viol = _value_violation(Xa, s, C, w)
    return w, f, viol, n_iter


def lr_l1_host(x, rows, labels, n_classes, C=1.0, vtol=1e-8, max_iter=400000):
    """One problem (its K one-vs-rest problems) solved in float64 until the violation is at most vtol; raises if it stops above.  K = 2 is
    solved once (class 1) and mirrored; a class with no sample or with every sample starts from its closed form, which ends it at once
    wherever that point is optimal.
    -> LrL1Host(coef float64 [K, dim], intercept [K], f [K], violation [K], n_iter [K])."""
    x, rows, y, K = problems.check_one_problem(x, rows, labels, n_classes)
    C = float(C)
    n = rows.size
    Xa = np.hstack([x[rows].astype(np.float64), np.ones((n, 1))])
    L = lipschitz(Xa, C)
    W, f, viol, n_iter = np.zeros((K, Xa.shape[1])), np.zeros(K), np.zeros(K), np.zeros(K, np.int64)
    S = _signs(y, K)
    for k in range(1 if K == 2 else 0, K):
        w0 = np.zeros(Xa.shape[1])
        if abs(S[k].sum()) == n and C * n > 1.0:
            w0[-1] = np.sign(S[k][0]) * np.log(C * n - 1.0)
        W[k], f[k], viol[k], n_iter[k] = _solve(Xa, S[k], C, L, float(vtol), int(max_iter), w0)
        if not viol[k] <= vtol:
            raise RuntimeError(f"lr_l1_host stopped at violation {viol[k]:.3e} above {vtol:.1e} after {n_iter[k]} iterations (class {k})")
    if K == 2:
        W[0] = np.where(W[1] == 0.0, 0.0, -W[1])
        f[0], viol[0], n_iter[0] = f[1], viol[1], n_iter[1]
    return LrL1Host(W[:, :-1].copy(), W[:, -1].copy(), f, viol, n_iter)


def check_problems(rows, labels, offsets, n_rows, dim, n_classes, C=1.0):
    """The refusals of fit_on_device, made before anything is uploaded: problems.check_problems under logreg's caps."""
    return problems.check_problems(rows, labels, offsets, n_rows, dim, n_classes, C, MAX_ROWS, MAX_CLASSES, MAX_DIM)


def fit_on_device(x, rows, labels, offsets, n_classes, C=1.0, max_iter=None, vtol=1e-3):
    """x: CUDA tensor or numpy array [bank rows, dim] float32; the lists and C as logreg.fit_on_device takes them.
    -> LrL1Fit(coef float32 [P, K, dim] (a weight the solver holds at zero is exactly 0.0), intercept float32 [P, K], info int32 [P, K, 4] =
    {status, n_iter, stop reason, non-zero weights among the dim (the bias is not counted)} per class, stats float64 [P, K, 2] = {f_k,
    violation} from logits formed afresh from the returned weights, d_coef / d_intercept = the two still on the device, as
    logreg.score_on_device takes them).  status 0 fitted, 2 = empty problem, label or row out of range (all K entries say so and nothing
    else is written for the problem); stop reason 0 = violation <= vtol, 1 = max_iter (sklearn's ConvergenceWarning, not an error).
    max_iter None = MAX_ITER.  One upload (lists, offsets, C), one launch, one copy back."""
    import torch
    n_rows, dim = problems.bank_shape(x)
    K = int(n_classes)
    rows, labels, off, Cs = check_problems(rows, labels, offsets, n_rows, dim, K, C)
    max_iter = MAX_ITER if max_iter is None else int(max_iter)
    if max_iter < 1 or not float(vtol) >= 0:
        raise ValueError("max_iter must be at least 1 and vtol non-negative")
    P = off.size - 1
    x = problems.device_bank(x)
    dev = x.device
    with torch.cuda.device(dev):
        d_in, (p_C, p_off, p_rows, p_labels) = _lib.upload_words([Cs, off, rows, labels], dev)
        out = _lib.OutputWords([("stats", np.float64, (P, K, 2)), ("coef", np.float32, (P, K, dim)), ("intercept", np.float32, (P, K)),
                                ("info", np.int32, (P, K, 4))], dev)
        if P:
            L = _lib.lib()
            n_work = int(L.mkws_lr_l1_work_floats(dim, P, K))
            d_work = torch.empty(n_work, dtype=torch.float32, device=dev)
            _lib.check(L.mkws_lr_l1_fit(x.data_ptr(), n_rows, dim, p_rows, p_labels, p_off, P, K, p_C, max_iter, float(vtol), out.ptr("coef"),
                                        out.ptr("intercept"), out.ptr("info"), out.ptr("stats"), problems.ptr_or_none(d_work), n_work,
                                        _lib.current_stream_ptr()))
        out.fetch()                                                    # the call's one synchronisation
    return LrL1Fit(out.host("coef"), out.host("intercept"), out.host("info"), out.host("stats"), out.device("coef"), out.device("intercept"))
