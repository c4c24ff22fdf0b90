"""K logistic regressions on embeddings: the specification (objective, logreg_host, predict_host) and the host wrappers over
mkws_logreg_fit / mkws_logreg_score (include/mkws.h).

What the DataPerf selection harness of the reference does with the exported embedding vectors (notebooks/dataperf_experiments.py:121-192,
notebooks/dataperf_test_harness.py:242-256,318-408) is sklearn.linear_model.LogisticRegression on 100 to 600 rows of 1024 features, once
per split.  For problem p with rows R_p, labels y, strength C_p and n_classes = K the objective is

    f_p(W, b) = C_p * sum_{i in R_p} [ logsumexp_k(z_ik) - z_{i,y_i} ] + (kappa / 2) * sum W^2,      z_i = W x~_i + b

with W [K, dim], b [K] unpenalised, kappa = 1 for K >= 3 (sklearn's multinomial objective) and kappa = 2 for K = 2: only then does the
two-row softmax solution reproduce sklearn's binary one (coef_ = W[1] - W[0], intercept_ = b[1] - b[0]).  b is fixed only up to a
constant; a gradient method started at zero keeps sum_k b_k = 0 and the solutions are returned that way: compare probabilities and
objectives, never b.  Every one of the K rows is fitted even when a class has no sample (the objective is still strictly convex in W);
this module follows the objective, not sklearn's class discovery.  standardize=True: x~ = (x - mu_p) / sigma_p over the problem's own
rows (ddof 0, sigma = 0 -> 1, as StandardScaler); the problem is solved and penalised in the scaled space, as in the reference's Pipeline,
and returned in raw space, W = W~ / sigma, b = b~ - W~ . (mu / sigma), so that scoring needs no scaler.

The problem is strictly convex in W, so the optimum is what a solver is held to: sklearn's own default run (lbfgs, tol 1e-4, max_iter
100) stops well above it, and tests/test_logreg_gpu.py asks the device to be at least as close to the optimum as sklearn is.
Host part: pure NumPy float64 on widened float32 inputs; neither scipy nor sklearn is imported."""
from collections import namedtuple

import numpy as np

from . import _lib, problems

MAX_ROWS = 1024               # MKWS_LOGREG_MAX_ROWS: rows of one problem
MAX_CLASSES = 8               # MKWS_LOGREG_MAX_CLASSES
MAX_DIM = 1024                # MKWS_LOGREG_MAX_DIM

LogregHost = namedtuple("LogregHost", "coef intercept f gnorm n_iter")
LogregFit = namedtuple("LogregFit", "coef intercept info stats d_coef d_intercept")


def kappa(n_classes):
    return 2.0 if int(n_classes) == 2 else 1.0


def _scaler(X, standardize):
    """(mu, sigma) of StandardScaler over the rows of X (float64), or (0, 1)."""
    return problems.standard_scaler(X) if standardize else (np.zeros(X.shape[1]), np.ones(X.shape[1]))


def _problem(x, rows, labels, n_classes, standardize):
    x, rows, y, _ = problems.check_one_problem(x, rows, labels, n_classes)
    X = x[rows].astype(np.float64)
    mu, sigma = _scaler(X, standardize)
    return (X - mu) / sigma, y, mu, sigma


def _value_grad(Xs, y, K, C, W, b):
    Z = Xs @ W.T + b
    m = Z.max(axis=1, keepdims=True)
    E = np.exp(Z - m)
    S = E.sum(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(S[:, 0])
    P = E / S
    f = C * (lse - Z[np.arange(len(y)), y]).sum() + 0.5 * kappa(K) * (W * W).sum()
    R = P.copy()
    R[np.arange(len(y)), y] -= 1.0
    return f, C * (R.T @ Xs) + kappa(K) * W, C * R.sum(axis=0), P


def objective(x, rows, labels, n_classes, C, coef, intercept, standardize=False):
    """-> (f, grad) in float64 at raw-space (coef [K, dim], intercept [K]), as fit_on_device and logreg_host return them.  With
    standardize the point is first taken to the scaled space (W~ = W * sigma, b~ = b + W . mu), where the problem is posed: f and
    grad = concatenate(df/dW~ .ravel(), df/db~) are the scaled problem's."""
    K = int(n_classes)
    Xs, y, mu, sigma = _problem(x, rows, labels, K, standardize)
    W = np.asarray(coef, dtype=np.float64).reshape(K, Xs.shape[1])
    b = np.asarray(intercept, dtype=np.float64).reshape(K)
    f, gW, gb, _ = _value_grad(Xs, y, K, float(C), W * sigma, b + W @ mu)
    return float(f), np.concatenate([gW.ravel(), gb])


def logreg_host(x, rows, labels, n_classes, C=1.0, standardize=False, gtol=1e-10, max_newton=200):
    """One problem solved in float64 until |grad|_inf <= gtol (1e-10: with a class that has no sample the infimum is approached as its
    intercept falls, and f is within about gtol of it): Newton steps whose linear systems are solved by conjugate gradients on
    Hessian-vector products (the Hessian is never formed), with a backtracking line search.
    -> LogregHost(coef float64 [K, dim] and intercept [K] in raw space with sum(intercept~) = 0 in the solved space, f, gnorm, n_iter)."""
    K, C = int(n_classes), float(C)
    Xs, y, mu, sigma = _problem(x, rows, labels, K, standardize)
    n, dim = Xs.shape
    kap = kappa(K)
    W, b = np.zeros((K, dim)), np.zeros(K)
    f, gW, gb, P = _value_grad(Xs, y, K, C, W, b)
    n_iter = 0
    for n_iter in range(int(max_newton) + 1):
        gnorm = max(np.abs(gW).max(), np.abs(gb).max())
        if gnorm <= gtol or n_iter == max_newton:
            break

        def hess(vW, vb):
            A = Xs @ vW.T + vb
            A = P * (A - (P * A).sum(axis=1, keepdims=True))
            return C * (A.T @ Xs) + kap * vW, C * A.sum(axis=0)

        # H d = -g by conjugate gradients.  H is singular only along a constant added to b, and g has no component there
        dW, db = np.zeros_like(W), np.zeros_like(b)
        rW, rb = -gW, -gb
        pW, pb = rW.copy(), rb.copy()
        rr = (rW * rW).sum() + (rb * rb).sum()
        stop = rr * 1e-20
        for _ in range(4 * (min(n, dim + 1) * K + K) + 50):
            hW, hb = hess(pW, pb)
            curv = (pW * hW).sum() + (pb * hb).sum()
            if curv <= 0.0:
                break
            a = rr / curv
            dW += a * pW
            db += a * pb
            rW -= a * hW
            rb -= a * hb
            rb -= rb.mean()                                          # (rounding must not feed the singular direction)
            rr_new = (rW * rW).sum() + (rb * rb).sum()
            if rr_new <= stop:
                break
            pW = rW + (rr_new / rr) * pW
            pb = rb + (rr_new / rr) * pb
            rr = rr_new
        slope = (gW * dW).sum() + (gb * db).sum()
        t = 1.0
        for _ in range(60):
            f_new, gW_new, gb_new, P_new = _value_grad(Xs, y, K, C, W + t * dW, b + t * db)
            if f_new <= f + 1e-4 * t * slope or t < 1e-12:
                break
            t *= 0.5
        # at the rounding floor of f the Armijo test is noise: there the full step is taken as long as it shrinks the gradient
        if t < 1.0:
            f_one, gW_one, gb_one, P_one = _value_grad(Xs, y, K, C, W + dW, b + db)
            if max(np.abs(gW_one).max(), np.abs(gb_one).max()) < gnorm and f_one <= f + 1e-9 * max(1.0, abs(f)):
                t, f_new, gW_new, gb_new, P_new = 1.0, f_one, gW_one, gb_one, P_one
        W, b = W + t * dW, b + t * db
        f, gW, gb, P = f_new, gW_new, gb_new, P_new
    b = b - b.mean()
    f, gW, gb, _ = _value_grad(Xs, y, K, C, W, b)
    gnorm = max(np.abs(gW).max(), np.abs(gb).max())
    if gnorm > gtol:
        raise RuntimeError(f"logreg_host stopped at |grad|_inf = {gnorm:.3e} above {gtol:.1e} after {n_iter} Newton steps")
    coef = W / sigma
    return LogregHost(coef, b - coef @ mu, float(f), float(gnorm), int(n_iter))


def predict_host(x, rows, coef, intercept):
    """-> (pred int32 = first argmax of the float64 logits, probs float64 [len(rows), K]) of bank rows `rows` under raw-space
    (coef, intercept): the expression mkws_logreg_score evaluates in float32."""
    rows = np.asarray(rows, dtype=np.int64)
    W, b = np.asarray(coef).astype(np.float64), np.asarray(intercept).astype(np.float64)
    Z = np.asarray(x)[rows].astype(np.float64) @ W.T + b
    E = np.exp(Z - Z.max(axis=1, keepdims=True)) if len(rows) else Z
    return Z.argmax(axis=1).astype(np.int32) if len(rows) else np.zeros(0, np.int32), E / E.sum(axis=1, keepdims=True) if len(rows) else E


def check_problems(rows, labels, offsets, n_rows, dim, n_classes, C=1.0):
    """The refusals of fit_on_device, made before anything is uploaded: problems.check_problems under this module's caps.  What the lists
    hold is the device's to check: an empty problem, a label outside [0, n_classes) or a row outside the bank gives that problem status 2."""
    return problems.check_problems(rows, labels, offsets, n_rows, dim, n_classes, C, MAX_ROWS, MAX_CLASSES, MAX_DIM)


def fit_on_device(x, rows, labels, offsets, n_classes, C=1.0, standardize=False, max_iter=300, gtol=1e-5):
    """x: CUDA tensor or numpy array [bank rows, dim] float32; problem p trains on bank rows rows[offsets[p] : offsets[p + 1]] with
    labels[...] in [0, n_classes) (rows may repeat inside and across problems: nothing is copied); C: one strength or one per problem.
    -> LogregFit(coef float32 [P, K, dim], intercept float32 [P, K] (raw space), info int32 [P, 4] = {status, n_iter, stop reason, rows},
    stats float64 [P, 2] = {objective, |grad|_inf} as the device last saw them, d_coef / d_intercept = the two still on the device).
    status 0 fitted, 2 = empty problem, label or row out of range (nothing else written for it); stop reason 0 = |grad|_inf <= gtol,
    1 = max_iter (sklearn's ConvergenceWarning, not an error).  One upload (lists, offsets, C), one launch, one copy back.  What
    check_problems refuses is refused before anything is uploaded."""
    import torch
    n_rows, dim = problems.bank_shape(x)
    K = int(n_classes)
    rows, labels, off, Cs = check_problems(rows, labels, offsets, n_rows, dim, K, C)
    if int(max_iter) < 1 or not float(gtol) >= 0:
        raise ValueError("max_iter must be at least 1 and gtol non-negative")
    P = off.size - 1
    x = problems.device_bank(x)
    dev = x.device
    with torch.cuda.device(dev):
        d_in, (p_C, p_off, p_rows, p_labels) = _lib.upload_words([Cs, off, rows, labels], dev)
        out = _lib.OutputWords([("stats", np.float64, (P, 2)), ("coef", np.float32, (P, K, dim)), ("intercept", np.float32, (P, K)),
                                ("info", np.int32, (P, 4))], dev)
        if P:
            L = _lib.lib()
            n_work = int(L.mkws_logreg_work_floats(dim, P, K))
            d_work = torch.empty(n_work, dtype=torch.float32, device=dev)
            _lib.check(L.mkws_logreg_fit(x.data_ptr(), n_rows, dim, p_rows, p_labels, p_off, P, K, p_C, int(bool(standardize)), int(max_iter),
                                         float(gtol), out.ptr("coef"), out.ptr("intercept"), out.ptr("info"), out.ptr("stats"), d_work.data_ptr(),
                                         n_work, _lib.current_stream_ptr()))
        out.fetch()                                                    # the call's one synchronisation
    return LogregFit(out.host("coef"), out.host("intercept"), out.host("info"), out.host("stats"), out.device("coef"), out.device("intercept"))


def score_on_device(x, rows, true, offsets, coef, intercept, want_probs=False, want_logits=False):
    """x: CUDA tensor [bank rows, dim] float32; problem p is scored on ITS list rows[offsets[p] : offsets[p + 1]] against true[...];
    coef CUDA [P, K, dim], intercept CUDA [P, K] (what fit_on_device left on the device).  rows / true / offsets: CUDA int32 tensors or
    host lists (uploaded non-blocking).
    -> (pred int32 [total] = first argmax of the float32 logits, correct int32 [P] = rows with pred == true, probs float32 [total, K] or
    None, logits float32 [total, K] or None), CUDA tensors.  Asynchronous: nothing is copied back and nothing waits.  A row outside the
    bank gets pred -1 (probs and logits NaN) and is never correct."""
    import torch
    x = problems.device_bank(x, upload=False)
    if not (torch.is_tensor(coef) and coef.is_cuda and coef.dtype == torch.float32 and coef.dim() == 3):
        raise ValueError("coef must be a CUDA tensor [problems, classes, dim] of float32")
    n_rows, dim = (int(v) for v in x.shape)
    P, K = int(coef.shape[0]), int(coef.shape[1])
    if int(coef.shape[2]) != dim:
        raise ValueError(f"coef of {int(coef.shape[2])} columns for rows of {dim}")
    if not (torch.is_tensor(intercept) and intercept.is_cuda and intercept.dtype == torch.float32 and tuple(intercept.shape) == (P, K)):
        raise ValueError("intercept must be a CUDA tensor [problems, classes] of float32")
    if not 2 <= K <= MAX_CLASSES or not 1 <= dim <= MAX_DIM:
        raise ValueError(f"n_classes {K} outside [2, {MAX_CLASSES}] or dim {dim} outside [1, {MAX_DIM}]")
    dev = x.device
    if coef.device != dev or intercept.device != dev:
        raise ValueError(f"coef and intercept must live on the device of x ({dev}), not {coef.device} / {intercept.device}")
    d_rows, d_true, d_off = (problems.device_int_list(a, name, dev) for name, a in (("rows", rows), ("true", true), ("offsets", offsets)))
    total = int(d_rows.numel())
    if d_true.numel() != total or d_off.numel() != P + 1:
        raise ValueError(f"{total} rows, {int(d_true.numel())} labels, {int(d_off.numel())} offsets for {P} problems")
    coef, intercept = coef.contiguous(), intercept.contiguous()
    ptr = problems.ptr_or_none
    with torch.cuda.device(dev):
        pred = torch.empty(total, dtype=torch.int32, device=dev)
        correct = torch.empty(P, dtype=torch.int32, device=dev)
        probs = torch.empty((total, K), dtype=torch.float32, device=dev) if want_probs else None
        logits = torch.empty((total, K), dtype=torch.float32, device=dev) if want_logits else None
        _lib.check(_lib.lib().mkws_logreg_score(x.data_ptr(), n_rows, dim, ptr(d_rows), ptr(d_true), d_off.data_ptr(), P, K, ptr(coef), ptr(intercept),
                                                total, ptr(pred), ptr(probs), ptr(logits), ptr(correct), _lib.current_stream_ptr()))
    return pred, correct, probs, logits
