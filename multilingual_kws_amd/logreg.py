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

from . import _lib

MAX_ROWS = 1024               # MKWS_LOGREG_MAX_ROWS: rows of one problem
MAX_CLASSES = 8               # MKWS_LOGREG_MAX_CLASSES
MAX_DIM = 1024                # MKWS_LOGREG_MAX_DIM

LogregHost = namedtuple("LogregHost", "coef intercept f gnorm n_iter")
LogregFit = namedtuple("LogregFit", "coef intercept info stats d_coef d_intercept")


def kappa(n_classes):
    return 2.0 if int(n_classes) == 2 else 1.0


def _scaler(X, standardize):
    """(mu, sigma) of StandardScaler over the rows of X (float64), or (0, 1)."""
    if not standardize:
        return np.zeros(X.shape[1]), np.ones(X.shape[1])
    mu = X.mean(axis=0)
    sigma = np.sqrt(((X - mu) ** 2).mean(axis=0))
    sigma[sigma == 0.0] = 1.0
    return mu, sigma


def _problem(x, rows, labels, n_classes, standardize):
    K = int(n_classes)
    rows, y = np.asarray(rows, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    x = np.asarray(x)
    if x.ndim != 2 or rows.ndim != 1 or rows.shape != y.shape or rows.size == 0:
        raise ValueError("x must be [rows, dim]; rows and labels one non-empty list each, of equal length")
    if K < 2 or y.min() < 0 or y.max() >= K or rows.min() < 0 or rows.max() >= x.shape[0]:
        raise ValueError("n_classes below 2, a label outside [0, n_classes) or a row outside the bank")
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
    """The refusals of fit_on_device / score_on_device, made before anything is uploaded -> (rows int32, labels int32, offsets int32,
    C float64 [P]).  Refused: n_classes outside [2, MAX_CLASSES], dim outside [1, MAX_DIM], lists of unequal length, offsets that are not
    P + 1 non-decreasing integers inside [0, len(rows)], a problem of more than MAX_ROWS rows, a C that is not positive and finite or not
    one per problem.  What the lists hold is the device's to check: an empty problem, a label outside [0, n_classes) or a row outside the
    bank gives that problem status 2."""
    K = int(n_classes)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"n_classes {K} outside [2, {MAX_CLASSES}]")
    if not 1 <= int(dim) <= MAX_DIM:
        raise ValueError(f"dim {int(dim)} outside [1, {MAX_DIM}]")
    if int(n_rows) < 0:
        raise ValueError("a bank of fewer than 0 rows")
    rows, labels, off = np.asarray(rows), np.asarray(labels), np.asarray(offsets)
    if rows.size == 0:
        rows = rows.astype(np.int32)
    if labels.size == 0:
        labels = labels.astype(np.int32)
    for name, a in (("rows", rows), ("labels", labels)):
        if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must be one flat list of integers")
    if rows.shape != labels.shape:
        raise ValueError(f"{rows.size} rows for {labels.size} labels")
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("offsets must be a list of P + 1 integers")
    off = off.astype(np.int64)
    if off[0] < 0 or off[-1] > rows.size or (np.diff(off) < 0).any():
        raise ValueError(f"offsets must be non-decreasing and inside [0, {rows.size}]")
    sizes = np.diff(off)
    for p in np.nonzero(sizes > MAX_ROWS)[0][:1]:
        raise ValueError(f"problem {int(p)} has {int(sizes[p])} rows: at most {MAX_ROWS}")
    P = off.size - 1
    Cs = np.full(P, float(C)) if np.ndim(C) == 0 else np.asarray(C, dtype=np.float64).reshape(-1)
    if Cs.size != P:
        raise ValueError(f"{Cs.size} values of C for {P} problems")
    if not (np.isfinite(Cs).all() and (Cs > 0).all()):
        raise ValueError("C must be positive and finite")
    clip = lambda a: np.clip(a, -2 ** 31, 2 ** 31 - 1).astype(np.int32)      # (an index out of int32 stays out of every bank)
    return clip(rows), clip(labels), off.astype(np.int32), Cs.astype(np.float64)


def _bank(x):
    """numpy float32 [rows, dim] is uploaded; a CUDA tensor is taken as it is."""
    import torch
    if not torch.is_tensor(x):
        x = np.ascontiguousarray(x)
        x = torch.from_numpy(x if x.flags.writeable else x.copy()).cuda()
    if not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("x must be a CUDA tensor or numpy array [rows, dim] of float32")
    return x.contiguous()


def _check_bank(x):
    import torch
    if not torch.is_tensor(x):
        x = np.asarray(x)
        if x.dtype != np.float32:
            raise ValueError("x must be float32")
    if x.ndim != 2:
        raise ValueError("x must be [rows, dim]")
    return x, int(x.shape[0]), int(x.shape[1])


def fit_on_device(x, rows, labels, offsets, n_classes, C=1.0, standardize=False, max_iter=300, gtol=1e-5):
    """x: CUDA tensor or numpy array [bank rows, dim] float32; problem p trains on bank rows rows[offsets[p] : offsets[p + 1]] with
    labels[...] in [0, n_classes) (rows may repeat inside and across problems: nothing is copied); C: one strength or one per problem.
    -> LogregFit(coef float32 [P, K, dim], intercept float32 [P, K] (raw space), info int32 [P, 4] = {status, n_iter, stop reason, rows},
    stats float64 [P, 2] = {objective, |grad|_inf} as the device last saw them, d_coef / d_intercept = the two still on the device).
    status 0 fitted, 2 = empty problem, label or row out of range (nothing else written for it); stop reason 0 = |grad|_inf <= gtol,
    1 = max_iter (sklearn's ConvergenceWarning, not an error).  One upload (lists, offsets, C), one launch, one copy back.  What
    check_problems refuses is refused before anything is uploaded."""
    import torch
    x, n_rows, dim = _check_bank(x)
    K = int(n_classes)
    rows, labels, off, Cs = check_problems(rows, labels, offsets, n_rows, dim, K, C)
    if int(max_iter) < 1 or not float(gtol) >= 0:
        raise ValueError("max_iter must be at least 1 and gtol non-negative")
    P = off.size - 1
    x = _bank(x)
    dev = x.device
    with torch.cuda.device(dev):
        d_in, (p_C, p_off, p_rows, p_labels) = _lib.upload_words([Cs, off, rows, labels], dev)
        # every output in ONE buffer of 4-byte words, so that they cross in one copy: stats (float64, first: 8-byte aligned), coef,
        # intercept, info
        at = np.cumsum([0, 4 * P, P * K * dim, P * K, 4 * P])
        d_out = torch.zeros(int(at[-1]), dtype=torch.int32, device=dev)
        ptr = [d_out.data_ptr() + 4 * int(a) for a in at]
        if P:
            L = _lib.lib()
            n_work = int(L.mkws_logreg_work_floats(dim, P, K))
            d_work = torch.empty(n_work, dtype=torch.float32, device=dev)
            _lib.check(L.mkws_logreg_fit(x.data_ptr(), n_rows, dim, p_rows, p_labels, p_off, P, K, p_C, int(bool(standardize)), int(max_iter),
                                         float(gtol), ptr[1], ptr[2], ptr[3], ptr[0], d_work.data_ptr(), n_work, _lib.current_stream_ptr()))
        out = d_out.cpu().numpy()                                      # the call's one synchronisation
    d_coef = d_out[int(at[1]):int(at[2])].view(torch.float32).view(P, K, dim)
    d_intercept = d_out[int(at[2]):int(at[3])].view(torch.float32).view(P, K)
    return LogregFit(out[at[1]:at[2]].view(np.float32).reshape(P, K, dim), out[at[2]:at[3]].view(np.float32).reshape(P, K),
                     out[at[3]:at[4]].reshape(P, 4), out[at[0]:at[1]].view(np.float64).reshape(P, 2), d_coef, d_intercept)


def score_on_device(x, rows, true, offsets, coef, intercept, want_probs=False, want_logits=False):
    """x: CUDA tensor [bank rows, dim] float32; problem p is scored on ITS list rows[offsets[p] : offsets[p + 1]] against true[...];
    coef CUDA [P, K, dim], intercept CUDA [P, K] (what fit_on_device left on the device).  rows / true / offsets: CUDA int32 tensors or
    host lists (uploaded non-blocking).
    -> (pred int32 [total] = first argmax of the float32 logits, correct int32 [P] = rows with pred == true, probs float32 [total, K] or
    None, logits float32 [total, K] or None), CUDA tensors.  Asynchronous: nothing is copied back and nothing waits.  A row outside the
    bank gets pred -1 (probs and logits NaN) and is never correct."""
    import torch
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        raise ValueError("x must be a CUDA tensor [rows, dim] of float32")
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
    lists = []
    for name, a in (("rows", rows), ("true", true), ("offsets", offsets)):
        if not torch.is_tensor(a):
            a = np.asarray(a)
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"{name} must hold integers")
            a = torch.from_numpy(np.ascontiguousarray(np.clip(a, -2 ** 31, 2 ** 31 - 1), dtype=np.int32).reshape(-1)).to(dev, non_blocking=True)
        if a.dtype != torch.int32 or a.dim() != 1 or a.device != dev:
            raise ValueError(f"{name} must be a flat int32 list on the device of x")
        lists.append(a.contiguous())
    d_rows, d_true, d_off = lists
    total = int(d_rows.numel())
    if d_true.numel() != total or d_off.numel() != P + 1:
        raise ValueError(f"{total} rows, {int(d_true.numel())} labels, {int(d_off.numel())} offsets for {P} problems")
    x, coef, intercept = x.contiguous(), coef.contiguous(), intercept.contiguous()
    with torch.cuda.device(dev):
        pred = torch.empty(total, dtype=torch.int32, device=dev)
        correct = torch.empty(P, dtype=torch.int32, device=dev)
        probs = torch.empty((total, K), dtype=torch.float32, device=dev) if want_probs else None
        logits = torch.empty((total, K), dtype=torch.float32, device=dev) if want_logits else None
        _lib.check(_lib.lib().mkws_logreg_score(x.data_ptr(), n_rows, dim, d_rows.data_ptr() if total else None, d_true.data_ptr() if total else None,
                                                d_off.data_ptr(), P, K, coef.data_ptr() if P else None, intercept.data_ptr() if P else None,
                                                total, pred.data_ptr() if total else None, probs.data_ptr() if want_probs and total else None,
                                                logits.data_ptr() if want_logits and total else None, correct.data_ptr() if P else None,
                                                _lib.current_stream_ptr()))
    return pred, correct, probs, logits
