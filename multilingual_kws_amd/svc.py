"""K RBF support-vector classifiers on embeddings: the specification (svc_host, decision_host, predict_host) and the host wrappers over
mkws_svc_prepare / mkws_svc_kernel / mkws_svc_fit / mkws_svc_score (include/mkws.h).

What the DataPerf selection harness of the reference does with sklearn.svm.SVC() (notebooks/dataperf_test_harness.py:224-239:
`simplest_svm`, `svm_with_scaling`): C-SVC with the RBF kernel and gamma="scale", one-vs-one over the classes.  For problem p with rows
R_p into the bank x, labels in [0, K), C, standardize and gamma:

  scaling   x~ = (x - mu) * inv: mu is ALWAYS the column mean of the problem's own rows (the kernel is translation invariant, and distances
            formed from centred rows cancel against the spread, not against the common offset of these non-negative vectors); inv = 1 / sigma
            with standardize (ddof 0, sigma = 0 -> 1, as StandardScaler), ones without.
  gamma     gamma itself where gamma > 0, otherwise sklearn's "scale": 1 / (dim * Var), Var the variance of all n * dim entries of the matrix
            the kernel sees (x[R_p] raw, or the standardised matrix) in float64; 1 where that variance is 0.
  kernel    k(a, b) = exp(-gamma * |a~ - b~|^2).
  pairs     for present classes i < j (class i is +1):  min 1/2 a'Qa - e'a,  0 <= a <= C,  y'a = 0,  Q_st = y_s y_t k(x_s, x_t);
            c_t = a_t y_t,  f_ij(x) = sum_t c_t k(x_t, x) - rho_ij;  rho by libsvm's rule: the mean of y_t G_t (G = Qa - e) over the free t,
            the midpoint of the two bounds where none is free.
  solver    SMO with libsvm's second-order working-set selection (the later index on ties), its clipping and its TAU = 1e-12 guard, without
            shrinking, until m(a) - M(a) < tol.
  predict   f_ij > 0 votes i, otherwise j; most votes wins, the lowest class on ties.  A class with no row is never predicted: its pairs
            carry zero coefficients, rho = 0 and no vote.  Fewer than two present classes is refused.

Coefficients are kept in libsvm's dual_coef_ layout turned on its side and aligned with the row list: coef[t, m] is row t's c_t in the
machine against the m-th OTHER class in ascending order (m = o for o < label, o - 1 above), zero where it is no support vector.  Decision
values are in the libsvm convention also for two classes, where sklearn's decision_function returns the negated value.

The dual is a convex QP and the decision function is unique even where a is not, so the float64 optimum (svc_host at tol 1e-10) is what
a solver is held to: sklearn's default run (tol 1e-3) stops 1e-4 from it, and tests/test_svc_gpu.py asks the device to be at least as
close.

probability=True, given the folds (cv_folds draws them; libsvm's own unseeded draw is the one thing not reproduced):
  cv        every entry's decision value under the pair's machine trained WITHOUT the entry's fold (cv_decision_host), centre, scale
            and gamma those of the whole problem;
  platt     per pair (A, B) minimising sum t z + log(1 + exp(-z)), z = A f + B, over those values (platt_host; Lin, Lin and Weng 2007);
  couple    r_ij = 1 / (1 + exp(A f_ij + B)) clipped to [1e-7, 1 - 1e-7], p = argmin sum_i sum_{j != i} (r_ji p_i - r_ij p_j)^2 on the
            simplex's plane (couple_host; Wu, Lin and Weng 2004, method 2), solved exactly instead of iterated to 0.005 / K.
Host part: pure NumPy float64 on widened float32 inputs; neither scipy nor sklearn is imported."""
from collections import namedtuple

import numpy as np

from . import _lib, problems
from .synth import splitmix64

MAX_ROWS = 1024               # MKWS_SVC_MAX_ROWS: rows of one problem
MAX_CLASSES = 8               # MKWS_SVC_MAX_CLASSES
MAX_DIM = 1024                # MKWS_SVC_MAX_DIM
TAU = 1e-12
WORK_BUDGET = 512 << 20       # bytes of Gram workspace one fit launch may ask for; a larger call is split into chunks of problems

SvcHost = namedtuple("SvcHost", "coef rho gamma centre inv_scale n_iter gap")
SvcProbaHost = namedtuple("SvcProbaHost", SvcHost._fields + ("probA", "probB", "cv_decision"))
SvcFit = namedtuple("SvcFit", "coef rho gamma centre inv_scale info gap d_coef d_rho d_gamma d_centre d_inv_scale d_info")
SvcProbaFit = namedtuple("SvcProbaFit", "coef rho gamma centre inv_scale info probA probB cv_decision cv_info present gap d_coef d_rho d_gamma d_centre "
                                        "d_inv_scale d_info d_probA d_probB d_cv_decision d_cv_info d_present")


def pairs(n_classes):
    """[(i, j)] in the order of rho and of the decision values: (0, 1), (0, 2), ..."""
    K = int(n_classes)
    return [(i, j) for i in range(K) for j in range(i + 1, K)]


def _slot(own, other):
    return other if other < own else other - 1


def scaling(x, rows, standardize=False, gamma=0.0):
    """-> (centre float64 [dim], inv_scale float64 [dim], gamma float64) of one problem, as the module docstring defines them."""
    X = np.asarray(x)[np.asarray(rows, dtype=np.int64)].astype(np.float64)
    mu, sigma = problems.standard_scaler(X)
    inv = 1.0 / sigma if standardize else np.ones(X.shape[1])
    if float(gamma) > 0.0:
        return mu, inv, float(gamma)
    seen = (X - mu) * inv if standardize else X
    var = float(((seen - seen.mean()) ** 2).mean())
    return mu, inv, 1.0 / (X.shape[1] * var) if var > 0.0 else 1.0


def kernel_host(x, rows_a, rows_b, centre, inv_scale, gamma):
    """float64 [len(rows_a), len(rows_b)]: exp(-gamma * |a~ - b~|^2) of bank rows under (centre, inv_scale, gamma), the distances formed
    from the centred and scaled rows."""
    x = np.asarray(x)
    c, s = np.asarray(centre, dtype=np.float64), np.asarray(inv_scale, dtype=np.float64)
    A = (x[np.asarray(rows_a, dtype=np.int64)].astype(np.float64) - c) * s
    B = (x[np.asarray(rows_b, dtype=np.int64)].astype(np.float64) - c) * s
    d2 = (A * A).sum(axis=1)[:, None] + (B * B).sum(axis=1)[None, :] - 2.0 * (A @ B.T)
    return np.exp(-float(gamma) * np.maximum(d2, 0.0))


def smo(Kp, y, C, tol, max_iter):
    """libsvm's Solver (no shrinking) on one pair: Kp float64 [m, m] kernel values, y in {+1, -1}.
    -> (alpha, G, rho, iterations, final gap m(a) - M(a), cut at max_iter)."""
    m = len(y)
    y = np.asarray(y, dtype=np.float64)
    alpha, G, QD = np.zeros(m), -np.ones(m), np.diag(Kp).copy()
    pos = y > 0
    it, gap, cut = 0, np.inf, False
    for it in range(int(max_iter) + 1):
        v = -y * G
        up = np.where(pos, alpha < C, alpha > 0.0)
        low = np.where(pos, alpha > 0.0, alpha < C)
        vi = np.where(up, v, -np.inf)
        i = m - 1 - int(np.argmax(vi[::-1]))
        gmax = vi[i]
        gap = gmax - np.where(low, v, np.inf).min()
        if gap < tol:
            break
        if it == max_iter:
            cut = True
            break
        gd = gmax - v
        quad = QD[i] + QD - 2.0 * Kp[i]
        quad = np.where(quad > 0.0, quad, TAU)
        obj = np.where(low & (gd > 0.0), -(gd * gd) / quad, np.inf)
        j = m - 1 - int(np.argmin(obj[::-1]))
        if not np.isfinite(obj[j]):
            break
        ai, aj = alpha[i], alpha[j]
        q = Kp[i, i] + Kp[j, j] - 2.0 * Kp[i, j]
        if q <= 0.0:
            q = TAU
        if y[i] != y[j]:
            delta = (-G[i] - G[j]) / q
            diff = ai - aj
            ni, nj = ai + delta, aj + delta
            if diff > 0.0:
                if nj < 0.0:
                    nj, ni = 0.0, diff
            elif ni < 0.0:
                ni, nj = 0.0, -diff
            if diff > 0.0:
                if ni > C:
                    ni, nj = C, C - diff
            elif nj > C:
                nj, ni = C, C + diff
        else:
            delta = (G[i] - G[j]) / q
            tot = ai + aj
            ni, nj = ai - delta, aj + delta
            if tot > C:
                if ni > C:
                    ni, nj = C, tot - C
            elif nj < 0.0:
                nj, ni = 0.0, tot
            if tot > C:
                if nj > C:
                    nj, ni = C, tot - C
            elif ni < 0.0:
                ni, nj = 0.0, tot
        G += y * (y[i] * Kp[i] * (ni - ai) + y[j] * Kp[j] * (nj - aj))
        alpha[i], alpha[j] = ni, nj
    yG = y * G
    upper, lower = alpha >= C, alpha <= 0.0
    free = ~upper & ~lower
    if free.any():
        rho = float(yG[free].mean())
    else:
        ub = np.where((upper & ~pos) | (lower & pos), yG, np.inf).min()
        lb = np.where((upper & pos) | (lower & ~pos), yG, -np.inf).max()
        rho = float((ub + lb) / 2.0)
    return alpha, G, rho, it, float(gap), cut


def _problem(x, rows, labels, n_classes):
    _, rows, y, K = problems.check_one_problem(x, rows, labels, n_classes)
    if len(np.unique(y)) < 2:
        raise ValueError("fewer than two classes have a row")
    return rows, y, K


def svc_host(x, rows, labels, n_classes, C=1.0, standardize=False, gamma=0.0, tol=1e-10, max_iter=10_000_000):
    """One problem in float64: every present pair's dual by SMO until its gap is below tol.
    -> SvcHost(coef float64 [len(rows), K - 1], rho float64 [K (K - 1) / 2], gamma, centre [dim], inv_scale [dim], n_iter = the largest
    iteration count of a pair, gap = the largest final gap)."""
    rows, y, K = _problem(x, rows, labels, n_classes)
    C = float(C)
    if not C > 0.0:
        raise ValueError("C must be positive")
    centre, inv, g = scaling(x, rows, standardize, gamma)
    Kall = kernel_host(x, rows, rows, centre, inv, g)
    coef, rho = np.zeros((len(rows), K - 1)), np.zeros(K * (K - 1) // 2)
    n_iter, worst = 0, 0.0
    for q, (i, j) in enumerate(pairs(K)):
        ti, tj = np.nonzero(y == i)[0], np.nonzero(y == j)[0]
        if not len(ti) or not len(tj):
            continue
        idx = np.concatenate([ti, tj])
        sign = np.concatenate([np.ones(len(ti)), -np.ones(len(tj))])
        alpha, _, r, it, gap, cut = smo(Kall[np.ix_(idx, idx)], sign, C, float(tol), max_iter)
        if cut:
            raise RuntimeError(f"svc_host: pair ({i}, {j}) stopped at a gap of {gap:.3e} above {tol:.1e} after {it} iterations")
        coef[ti, _slot(i, j)] = alpha[:len(ti)]
        coef[tj, _slot(j, i)] = -alpha[len(ti):]
        rho[q] = r
        n_iter, worst = max(n_iter, it), max(worst, gap)
    return SvcHost(coef, rho, g, centre, inv, n_iter, worst)


def decision_host(x, eval_rows, train_rows, train_labels, n_classes, coef, rho, gamma, centre, inv_scale):
    """float64 [len(eval_rows), K (K - 1) / 2]: f_ij of bank rows `eval_rows` under a model (its training rows and labels, coef
    [len(train_rows), K - 1], rho, gamma, centre, inv_scale), pairs in the order of pairs(K); 0 for a pair with an absent class.  The
    expression mkws_svc_score evaluates in float32."""
    K = int(n_classes)
    y = np.asarray(train_labels, dtype=np.int64)
    coef, rho = np.asarray(coef).astype(np.float64), np.asarray(rho).astype(np.float64)
    kv = kernel_host(x, train_rows, eval_rows, centre, inv_scale, gamma)                      # [train, eval]
    out = np.zeros((len(np.asarray(eval_rows)), K * (K - 1) // 2))
    for q, (i, j) in enumerate(pairs(K)):
        ti, tj = y == i, y == j
        if ti.any() and tj.any():
            out[:, q] = coef[ti, _slot(i, j)] @ kv[ti] + coef[tj, _slot(j, i)] @ kv[tj] - rho[q]
    return out


def predict_host(decision, train_labels, n_classes):
    """int32 [rows]: one-vs-one votes over the pairs of present classes (f_ij > 0 votes i, otherwise j), the lowest class on ties."""
    K = int(n_classes)
    present = np.bincount(np.asarray(train_labels, dtype=np.int64), minlength=K) > 0
    decision = np.asarray(decision)
    votes = np.zeros((decision.shape[0], K), np.int64)
    for q, (i, j) in enumerate(pairs(K)):
        if present[i] and present[j]:
            win = decision[:, q] > 0
            votes[:, i] += win
            votes[:, j] += ~win
    votes[:, ~present] = -1
    return votes.argmax(axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ probability=True, given the folds

MIN_FOLDS, MAX_FOLDS = 2, 16
R_CLIP = 1e-7                 # libsvm's min_prob: pairwise probabilities are clipped to [R_CLIP, 1 - R_CLIP] before they are coupled


def cv_folds(labels, offsets, n_folds=5, seed=0):
    """int32 [len(labels)]: the fold of every list entry.  Inside each problem p and class, the entries are ordered by
        key(seed, p, t) = splitmix64(splitmix64(splitmix64(seed + 0x9E3779B97F4A7C15) + p) + t)        (uint64, wrapping)
    with t the entry's position in the problem's list (synth.splitmix64; equal keys keep list order), and dealt folds 0, 1, ..., F - 1,
    0, ... in that order.  Stratified, which libsvm's draw is not: a class's folds differ in size by at most one, a pair's held-out sets
    by at most two."""
    y = np.asarray(labels, dtype=np.int64).reshape(-1)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    F = int(n_folds)
    if not MIN_FOLDS <= F <= MAX_FOLDS:
        raise ValueError(f"n_folds {F} outside [{MIN_FOLDS}, {MAX_FOLDS}]")
    folds = np.zeros(y.size, np.int32)
    with np.errstate(over="ignore"):
        base = splitmix64(np.asarray([int(seed) % (1 << 64)], np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        for p, (a, b) in enumerate(zip(off[:-1], off[1:])):
            key = splitmix64(splitmix64(base + np.uint64(p)) + np.arange(b - a, dtype=np.uint64))
            for c in np.unique(y[a:b]):
                t = np.nonzero(y[a:b] == c)[0]
                folds[a + t[np.argsort(key[t], kind="stable")]] = np.arange(len(t)) % F
    return folds


def _check_folds(folds, n, n_folds):
    F = int(n_folds)
    folds = np.asarray(folds, dtype=np.int64).reshape(-1)
    if not MIN_FOLDS <= F <= MAX_FOLDS:
        raise ValueError(f"n_folds {F} outside [{MIN_FOLDS}, {MAX_FOLDS}]")
    if folds.size != n or (folds.size and (folds.min() < 0 or folds.max() >= F)):
        raise ValueError(f"folds: {n} values in [0, {F})")
    return folds, F


def _cv_decision(Kall, y, K, folds, F, C, tol, max_iter=10_000_000):
    """-> (the values, sum_s |c_s| k(x_s, x_t) + |rho| of the machine behind each: what their float32 storage scales with)."""
    out, weight = np.zeros((len(y), K - 1)), np.zeros((len(y), K - 1))
    for i, j in pairs(K):
        ti, tj = np.nonzero(y == i)[0], np.nonzero(y == j)[0]
        if not len(ti) or not len(tj):
            continue
        idx = np.concatenate([ti, tj])
        sign = np.concatenate([np.ones(len(ti)), -np.ones(len(tj))])
        slot = np.concatenate([np.full(len(ti), _slot(i, j)), np.full(len(tj), _slot(j, i))])
        for f in range(F):
            out_f = folds[idx] == f
            if not out_f.any():
                continue
            tr = ~out_f
            n_i, n_j = int((tr & (sign > 0)).sum()), int((tr & (sign < 0)).sum())
            if n_i == 0 or n_j == 0:                                 # libsvm's svm_binary_svc_probability
                value = 0.0 if n_i == n_j else 1.0 if n_i else -1.0
            else:
                alpha, _, rho, it, gap, cut = smo(Kall[np.ix_(idx[tr], idx[tr])], sign[tr], C, float(tol), max_iter)
                if cut:
                    raise RuntimeError(f"cv_decision_host: pair ({i}, {j}) fold {f} stopped at a gap of {gap:.3e} after {it} iterations")
                value = (alpha * sign[tr]) @ Kall[np.ix_(idx[tr], idx[out_f])] - rho
                weight[idx[out_f], slot[out_f]] = alpha @ Kall[np.ix_(idx[tr], idx[out_f])] + abs(rho)
            out[idx[out_f], slot[out_f]] = value
    return out, weight


def cv_decision_host(x, rows, labels, n_classes, folds, n_folds=5, C=1.0, standardize=False, gamma=0.0, tol=1e-10, want_weight=False):
    """float64 [len(rows), K - 1], laid out as coef: entry t against its m-th other class.  The value is f_ij(x_t) in the libsvm
    convention (positive means the lower class i) of the machine for the pair (i, j) trained on the pair's entries whose fold is not
    t's; centre, scale and gamma are the whole problem's (scaling(): sklearn fixes gamma before libsvm sees the data).  Where that
    training set has no entry of i and none of j the value is 0, with only class i it is +1, with only class j it is -1
    (libsvm's svm_binary_svc_probability); 0 where the other class is absent from the problem.  folds: ints in [0, n_folds).
    want_weight: -> (the values, sum_s |c_s| k(x_s, x_t) + |rho| of the machine behind each, 0 where no machine was trained)."""
    rows, y, K = _problem(x, rows, labels, n_classes)
    folds, F = _check_folds(folds, len(rows), n_folds)
    centre, inv, g = scaling(x, rows, standardize, gamma)
    out = _cv_decision(kernel_host(x, rows, rows, centre, inv, g), y, K, folds, F, float(C), tol)
    return out if want_weight else out[0]


def platt_objective(dec, y, A, B):
    """-> (f, gradient [2], Hessian [2, 2]) of sum t z + log(1 + exp(-z)), z = A dec + B, in the overflow-safe form, with the targets
    t = (N+ + 1) / (N+ + 2) for y = +1 and 1 / (N- + 2) for y = -1."""
    dec, pos = np.asarray(dec, dtype=np.float64), np.asarray(y) > 0
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    t = np.where(pos, (n_pos + 1.0) / (n_pos + 2.0), 1.0 / (n_neg + 2.0))
    z = A * dec + B
    e = np.exp(-np.abs(z))
    f = float((np.where(z >= 0, t, t - 1.0) * z + np.log1p(e)).sum())
    p = np.where(z >= 0, e, 1.0) / (1.0 + e)                         # 1 / (1 + exp(z))
    d1, d2 = t - p, p * (1.0 - p)
    g = np.asarray([(dec * d1).sum(), d1.sum()])
    H = np.asarray([[(dec * dec * d2).sum(), (dec * d2).sum()], [(dec * d2).sum(), d2.sum()]])
    return f, g, H


def platt_host(dec, y, eps=1e-12, max_newton=200):
    """(A, B) of P(class i | f) = 1 / (1 + exp(A f + B)): the minimiser of platt_objective, from (0, log((N- + 1) / (N+ + 1))) by Newton
    steps with a ridge of 1e-12 on the Hessian and backtracking, until |g|_inf <= eps (or the objective's rounding floor).  The algorithm
    of Lin, Lin and Weng (2007), which libsvm's sigmoid_train runs with eps 1e-5 and 100 iterations.  Where all dec are equal only
    A dec + B is unique: compare those values, never A and B."""
    dec, pos = np.asarray(dec, dtype=np.float64), np.asarray(y) > 0
    A, B = 0.0, float(np.log((int((~pos).sum()) + 1.0) / (int(pos.sum()) + 1.0)))
    f, g, H = platt_objective(dec, y, A, B)
    for _ in range(int(max_newton)):
        gn = np.abs(g).max()
        if gn <= eps:
            break
        a, b, c = H[0, 0] + 1e-12, H[0, 1], H[1, 1] + 1e-12
        det = a * c - b * b
        dA, dB = -(c * g[0] - b * g[1]) / det, -(-b * g[0] + a * g[1]) / det
        slope, step, moved = g[0] * dA + g[1] * dB, 1.0, False
        for _ in range(40):
            f2, g2, H2 = platt_objective(dec, y, A + step * dA, B + step * dB)
            # at the rounding floor of f the sufficient-decrease test is noise: there a step that shrinks the gradient is taken
            if f2 < f + 1e-4 * step * slope or (np.abs(g2).max() < gn and f2 <= f + 1e-9 * max(1.0, abs(f))):
                A, B, f, g, H, moved = A + step * dA, B + step * dB, f2, g2, H2, True
                break
            step *= 0.5
        if not moved:
            break
    return float(A), float(B)


def pair_probability(f, A, B):
    """1 / (1 + exp(A f + B)) in the overflow-safe form, clipped to [R_CLIP, 1 - R_CLIP]."""
    z = np.asarray(A, dtype=np.float64) * np.asarray(f, dtype=np.float64) + np.asarray(B, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.clip(np.where(z >= 0, e, 1.0) / (1.0 + e), R_CLIP, 1.0 - R_CLIP)


def couple_matrix(r):
    """Q of Wu, Lin and Weng's method 2 for r [k, k] (r[i, j] + r[j, i] = 1): Q_tt = sum_{j != t} r_jt^2, Q_tj = -r_jt r_tj."""
    Q = -(r.T * r)
    np.fill_diagonal(Q, 0.0)
    off = r.T ** 2
    np.fill_diagonal(off, 0.0)
    return Q + np.diag(off.sum(axis=1))


def couple_host(decision, probA, probB, present):
    """float64 [rows, K]: decision [rows, K (K - 1) / 2] (pairs() order), probA / probB [K (K - 1) / 2], present bool [K].
    r_ij = pair_probability(f_ij, A_ij, B_ij), r_ji = 1 - r_ij over the present classes; p minimises sum_i sum_{j != i} (r_ji p_i -
    r_ij p_j)^2 subject to sum p = 1, from the KKT system [[Q, e], [e', 0]] [p; b] = [0; 1] (couple_matrix) solved directly; libsvm's
    multiclass_probability iterates to 0.005 / K instead.  Absent classes get probability 0; a row with a NaN decision value is NaN."""
    decision = np.asarray(decision, dtype=np.float64)
    present = np.asarray(present, dtype=bool)
    K = present.size
    cls = np.nonzero(present)[0]
    k = len(cls)
    if k < 2:
        raise ValueError("fewer than two classes are present")
    qs = {pr: q for q, pr in enumerate(pairs(K))}
    out = np.zeros((decision.shape[0], K))
    R = np.zeros((decision.shape[0], k, k))
    for a in range(k):
        for b in range(a + 1, k):
            q = qs[(cls[a], cls[b])]
            R[:, a, b] = pair_probability(decision[:, q], np.asarray(probA)[q], np.asarray(probB)[q])
            R[:, b, a] = 1.0 - R[:, a, b]
    M = np.zeros((k + 1, k + 1))
    M[:k, k] = M[k, :k] = 1.0
    rhs = np.zeros(k + 1)
    rhs[k] = 1.0
    for t in range(decision.shape[0]):
        if not np.isfinite(R[t]).all():
            out[t] = np.nan
            continue
        M[:k, :k] = couple_matrix(R[t])
        out[t, cls] = np.linalg.solve(M, rhs)[:k]
    return out


def couple_iterative(r, eps=1e-14, max_iter=100000):
    """libsvm's multiclass_probability on r [k, k]: the fixed-point iteration of Wu, Lin and Weng's algorithm 2 until
    max_t |Q_t p - p'Qp| < eps (libsvm: 0.005 / k, at most max(100, k) sweeps).  -> (p, sweeps)."""
    k = r.shape[0]
    Q = couple_matrix(np.asarray(r, dtype=np.float64))
    p = np.full(k, 1.0 / k)
    it = 0
    for it in range(int(max_iter)):
        Qp = Q @ p
        pQp = float(p @ Qp)
        if np.abs(Qp - pQp).max() < eps:
            break
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t, t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t, t] + 2.0 * Qp[t])) / (1.0 + diff) ** 2
            Qp = (Qp + diff * Q[t]) / (1.0 + diff)
            p /= 1.0 + diff
    return p, it


def svc_proba_host(x, rows, labels, n_classes, folds, n_folds=5, C=1.0, standardize=False, gamma=0.0, tol=1e-10):
    """svc_host plus the sigmoids: -> SvcProbaHost(SvcHost's fields, probA and probB float64 [K (K - 1) / 2] (0 for a pair with an absent
    class), cv_decision float64 [len(rows), K - 1] as cv_decision_host returns it)."""
    model = svc_host(x, rows, labels, n_classes, C, standardize, gamma, tol)
    rows, y, K = _problem(x, rows, labels, n_classes)
    cv = cv_decision_host(x, rows, labels, K, folds, n_folds, C, standardize, gamma, tol)
    probA, probB = np.zeros(K * (K - 1) // 2), np.zeros(K * (K - 1) // 2)
    for q, (i, j) in enumerate(pairs(K)):
        ti, tj = np.nonzero(y == i)[0], np.nonzero(y == j)[0]
        if len(ti) and len(tj):
            dec = np.concatenate([cv[ti, _slot(i, j)], cv[tj, _slot(j, i)]])
            probA[q], probB[q] = platt_host(dec, np.concatenate([np.ones(len(ti)), -np.ones(len(tj))]))
    return SvcProbaHost(*model, probA, probB, cv)


def proba_host(x, eval_rows, train_rows, train_labels, n_classes, folds, n_folds=5, C=1.0, standardize=False, gamma=0.0, tol=1e-10, model=None):
    """float64 [len(eval_rows), K]: SVC(probability=True).predict_proba given the folds: svc_proba_host (or `model`, one it returned),
    decision_host on the evaluation rows, couple_host."""
    m = model if model is not None else svc_proba_host(x, train_rows, train_labels, n_classes, folds, n_folds, C, standardize, gamma, tol)
    dec = decision_host(x, eval_rows, train_rows, train_labels, n_classes, m.coef, m.rho, m.gamma, m.centre, m.inv_scale)
    present = np.bincount(np.asarray(train_labels, dtype=np.int64), minlength=int(n_classes)) > 0
    return couple_host(dec, m.probA, m.probB, present)


def check_problems(rows, labels, offsets, n_rows, dim, n_classes, C=1.0):
    """The refusals of fit_on_device, made before anything is uploaded: problems.check_problems under this module's caps.  What the lists
    hold is the device's to check: an empty problem, a label outside [0, n_classes), a row outside the bank or fewer than two present
    classes gives that problem status 2."""
    return problems.check_problems(rows, labels, offsets, n_rows, dim, n_classes, C, MAX_ROWS, MAX_CLASSES, MAX_DIM)


def chunks(offsets, budget):
    """[(first problem, one past the last)]: consecutive runs of problems whose Gram workspace (problems * largest row count squared * 4
    bytes) stays inside `budget`; a single problem always forms a chunk."""
    sizes = np.diff(np.asarray(offsets, dtype=np.int64))
    out, lo, biggest = [], 0, 0
    for p, n in enumerate(sizes):
        grown = max(biggest, int(n))
        if p > lo and (p + 1 - lo) * grown * grown * 4 > int(budget):
            out.append((lo, p))
            lo, grown = p, int(n)
        biggest = grown
    if len(sizes) > lo:
        out.append((lo, len(sizes)))
    return out


def fit_on_device(x, rows, labels, offsets, n_classes, C=1.0, standardize=False, gamma=0.0, tol=1e-5, max_iter=100000, work_budget=WORK_BUDGET,
                  timings=None):
    """x: CUDA tensor or numpy array [bank rows, dim] float32; problem p trains on bank rows rows[offsets[p] : offsets[p + 1]] with
    labels[...] in [0, n_classes) (rows may repeat inside and across problems: nothing is copied); C: one value or one per problem;
    gamma: a positive value, or 0 for sklearn's "scale".
    -> SvcFit(coef float32 [len(rows), K - 1] aligned with the flat row list (module docstring), rho float32 [P, K (K - 1) / 2], gamma
    float32 [P], centre and inv_scale float32 [P, dim], info int32 [P, 4] = {status, present pairs, pairs cut at max_iter, largest
    iteration count of a pair}, gap float32 [P] = the largest final m(a) - M(a) of a pair, and d_* = the same still on the device).
    status 0 fitted, 2 = no row, a label or row out of range, or fewer than two present classes (nothing else is written for it).
    Three launches per chunk (mkws_svc_prepare, mkws_svc_kernel for the Gram matrices, mkws_svc_fit) and one copy back.  The Gram
    matrices take problems * (largest row count)^2 * 4 bytes; a call that would need more than work_budget bytes (default 512 MiB) is
    run as consecutive chunks of problems, with the same results.  timings: a dict that receives prepare / gram / smo milliseconds
    (device events; this synchronises).  What check_problems refuses is refused before anything is uploaded."""
    return _fit(x, rows, labels, offsets, n_classes, C, standardize, gamma, tol, max_iter, work_budget, timings, None)


def fit_proba_on_device(x, rows, labels, offsets, n_classes, folds=None, n_folds=5, seed=0, C=1.0, standardize=False, gamma=0.0, tol=1e-5,
                        max_iter=100000, platt_eps=1e-8, work_budget=WORK_BUDGET, timings=None):
    """fit_on_device plus what SVC(probability=True) adds, given the folds: int32 [len(rows)] in [0, n_folds), None = cv_folds(labels,
    offsets, n_folds, seed).  Two more launches per chunk, issued while the chunk's Gram matrices are alive: mkws_svc_fit_cv (every
    entry's decision value under the machines trained without its fold) and mkws_svc_platt (the sigmoids, to |gradient|_inf < platt_eps).
    Still one upload and one copy back.
    -> SvcProbaFit: SvcFit's fields plus probA / probB float64 [P, K (K - 1) / 2] (P(class i | f) = 1 / (1 + exp(A f + B)); 0 for a pair
    with an absent class), cv_decision float32 [len(rows), K - 1] (cv_decision_host's layout), cv_info int32 [P, 4] = {status, sub-fits
    solved, sub-fits cut at max_iter, largest iteration count of a sub-fit}, present int32 [P] = bit k set where class k has a row, and
    their d_* twins.  cv_info status 2 = the problem was refused by the fit, or a fold value is outside [0, n_folds): no cv_decision, probA,
    probB or present is written for it.  timings also receives cv / platt milliseconds."""
    return _fit(x, rows, labels, offsets, n_classes, C, standardize, gamma, tol, max_iter, work_budget, timings,
                dict(folds=folds, n_folds=int(n_folds), seed=int(seed), eps=float(platt_eps)))


def _fit(x, rows, labels, offsets, n_classes, C, standardize, gamma, tol, max_iter, work_budget, timings, proba):
    """fit_on_device (proba = None) and fit_proba_on_device (proba = its folds, n_folds, seed and eps)."""
    import torch
    n_rows, dim = problems.bank_shape(x)
    K = int(n_classes)
    rows, labels, off, Cs = check_problems(rows, labels, offsets, n_rows, dim, K, C)
    if int(max_iter) < 1 or not float(tol) >= 0 or not np.isfinite(float(gamma)) or int(work_budget) < 1:
        raise ValueError("max_iter must be at least 1, tol non-negative, gamma finite and work_budget positive")
    P, n_list, npairs = off.size - 1, rows.size, K * (K - 1) // 2
    parts, phases = [off, rows, labels], ("prepare", "gram", "smo")
    if proba is not None:
        folds, F, eps = proba["folds"], proba["n_folds"], proba["eps"]
        if not MIN_FOLDS <= F <= MAX_FOLDS or not eps >= 0:
            raise ValueError(f"n_folds {F} outside [{MIN_FOLDS}, {MAX_FOLDS}], or a negative platt_eps")
        folds = cv_folds(labels, off, F, proba["seed"]) if folds is None else np.asarray(folds)
        if folds.shape != (n_list,) or (folds.size and not np.issubdtype(folds.dtype, np.integer)):
            raise ValueError(f"folds must be one flat list of {n_list} integers")
        # (a value outside [0, n_folds) is the device's to find: that problem gets cv_info status 2)
        parts, phases = parts + [np.clip(folds, -2 ** 31, 2 ** 31 - 1).astype(np.int32)], phases + ("cv", "platt")
    x = problems.device_bank(x)
    dev = x.device
    L = _lib.lib()
    f32 = np.float32
    with torch.cuda.device(dev):
        d_in, (p_C, p_off, p_rows, p_labels, *p_folds) = _lib.upload_words([Cs] + parts, dev)
        extra = [] if proba is None else [("probA", np.float64, (P, npairs)), ("probB", np.float64, (P, npairs))]
        more = [] if proba is None else [("cv_decision", f32, (n_list, K - 1)), ("cv_info", np.int32, (P, 4)), ("present", np.int32, (P,))]
        out = _lib.OutputWords(extra + [("coef", f32, (n_list, K - 1)), ("rho", f32, (P, npairs)), ("gamma", f32, (P,)), ("centre", f32, (P, dim)),
                                ("inv_scale", f32, (P, dim)), ("info", np.int32, (P, 4)), ("gap", f32, (P,))] + more, dev)
        stream = _lib.current_stream_ptr()
        marks = []
        for lo, hi in chunks(off, work_budget) if P else []:
            n, biggest = hi - lo, int(np.diff(off[lo:hi + 1]).max())
            d_work = torch.empty(int(L.mkws_svc_work_bytes(n, biggest)) // 4, dtype=torch.float32, device=dev)
            q_off, q_C = p_off + 4 * lo, p_C + 8 * lo
            centre, inv_scale, d_gamma = out.ptr("centre", lo * dim), out.ptr("inv_scale", lo * dim), out.ptr("gamma", lo)
            info, gap = out.ptr("info", lo * 4), out.ptr("gap", lo)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)] if timings is not None else None
            if ev:
                ev[0].record()
            _lib.check(L.mkws_svc_prepare(x.data_ptr(), n_rows, dim, p_rows, p_labels, q_off, n, K, biggest, int(bool(standardize)), float(gamma),
                                          centre, inv_scale, d_gamma, info, gap, stream))
            if ev:
                ev[1].record()
            _lib.check(L.mkws_svc_kernel(x.data_ptr(), n_rows, dim, p_rows, q_off, biggest, p_rows, q_off, biggest, n, centre, inv_scale, d_gamma,
                                         info, d_work.data_ptr(), biggest * biggest, stream))
            if ev:
                ev[2].record()
            _lib.check(L.mkws_svc_fit(p_labels, q_off, n, K, biggest, q_C, float(tol), int(max_iter), d_work.data_ptr(), biggest * biggest,
                                      out.ptr("coef"), out.ptr("rho", lo * npairs), info, gap, stream))
            if ev:
                ev[3].record()
            if proba is not None:                                      # two more launches while the Gram matrices are alive
                _lib.check(L.mkws_svc_fit_cv(p_labels, q_off, p_folds[0], F, n, K, biggest, q_C, float(tol), int(max_iter), d_work.data_ptr(),
                                             biggest * biggest, info, out.ptr("cv_decision"), out.ptr("cv_info", lo * 4), stream))
                if ev:
                    ev[4].record()
                _lib.check(L.mkws_svc_platt(p_labels, q_off, n, K, biggest, out.ptr("cv_decision"), info, out.ptr("cv_info", lo * 4), eps,
                                            out.ptr("probA", lo * npairs), out.ptr("probB", lo * npairs), out.ptr("present", lo), stream))
                if ev:
                    ev[5].record()
            if ev:
                marks.append(ev)
        out.fetch()                                                    # the call's one synchronisation
        if timings is not None:
            for k, name in enumerate(phases):
                timings[name] = timings.get(name, 0.0) + sum(ev[k].elapsed_time(ev[k + 1]) for ev in marks)
    names = ("coef", "rho", "gamma", "centre", "inv_scale", "info")
    if proba is None:
        return SvcFit(*(out.host(part) for part in names + ("gap",)), *(out.device(part) for part in names))
    names += ("probA", "probB", "cv_decision", "cv_info", "present")
    return SvcProbaFit(*(out.host(part) for part in names + ("gap",)), *(out.device(part) for part in names))


def kernel_on_device(x, rows_a, rows_b, centre, inv_scale, gamma):
    """x: CUDA tensor [bank rows, dim] float32; rows_a / rows_b: CUDA int32 lists or host lists; centre / inv_scale: CUDA float32 [dim]
    or host arrays; gamma: a float.  -> CUDA float32 [len(rows_a), len(rows_b)] = exp(-gamma * max(0, s_a + s_b - 2 a~.b~)) (float64 exp, rounded once),
    NaN where a row is outside the bank.  Asynchronous."""
    import torch
    x = problems.device_bank(x)
    dev = x.device
    n_rows, dim = (int(v) for v in x.shape)
    if not 1 <= dim <= MAX_DIM:
        raise ValueError(f"dim {dim} outside [1, {MAX_DIM}]")
    d_a, d_b = problems.device_int_list(rows_a, "rows_a", dev), problems.device_int_list(rows_b, "rows_b", dev)
    par = []
    for name, a in (("centre", centre), ("inv_scale", inv_scale)):
        if not torch.is_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        if a.dtype != torch.float32 or tuple(a.shape) != (dim,) or a.device != dev:
            raise ValueError(f"{name} must be float32 [{dim}] on the device of x")
        par.append(a.contiguous())
    na, nb = int(d_a.numel()), int(d_b.numel())
    with torch.cuda.device(dev):
        d_gamma = torch.full((1,), float(gamma), dtype=torch.float32, device=dev)
        d_offs = torch.tensor([0, na, 0, nb], dtype=torch.int32, device=dev)
        out = torch.empty((na, nb), dtype=torch.float32, device=dev)
        if na and nb:
            _lib.check(_lib.lib().mkws_svc_kernel(x.data_ptr(), n_rows, dim, d_a.data_ptr(), d_offs.data_ptr(), na, d_b.data_ptr(), d_offs.data_ptr() + 8, nb,
                                                  1, par[0].data_ptr(), par[1].data_ptr(), d_gamma.data_ptr(), None, out.data_ptr(), na * nb,
                                                  _lib.current_stream_ptr()))
    return out


def score_on_device(x, rows, true, offsets, train_rows, train_labels, train_offsets, n_classes, coef, rho, gamma, centre, inv_scale, info=None,
                    want_decision=False, timings=None):
    """x: CUDA tensor [bank rows, dim] float32; problem p is scored on ITS list rows[offsets[p] : offsets[p + 1]] against true[...] under
    model p: the flat training lists it was fitted on (train_rows, train_labels, train_offsets) and what fit_on_device left on the device
    (coef [len(train_rows), K - 1], rho [P, K (K - 1) / 2], gamma [P], centre / inv_scale [P, dim], optionally info [P, 4]).  Lists: CUDA
    int32 tensors or host lists (uploaded non-blocking).
    -> (pred int32 [total], correct int32 [P] = rows with pred == true, decision float32 [total, K (K - 1) / 2] or None), CUDA tensors.
    Asynchronous unless timings (a dict that receives "score" milliseconds) is given.  A row outside the bank, an entry outside every list
    or a problem whose info says it was refused gets pred -1 (NaN decision values) and is never correct."""
    import torch
    x = problems.device_bank(x)
    dev = x.device
    n_rows, dim = (int(v) for v in x.shape)
    K = int(n_classes)
    if not 2 <= K <= MAX_CLASSES or not 1 <= dim <= MAX_DIM:
        raise ValueError(f"n_classes {K} outside [2, {MAX_CLASSES}] or dim {dim} outside [1, {MAX_DIM}]")
    npairs = K * (K - 1) // 2
    d_rows, d_true, d_off = (problems.device_int_list(a, n, dev) for a, n in ((rows, "rows"), (true, "true"), (offsets, "offsets")))
    t_rows, t_labels, t_off = (problems.device_int_list(a, n, dev) for a, n in ((train_rows, "train_rows"), (train_labels, "train_labels"), (train_offsets, "train_offsets")))
    P, total, n_train = int(d_off.numel()) - 1, int(d_rows.numel()), int(t_rows.numel())
    if P < 0 or d_true.numel() != total or t_off.numel() != P + 1 or t_labels.numel() != n_train:
        raise ValueError(f"{total} rows, {int(d_true.numel())} labels, {int(d_off.numel())} offsets and {int(t_off.numel())} training offsets")
    for name, a, shape in (("coef", coef, (n_train, K - 1)), ("rho", rho, (P, npairs)), ("gamma", gamma, (P,)), ("centre", centre, (P, dim)),
                           ("inv_scale", inv_scale, (P, dim))):
        if not (torch.is_tensor(a) and a.device == dev and a.dtype == torch.float32 and tuple(a.shape) == shape):
            raise ValueError(f"{name} must be a CUDA float32 tensor of shape {shape}")
    if info is not None and not (torch.is_tensor(info) and info.device == dev and info.dtype == torch.int32 and tuple(info.shape) == (P, 4)):
        raise ValueError(f"info must be a CUDA int32 tensor of shape {(P, 4)}")
    # the grid is sized by the longest lists: offsets given on the host are read here, device ones are copied back (a synchronisation)
    longest = lambda a, d: int(np.diff(np.asarray(a)).max()) if not torch.is_tensor(a) else int((d[1:] - d[:-1]).max().item())
    max_eval = max(longest(offsets, d_off), 0) if P else 0
    max_train = max(longest(train_offsets, t_off), 0) if P else 0
    if max_train > MAX_ROWS:
        raise ValueError(f"a model of {max_train} rows: at most {MAX_ROWS}")
    coef, rho, gamma, centre, inv_scale = (a.contiguous() for a in (coef, rho, gamma, centre, inv_scale))
    ptr = problems.ptr_or_none
    with torch.cuda.device(dev):
        pred = torch.empty(total, dtype=torch.int32, device=dev)
        correct = torch.empty(P, dtype=torch.int32, device=dev)
        decision = torch.empty((total, npairs), dtype=torch.float32, device=dev) if want_decision else None
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timings is not None else None
        if ev:
            ev[0].record()
        _lib.check(_lib.lib().mkws_svc_score(x.data_ptr(), n_rows, dim, ptr(t_rows), ptr(t_labels), t_off.data_ptr(), max_train, ptr(coef), ptr(rho),
                                             ptr(gamma), ptr(centre), ptr(inv_scale), ptr(info.contiguous()) if info is not None else None, P, K,
                                             ptr(d_rows), ptr(d_true), d_off.data_ptr(), total, max_eval, ptr(pred), ptr(correct), ptr(decision),
                                             _lib.current_stream_ptr()))
        if ev:
            ev[1].record()
            ev[1].synchronize()
            timings["score"] = timings.get("score", 0.0) + ev[0].elapsed_time(ev[1])
    return pred, correct, decision


def _eval_lists(true, offsets, total, dev):
    import torch
    d_true, d_off = problems.device_int_list(true, "true", dev), problems.device_int_list(offsets, "offsets", dev)
    if int(d_true.numel()) != total or int(d_off.numel()) < 1:
        raise ValueError(f"{total} rows, {int(d_true.numel())} labels and {int(d_off.numel())} offsets")
    return d_true, d_off, int(d_off.numel()) - 1


def couple_on_device(decision, true, offsets, probA, probB, present):
    """mkws_svc_couple alone: decision CUDA float32 [total, K (K - 1) / 2] (what score_on_device(want_decision=True) returns), true /
    offsets the evaluation lists, probA / probB CUDA float64 [P, K (K - 1) / 2], present CUDA int32 [P] (bit k = class k has a training row).
    -> (pred int32 [total], correct int32 [P], probs float32 [total, K]), CUDA tensors.  Asynchronous."""
    import torch
    dev = decision.device
    total, npairs = (int(v) for v in decision.shape)
    K = next((k for k in range(2, MAX_CLASSES + 1) if k * (k - 1) // 2 == npairs), None)
    if K is None or decision.dtype != torch.float32 or not decision.is_cuda:
        raise ValueError("decision must be a CUDA float32 tensor [total, K (K - 1) / 2]")
    d_true, d_off, P = _eval_lists(true, offsets, total, dev)
    for name, a, dtype, shape in (("probA", probA, torch.float64, (P, npairs)), ("probB", probB, torch.float64, (P, npairs)),
                                  ("present", present, torch.int32, (P,))):
        if not (torch.is_tensor(a) and a.device == dev and a.dtype == dtype and tuple(a.shape) == shape):
            raise ValueError(f"{name} must be a CUDA {dtype} tensor of shape {shape}")
    decision, probA, probB, present = (a.contiguous() for a in (decision, probA, probB, present))
    ptr = problems.ptr_or_none
    with torch.cuda.device(dev):
        pred = torch.empty(total, dtype=torch.int32, device=dev)
        correct = torch.empty(P, dtype=torch.int32, device=dev)
        probs = torch.empty((total, K), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().mkws_svc_couple(ptr(decision), ptr(d_true), d_off.data_ptr(), P, K, total, ptr(probA), ptr(probB), ptr(present),
                                              ptr(probs), ptr(pred), ptr(correct), _lib.current_stream_ptr()))
    return pred, correct, probs


def proba_on_device(x, rows, true, offsets, train_rows, train_labels, train_offsets, n_classes, coef, rho, gamma, centre, inv_scale, probA, probB,
                    present, info=None):
    """SVC(probability=True).predict_proba and predict for every problem's own evaluation list: score_on_device(want_decision=True)
    followed by mkws_svc_couple under the sigmoids fit_proba_on_device left on the device (d_probA, d_probB, d_present).
    -> (pred int32 [total] = the first argmax of the probabilities, correct int32 [P], probs float32 [total, K]), CUDA tensors.  A row
    outside the bank, an entry outside every list and a refused problem get pred -1 and NaN probabilities."""
    _, _, decision = score_on_device(x, rows, true, offsets, train_rows, train_labels, train_offsets, n_classes, coef, rho, gamma, centre, inv_scale,
                                     info=info, want_decision=True)
    return couple_on_device(decision, true, offsets, probA, probB, present)


def soft_vote_host(probs_a, probs_b):
    """-> (pred int32 = the first argmax of the float64 mean, -1 where either row holds a NaN; the mean)."""
    mean = 0.5 * (np.asarray(probs_a, dtype=np.float64) + np.asarray(probs_b, dtype=np.float64))
    bad = np.isnan(mean).any(axis=1)
    return np.where(bad, -1, np.where(np.isnan(mean), -np.inf, mean).argmax(axis=1)).astype(np.int32), mean


def soft_vote_on_device(probs_a, probs_b, true, offsets, want_mean=False):
    """mkws_soft_vote: VotingClassifier(voting="soft", weights=None) over two classifiers' probabilities, CUDA float32 [total, K] each.
    -> (pred int32 [total] = the first argmax of 0.5 * (a + b), -1 where either row holds a NaN, correct int32 [P], the mean or None),
    CUDA tensors.  Asynchronous."""
    import torch
    dev = probs_a.device
    if not (probs_a.is_cuda and probs_a.dtype == torch.float32 and probs_a.dim() == 2 and probs_b.dtype == torch.float32
            and probs_b.device == dev and probs_b.shape == probs_a.shape and 2 <= int(probs_a.shape[1]) <= MAX_CLASSES):
        raise ValueError(f"two CUDA float32 tensors [total, classes] of one shape, 2 to {MAX_CLASSES} classes")
    total, K = (int(v) for v in probs_a.shape)
    d_true, d_off, P = _eval_lists(true, offsets, total, dev)
    probs_a, probs_b = probs_a.contiguous(), probs_b.contiguous()
    ptr = problems.ptr_or_none
    with torch.cuda.device(dev):
        pred = torch.empty(total, dtype=torch.int32, device=dev)
        correct = torch.empty(P, dtype=torch.int32, device=dev)
        mean = torch.empty((total, K), dtype=torch.float32, device=dev) if want_mean else None
        _lib.check(_lib.lib().mkws_soft_vote(ptr(probs_a), ptr(probs_b), ptr(d_true), d_off.data_ptr(), P, K, total, ptr(pred), ptr(correct), ptr(mean),
                                             _lib.current_stream_ptr()))
    return pred, correct, mean
