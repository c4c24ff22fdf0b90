"""K L1 logistic regressions on the device (mkws_lr_l1_fit, multilingual_kws_amd/lr_l1.py) against the golden fixture
tests/golden/lr_l1_golden.npz (made on the CPU by tests/golden/make_lr_l1_golden.py; this file reads only it plus NumPy).

The yardstick is the optimum of the convex one-vs-rest problems.  With u = 2^-24, the returned float32 weights widened to float64 and
r_i = sigma(-s_i z_i), the float64 violation of a class that stopped for reason 0 is at most vtol + e,

    e = max_j C sum_i |x_ij| (delta_i + (n + 2) u r_i),      delta_i = 1/4 (dim + 2) u (sum_j |x_ij w_j| + |b|) + 8 u,

the worst-case forward error of a float32 evaluation of the gradient in any summation order (delta_i: the logit's dot product through
sigma's slope of at most 1/4, plus the rounding of exp, the division and the product; (n + 2) u: the column sum).  It is loose, around
1e-2 at the harness shape; what is consumed downstream is an argmax.  From it, by convexity (f(w) - f* <= |v|_inf |w - w*|_1),
f_dev - f* <= (vtol + e) (|w_dev|_1 + |w*|_1)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from lr_l1_cases import AGAINST_SKLEARN, CASES, case, dense_star, problems, x_hash  # noqa: E402
from test_selection_eval_cpu import WORDS, experiment, splits_for, stub_bank  # noqa: E402

from multilingual_kws_amd import logreg, lr_l1  # noqa: E402
from multilingual_kws_amd.embedding import selection_eval as se  # noqa: E402

pytestmark = pytest.mark.gpu

VTOL = 1e-3
U = 2.0 ** -24
_GOLDEN, _FIT = [], {}


def golden(golden_dir):
    if not _GOLDEN:
        _GOLDEN.append(dict(np.load(os.path.join(golden_dir, "lr_l1_golden.npz"))))
    return _GOLDEN[0]


def fitted(name):
    """One fit_on_device call per case (the wrapper's defaults), shared by the tests and left unchanged."""
    if name not in _FIT:
        c = case(name)
        _FIT[name] = lr_l1.fit_on_device(c["x"], c["rows"], c["labels"], c["offsets"], c["n_classes"], C=c["C"])
    return _FIT[name]


def gradient_error(x, rows, y, K, C, coef, intercept):
    """e [K] of the module docstring at the float32 point (coef [K, dim], intercept [K])."""
    X = np.abs(x[rows].astype(np.float64))
    Xs = x[rows].astype(np.float64)
    n, dim = X.shape
    W, b = coef.astype(np.float64), intercept.astype(np.float64)
    S = np.where(np.asarray(y)[None, :] == np.arange(K)[:, None], 1.0, -1.0)                 # [K, n]
    Z = Xs @ W.T + b                                                                         # [n, K]
    r = np.exp(-np.logaddexp(0.0, S * Z.T))                                                  # [K, n]
    delta = 0.25 * (dim + 2) * U * (X @ np.abs(W).T + np.abs(b)).T + 8 * U                   # [K, n]
    t = delta + (n + 2) * U * r
    return C * np.maximum((t @ X).max(axis=1), t.sum(axis=1))                                # (the bias column is all ones)


@pytest.mark.parametrize("name", list(CASES))
def test_contract_optimality_and_objective_gap(name, golden_dir):
    pytest.importorskip("torch")
    g, c = golden(golden_dir), case(name)
    assert str(g[name + "/x_sha1"]) == x_hash(c)
    K, dim = c["n_classes"], c["x"].shape[1]
    P = len(c["offsets"]) - 1
    fit = fitted(name)
    assert fit.coef.shape == (P, K, dim) and fit.coef.dtype == np.float32 and fit.intercept.shape == (P, K) and fit.intercept.dtype == np.float32
    assert fit.info.shape == (P, K, 4) and fit.info.dtype == np.int32 and fit.stats.shape == (P, K, 2) and fit.stats.dtype == np.float64
    assert tuple(fit.d_coef.shape) == (P, K, dim) and tuple(fit.d_intercept.shape) == (P, K) and fit.d_coef.is_cuda
    star_w, star_b = dense_star(g, name, P, K, dim)
    worst_gap, worst_viol, worst_e, n_iter_seen = 0.0, 0.0, 0.0, []
    for p, (rows, y, C, _, _) in enumerate(problems(c)):
        f_dev, v_dev = lr_l1.objective(c["x"], rows, y, K, C, fit.coef[p], fit.intercept[p])
        e = gradient_error(c["x"], rows, y, K, C, fit.coef[p], fit.intercept[p])
        f_star = g[name + "/f_star"][p]
        norms = np.abs(fit.coef[p].astype(np.float64)).sum(axis=1) + np.abs(fit.intercept[p].astype(np.float64)) + np.abs(star_w[p]).sum(axis=1) + np.abs(star_b[p])
        for k in range(K):
            status, n_iter, reason, nnz = fit.info[p, k].tolist()
            assert status == 0 and 1 <= n_iter <= lr_l1.MAX_ITER and reason in (0, 1), fit.info[p, k]
            assert reason == (0 if fit.stats[p, k, 1] <= VTOL else 1) and (reason == 0 or n_iter == lr_l1.MAX_ITER), (fit.info[p, k], fit.stats[p, k])
            assert reason == 0 or (name == "c_0p01_1_100" and C == 100.0), (name, p, k, fit.info[p, k])
            assert nnz == int(np.count_nonzero(fit.coef[p, k]))
            slack = VTOL + e[k] if reason == 0 else v_dev[k]          # (a class stopped by max_iter: the convexity bound under its own violation)
            if P <= 3:
                print(f"{name} problem {p} class {k}: n_iter {n_iter}, reason {reason}, non-zeros {nnz}, float64 violation {v_dev[k]:.3e} (e {e[k]:.3e}), "
                      f"f_dev - f* {f_dev[k] - f_star[k]:.3e} = {(f_dev[k] - f_star[k]) / f_star[k]:.2e} f*, bound {slack * norms[k]:.3e}")
            assert v_dev[k] <= slack, (name, p, k, v_dev[k], e[k])
            assert -1e-9 * f_star[k] <= f_dev[k] - f_star[k] <= slack * norms[k], (name, p, k, f_dev[k] - f_star[k], slack * norms[k])
            # what the device reports is what it returned
            assert abs(fit.stats[p, k, 0] - f_dev[k]) <= 1e-4 * max(1.0, f_dev[k]), (name, p, k, fit.stats[p, k, 0], f_dev[k])
            if reason == 0:
                worst_gap = max(worst_gap, (f_dev[k] - f_star[k]) / f_star[k])
                worst_viol, worst_e = max(worst_viol, v_dev[k]), max(worst_e, e[k])
                n_iter_seen.append(n_iter)
        if name in AGAINST_SKLEARN:                                   # at least as converged as sklearn's default run, all classes together
            gap_dev, gap_sk = float((f_dev - f_star).sum()), float((g[name + "/f_sklearn"][p] - f_star).sum())
            print(f"{name} problem {p}: sum_k (f_dev - f*) {gap_dev:.3e} = {gap_dev / f_star.sum():.2e} relative; sklearn's default run {gap_sk:.3e} = {gap_sk / f_star.sum():.2e}")
            assert gap_dev <= gap_sk, (name, p, gap_dev, gap_sk)
    print(f"{name}: largest relative gap (f_dev - f*) / f* of a class stopped for reason 0 {worst_gap:.3e}; such classes: {len(n_iter_seen)} with {min(n_iter_seen)} to "
          f"{max(n_iter_seen)} iterations, largest float64 violation {worst_viol:.3e}, largest e {worst_e:.3e}")


@pytest.mark.parametrize("name", list(CASES))
def test_predictions_are_the_optimums_on_clear_rows(name, golden_dir):
    """Through logreg.score_on_device on the case's evaluation rows.  A row is clear when the top-two margin of the optimum's float64 logits
    exceeds twice (gamma_{dim+1} + vtol + e) (sum_j |x_j w_j| + |b|): the rounding bound of the float32 dot product of
    tests/test_logreg_gpu.py and the solver's slack, scaled the same way.  At least 0.9 of every problem's rows are clear (a condition on
    the inputs)."""
    torch = pytest.importorskip("torch")
    g, c, fit = golden(golden_dir), case(name), fitted(name)
    K, dim = c["n_classes"], c["x"].shape[1]
    d_x = torch.from_numpy(c["x"].copy()).cuda()
    pred, correct, _, _ = logreg.score_on_device(d_x, c["eval_rows"], c["eval_true"], c["eval_offsets"], fit.d_coef, fit.d_intercept)
    pred, correct = pred.cpu().numpy(), correct.cpu().numpy()
    gamma = (dim + 1) * U / (1 - (dim + 1) * U)
    ev = c["eval_offsets"]
    tightest = np.inf
    for p, (rows, y, C, ev_rows, ev_true) in enumerate(problems(c)):
        lo, hi = int(ev[p]), int(ev[p + 1])
        z_star = g[name + "/z_star"][lo:hi]
        if (fit.info[p, :, 2] != 0).any():                            # the C = 100 problem stopped by max_iter: no slack is promised for it
            continue
        if not z_star.any():                                          # the C = 0.01 problem: the optimum is zero, no row has a margin, and
            assert not fit.coef[p].any() and not fit.intercept[p].any() and not pred[lo:hi].any()      # the first argmax of equal logits is class 0
            continue
        e = gradient_error(c["x"], rows, y, K, C, fit.coef[p], fit.intercept[p])
        size = np.abs(c["x"][ev_rows].astype(np.float64)) @ np.abs(fit.coef[p].astype(np.float64)).T + np.abs(fit.intercept[p].astype(np.float64))
        bound = ((gamma + VTOL + e)[None, :] * size).max(axis=1)
        top = np.sort(z_star, axis=1)
        clear = top[:, -1] - top[:, -2] > 2 * bound
        z_dev = c["x"][ev_rows].astype(np.float64) @ fit.coef[p].astype(np.float64).T + fit.intercept[p].astype(np.float64)
        tightest = min(tightest, float(((top[:, -1] - top[:, -2])[clear] / np.maximum(2 * np.abs(z_dev - z_star).max(axis=1)[clear], 1e-300)).min()))
        assert clear.mean() >= 0.9, (name, p, clear.mean())
        assert np.array_equal(pred[lo:hi][clear], z_star.argmax(axis=1)[clear]), (name, p)
        assert correct[p] == int((pred[lo:hi] == ev_true).sum())
    print(f"{name}: the closest clear row's margin is {tightest:.1f} times twice the logits' actual distance from the optimum's")


def test_degenerate_solutions(golden_dir):
    torch = pytest.importorskip("torch")
    # C = 0.01: nothing leaves zero
    c, fit = case("c_0p01_1_100"), fitted("c_0p01_1_100")
    assert c["C"][0] == 0.01 and fit.coef[0].tobytes() == bytes(fit.coef[0].nbytes) and fit.intercept[0].tobytes() == bytes(fit.intercept[0].nbytes)
    assert (fit.info[0, :, 1] <= lr_l1.CHECK_EVERY).all() and (fit.info[0, :, 2] == 0).all() and (fit.info[0, :, 3] == 0).all()
    n = int(c["offsets"][1] - c["offsets"][0])
    assert np.allclose(fit.stats[0, :, 0], 0.01 * n * np.log(2.0), rtol=1e-6) and (fit.stats[0, :, 1] == 0).all()
    pred = logreg.score_on_device(torch.from_numpy(c["x"].copy()).cuda(), c["eval_rows"], c["eval_true"], c["eval_offsets"], fit.d_coef, fit.d_intercept)[0]
    assert not pred.cpu().numpy()[:int(c["eval_offsets"][1])].any()                       # every prediction is class 0
    # K = 2: row 0 is the negation of row 1, bit for bit, and zeros stay +0.0
    fit = fitted("n10_k2_dim1024")
    w1, b1 = fit.coef[0, 1], fit.intercept[0, 1]
    assert fit.coef[0, 0].tobytes() == np.where(w1 == 0, np.float32(0), -w1).astype(np.float32).tobytes() and fit.intercept[0, 0] == -b1
    assert np.count_nonzero(w1) >= 1 and fit.info[0, 0].tolist() == fit.info[0, 1].tolist() and fit.stats[0, 0].tolist() == fit.stats[0, 1].tolist()
    # the absent class: its closed form within the violation bound
    c, fit = case("absent_class"), fitted("absent_class")
    rows, y, C, _, _ = problems(c)[0]
    assert 2 not in set(y.tolist()) and not fit.coef[0, 2].any()
    e = gradient_error(c["x"], rows, y, 4, C, fit.coef[0], fit.intercept[0])[2]
    # with w = 0 the bias gradient is g(b) = C n sigma(b); the violation |g(b) - 1| <= vtol + e puts sigma(b) within (vtol + e) / (C n) of
    # 1 / (C n), and b = logit(sigma(b))
    cn, slack = C * len(rows), VTOL + e
    lo, hi = np.log((1 - slack) / (cn - (1 - slack))), np.log((1 + slack) / (cn - (1 + slack)))
    print(f"absent class: b = {fit.intercept[0, 2]:.6f}, closed form {-np.log(cn - 1):.6f}, admitted [{lo:.6f}, {hi:.6f}]")
    assert lo - 1e-6 <= fit.intercept[0, 2] <= hi + 1e-6


def test_two_calls_write_equal_bytes_and_a_problem_does_not_see_its_neighbours():
    pytest.importorskip("torch")
    c, fit = case("ragged_50_20_64"), fitted("ragged_50_20_64")
    again = lr_l1.fit_on_device(c["x"], c["rows"], c["labels"], c["offsets"], c["n_classes"], C=c["C"])
    for part in ("coef", "intercept", "info", "stats"):
        assert getattr(again, part).tobytes() == getattr(fit, part).tobytes(), part
    off = c["offsets"]
    for p in (1, 2):                                                  # problem 1 shares a row with problem 0; problem 2 names a row twice
        alone = lr_l1.fit_on_device(c["x"], c["rows"], c["labels"], off[p:p + 2], c["n_classes"], C=c["C"][p])
        for part in ("coef", "intercept", "info", "stats"):
            assert getattr(alone, part)[0].tobytes() == getattr(fit, part)[p].tobytes(), (p, part)


def test_one_iteration_goes_downhill():
    pytest.importorskip("torch")
    c = case("n7_k3_dim37")
    fit = lr_l1.fit_on_device(c["x"], c["rows"], c["labels"], c["offsets"], 3, C=c["C"], max_iter=1, vtol=0.0)
    assert (fit.info[0, :, 0] == 0).all() and (fit.info[0, :, 1] == 1).all() and (fit.info[0, :, 2] == 1).all()
    f0 = float(c["C"][0]) * len(c["rows"]) * np.log(2.0)
    f_dev, _ = lr_l1.objective(c["x"], c["rows"], c["labels"], 3, c["C"][0], fit.coef[0], fit.intercept[0])
    assert (f_dev < f0).all() and (fit.stats[0, :, 0] < f0).all() and (fit.stats[0, :, 1] > 0).all(), (f_dev, f0)


@pytest.mark.parametrize("kind", ["empty", "label", "row"])
def test_bad_problems_get_status_2_beside_unaffected_neighbours(kind):
    pytest.importorskip("torch")
    c, fit = case("ragged_50_20_64"), fitted("ragged_50_20_64")
    rows, labels, off, K = c["rows"].copy(), c["labels"].copy(), c["offsets"].copy(), c["n_classes"]
    if kind == "empty":                                               # an empty problem between problems 0 and 1
        off = np.asarray([off[0], off[1], off[1], off[2], off[3]], np.int32)
        bad, same = 1, {0: 0, 2: 1, 3: 2}
    else:
        if kind == "label":
            labels[off[1] + 5] = K
        else:
            rows[off[2] - 1] = c["x"].shape[0]
        bad, same = 1, {0: 0, 2: 2}
    got = lr_l1.fit_on_device(c["x"], rows, labels, off, K, C=1.0)
    assert got.info[bad].tolist() == [[2, 0, 0, 0]] * K
    assert not got.coef[bad].any() and not got.intercept[bad].any() and not got.stats[bad].any()      # (the wrapper's buffers start as zeros)
    for q, p in same.items():
        for part in ("coef", "intercept", "info", "stats"):
            assert getattr(got, part)[q].tobytes() == getattr(fit, part)[p].tobytes(), (kind, q, part)


def test_harness_on_the_device_equals_the_host_path():
    """2 experiments x 3 splits on the well separated stub bank of tests/test_selection_eval_cpu.py.  Compared with == after asserting that
    every compared row is clear: the top-two gap of the host model's float64 logits exceeds twice what the device model's differ by."""
    torch = pytest.importorskip("torch")
    bank, word_rows, ut, ue = stub_bank(spread=0.3)
    exps = [experiment(word_rows, WORDS[:3]), experiment(word_rows, WORDS[3:6])]
    splits = [splits_for(e, 3, 20 + i) for i, e in enumerate(exps)]
    K, fit_l, val_l, dev_l, n_splits = se._lists(exps, ut, ue, splits)
    d_bank = torch.from_numpy(bank.copy()).cuda()
    dev = se._lr_l1_fit(d_bank, fit_l, K, 1.0, False, lr_l1.MAX_ITER, 1e-6, 1e-5)
    hosts = se._lr_l1_fit(bank, fit_l, K, 1.0, False, lr_l1.MAX_ITER, 1e-6, 1e-5)
    assert K == 4 and n_splits == [3, 3] and (dev.info[:, :, 0] == 0).all() and (dev.info[:, :, 2] == 0).all()
    tightest = np.inf
    for p, h in enumerate(hosts):
        rows = np.concatenate([val_l[0][val_l[2][p]:val_l[2][p + 1]], dev_l[0][dev_l[2][p // 3]:dev_l[2][p // 3 + 1]]])
        X = bank[rows].astype(np.float64)
        z_h, z_d = X @ h.coef.T + h.intercept, X @ dev.coef[p].astype(np.float64).T + dev.intercept[p].astype(np.float64)
        top = np.sort(z_h, axis=1)
        gap, apart = top[:, -1] - top[:, -2], np.abs(z_d - z_h).max(axis=1) + logreg_dot_bound(bank[rows], dev.coef[p], dev.intercept[p])
        tightest = min(tightest, float((gap / (2 * apart)).min()))
        assert np.all(gap > 2 * apart), (p, float(gap.min()), float(apart.max()))
    print(f"the closest row clears its boundary {tightest:.1f} times over")
    on_dev = se.experiment_run_many(d_bank, exps, ut, ue, splits, classifier="lr_l1")
    on_host = se.experiment_run_many(bank, exps, ut, ue, splits, classifier="lr_l1", on_device=False)
    assert on_dev == on_host, (on_dev, on_host)
    assert se.experiment_run_many(bank, exps, ut, ue, splits, classifier="lr_l1", on_device=True) == on_dev        # a host bank is uploaded
    with pytest.raises(ValueError, match="refused"):
        se.experiment_run_many(d_bank, exps, np.asarray([len(bank), 0]), ue, splits, classifier="lr_l1")           # a training row outside the bank


def logreg_dot_bound(x_rows, coef, intercept):
    """The float32 dot-product bound of tests/test_logreg_gpu.py, the largest over the classes per row."""
    n = coef.shape[1] + 1
    gamma = n * U / (1 - n * U)
    return (gamma * (np.abs(x_rows.astype(np.float64)) @ np.abs(coef.astype(np.float64)).T + np.abs(intercept.astype(np.float64)))).max(axis=1)
