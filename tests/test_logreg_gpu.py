"""K logistic regressions on the device (mkws_logreg_fit / mkws_logreg_score, multilingual_kws_amd/logreg.py) against the golden fixture
tests/golden/logreg_golden.npz (made on the CPU by tests/golden/make_logreg_golden.py; this file reads only it plus NumPy).

The problem is strictly convex in W, so the yardstick is the optimum: for every fitted problem the float64 objective at the returned
float32 (W, b) -- logreg.objective, in the scaled space for the scaled cases -- must satisfy  f_dev - f_star <= f_sklearn - f_star, i.e.
the device is at least as converged as sklearn's default run, with no further margin; likewise max |P_dev - P*| <= p_sklearn on the
evaluation rows.  The scorer is held to the rounding bound of a float32 dot product."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from logreg_cases import CASES, case, problems, x_hash  # noqa: E402

from multilingual_kws_amd import logreg  # noqa: E402

MAX_ITER, GTOL = 300, 1e-6
U = 2.0 ** -24
_GOLDEN, _FIT = [], {}


def golden(golden_dir):
    if not _GOLDEN:
        _GOLDEN.append(dict(np.load(os.path.join(golden_dir, "logreg_golden.npz"))))
    return _GOLDEN[0]


def fitted(name):
    """One fit_on_device call per case, shared by the tests and left unchanged."""
    if name not in _FIT:
        c = case(name)
        _FIT[name] = logreg.fit_on_device(c["x"], c["rows"], c["labels"], c["offsets"], c["n_classes"], C=c["C"], standardize=c["standardize"],
                                          max_iter=MAX_ITER, gtol=GTOL)
    return _FIT[name]


def star(g, name, p, K, dim):
    theta = g[name + "/theta_star"][p]
    return theta[:K * dim].reshape(K, dim), theta[K * dim:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_is_at_least_as_converged_as_sklearn(name, golden_dir):
    pytest.importorskip("torch")
    g, c = golden(golden_dir), case(name)
    assert str(g[name + "/x_sha1"]) == x_hash(c)
    K, dim = c["n_classes"], c["x"].shape[1]
    fit = fitted(name)
    P = len(c["offsets"]) - 1
    assert fit.coef.shape == (P, K, dim) and fit.coef.dtype == np.float32 and fit.intercept.shape == (P, K) and fit.info.shape == (P, 4)
    worst_f, worst_p = 0.0, 0.0
    for p, (rows, y, C, ev_rows, _) in enumerate(problems(c)):
        status, n_iter, reason, n = fit.info[p].tolist()
        assert status == 0 and n == len(rows) and 1 <= n_iter <= MAX_ITER and reason == (1 if n_iter == MAX_ITER and fit.stats[p, 1] > GTOL else 0), fit.info[p]
        f_dev, _ = logreg.objective(c["x"], rows, y, K, C, fit.coef[p], fit.intercept[p], c["standardize"])
        f_star, f_sk = g[name + "/f_star"][p], g[name + "/f_sklearn"][p]
        _, p_star = logreg.predict_host(c["x"], ev_rows, *star(g, name, p, K, dim))
        _, p_dev = logreg.predict_host(c["x"], ev_rows, fit.coef[p], fit.intercept[p])
        dp = np.abs(p_dev - p_star).max()
        if P <= 3:
            print(f"{name} problem {p}: n_iter {n_iter}, reason {reason}, f_dev - f_star {f_dev - f_star:.3e} (sklearn {f_sk - f_star:.3e}), "
                  f"max |P_dev - P*| {dp:.3e} (sklearn {g[name + '/p_sklearn'][p]:.3e}), |g|_inf {fit.stats[p, 1]:.2e}")
        worst_f, worst_p = max(worst_f, (f_dev - f_star) / (f_sk - f_star)), max(worst_p, dp / g[name + "/p_sklearn"][p])
        assert f_dev - f_star <= f_sk - f_star, (name, p, f_dev - f_star, f_sk - f_star)
        assert dp <= g[name + "/p_sklearn"][p], (name, p, dp)
        # what the device reports is what it returned: its float32 objective against the float64 one at the same point
        assert abs(fit.stats[p, 0] - f_dev) <= 1e-4 * max(1.0, f_dev) and fit.stats[p, 1] >= 0
        assert abs(float(fit.intercept[p].astype(np.float64).sum() + _shift(c, rows, fit.coef[p]))) <= 1e-4 * max(1.0, np.abs(fit.intercept[p]).max())
    print(f"{name}: worst share of sklearn's slack used: objective {worst_f:.3e}, probabilities {worst_p:.3e}")


def _shift(c, rows, coef):
    """sum_k W_k . mu for the scaled cases (there sum_k b~_k = sum_k (b_k + W_k . mu) is what is zero), 0 for the raw ones."""
    if not c["standardize"]:
        return 0.0
    return float((coef.astype(np.float64) @ c["x"][rows].astype(np.float64).mean(axis=0)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged_50_20_64", "65_problems_of_8_dim16", "k6_n200_scaled"])
def test_two_calls_write_equal_bytes(name):
    pytest.importorskip("torch")
    c, first = case(name), fitted(name)
    again = logreg.fit_on_device(c["x"], c["rows"], c["labels"], c["offsets"], c["n_classes"], C=c["C"], standardize=c["standardize"],
                                 max_iter=MAX_ITER, gtol=GTOL)
    for a, b in zip(first[:4], again[:4]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_shared_and_repeated_rows_are_gathered_not_copied():
    """Problem 1 of the ragged case alone (its list names a row of problem 0) gives the bytes it gives beside its neighbours."""
    pytest.importorskip("torch")
    c, all3 = case("ragged_50_20_64"), fitted("ragged_50_20_64")
    lo, hi = int(c["offsets"][1]), int(c["offsets"][2])
    alone = logreg.fit_on_device(c["x"], c["rows"][lo:hi], c["labels"][lo:hi], [0, hi - lo], c["n_classes"], C=c["C"][1], max_iter=MAX_ITER, gtol=GTOL)
    assert alone.coef[0].tobytes() == all3.coef[1].tobytes() and alone.info[0].tolist() == all3.info[1].tolist()
    assert set(c["rows"][lo:hi].tolist()) & set(c["rows"][int(c["offsets"][0]):lo].tolist())
    assert len(set(c["rows"][hi:int(c["offsets"][3])].tolist())) == 63


@pytest.mark.gpu
def test_one_iteration_is_a_step_downhill():
    """max_iter = 1: status 0, stop reason 1, n_iter 1 and an objective below f(0) = C n ln K."""
    pytest.importorskip("torch")
    c = case("c_0p01_1_100")
    fit = logreg.fit_on_device(c["x"], c["rows"], c["labels"], c["offsets"], 3, C=c["C"], max_iter=1, gtol=0.0)
    for p, (rows, y, C, _, _) in enumerate(problems(c)):
        assert fit.info[p].tolist() == [0, 1, 1, 60]
        f_dev, _ = logreg.objective(c["x"], rows, y, 3, C, fit.coef[p], fit.intercept[p])
        assert f_dev < C * 60 * np.log(3) and fit.stats[p, 0] < C * 60 * np.log(3)
        assert abs(fit.stats[p, 0] - f_dev) <= 1e-5 * f_dev


@pytest.mark.gpu
def test_bad_problems_get_status_2_beside_unaffected_neighbours():
    pytest.importorskip("torch")
    c, good = case("ragged_50_20_64"), fitted("ragged_50_20_64")
    off = c["offsets"].tolist()
    n_bank = c["x"].shape[0]
    for what in ("empty", "label", "negative label", "row", "negative row"):
        rows, labels, offsets = c["rows"].copy(), c["labels"].copy(), list(off)
        if what == "empty":
            rows, labels = np.delete(rows, np.s_[off[1]:off[2]]), np.delete(labels, np.s_[off[1]:off[2]])
            offsets = [off[0], off[1], off[1], off[3] - (off[2] - off[1])]
        elif what == "label":
            labels[off[1] + 5] = c["n_classes"]
        elif what == "negative label":
            labels[off[1] + 5] = -1
        elif what == "row":
            rows[off[2] - 1] = n_bank
        else:
            rows[off[1]] = -1
        fit = logreg.fit_on_device(c["x"], rows, labels, offsets, c["n_classes"], C=c["C"], max_iter=MAX_ITER, gtol=GTOL)
        assert fit.info[1].tolist() == [2, 0, 0, 0 if what == "empty" else 20], (what, fit.info[1])
        assert not fit.coef[1].any() and not fit.intercept[1].any() and not fit.stats[1].any(), what      # nothing else is written (on canary-filled outputs: tests/test_dataperf_fenced_gpu.py)
        for p in (0, 2):
            assert fit.coef[p].tobytes() == good.coef[p].tobytes() and fit.info[p].tolist() == good.info[p].tolist(), (what, p)
            assert fit.stats[p].tobytes() == good.stats[p].tobytes() and fit.intercept[p].tobytes() == good.intercept[p].tobytes()


@pytest.mark.gpu
def test_refused_arguments_and_no_problem():
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib
    c = case("n7_k3_dim37")
    empty = logreg.fit_on_device(c["x"], [], [], [0], 3)
    assert empty.coef.shape == (0, 3, 37) and empty.info.shape == (0, 4) and empty.stats.shape == (0, 2)
    L = _lib.lib()
    d_x = torch.from_numpy(c["x"].copy()).cuda()
    d_rows, d_y, d_off = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("rows", "labels", "offsets"))
    d_C = torch.ones(1, dtype=torch.float64, device="cuda")
    out = torch.zeros(4096, dtype=torch.float32, device="cuda")
    d_info, d_stats = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda")
    n_work = L.mkws_logreg_work_floats(37, 1, 3)
    assert n_work == 3 * 3 * 37
    d_work = torch.zeros(n_work, dtype=torch.float32, device="cuda")

    def call(K=3, dim=37, max_iter=10, gtol=1e-6, standardize=0, work=n_work, coef=out.data_ptr(), P=1):
        return L.mkws_logreg_fit(d_x.data_ptr(), c["x"].shape[0], dim, d_rows.data_ptr(), d_y.data_ptr(), d_off.data_ptr(), P, K, d_C.data_ptr(), standardize,
                                 max_iter, gtol, coef, out.data_ptr() + 2048, d_info.data_ptr(), d_stats.data_ptr(), d_work.data_ptr(), work, None)

    assert call(K=1) == -1 and call(K=9) == -2 and call(dim=0) == -1 and call(dim=1025) == -2 and call(max_iter=0) == -1
    assert call(gtol=-1.0) == -1 and call(gtol=float("nan")) == -1 and call(standardize=2) == -1 and call(work=n_work - 1) == -1
    assert call(coef=None) == -1 and call(P=-1) == -1
    assert call(P=0) == 0
    torch.cuda.synchronize()
    assert not out.any().item() and not d_info.any().item()           # a refused call writes nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert d_info.cpu().tolist()[0] == 0 and out.any().item()
    with pytest.raises(ValueError):
        logreg.score_on_device(d_x, [0], [0], [0, 1], out[:3 * 36].view(1, 3, 36), out[:3].view(1, 3))


# ------------------------------------------------------------------------------------------------ the scorer

def dot_bound(x_rows, coef, intercept):
    """gamma_{dim+1} * (sum_j |w_j x_j| + |b|) with gamma_n = n u / (1 - n u), u = 2^-24: the bound on a float32 dot product of dim terms
    and the bias added in any order, with or without fused multiply-adds."""
    n = coef.shape[1] + 1
    gamma = n * U / (1 - n * U)
    return gamma * ((np.abs(x_rows.astype(np.float64))[:, None, :] * np.abs(coef.astype(np.float64))[None]).sum(-1) + np.abs(intercept.astype(np.float64)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_score_is_the_float32_dot_product_within_its_bound(name):
    torch = pytest.importorskip("torch")
    c, fit = case(name), fitted(name)
    K = c["n_classes"]
    d_x = torch.from_numpy(c["x"].copy()).cuda()
    pred, correct, probs, logits = logreg.score_on_device(d_x, c["eval_rows"], c["eval_true"], c["eval_offsets"], fit.d_coef, fit.d_intercept,
                                                          want_probs=True, want_logits=True)
    pred, correct, probs, logits = pred.cpu().numpy(), correct.cpu().numpy(), probs.cpu().numpy(), logits.cpu().numpy()
    only_pred, only_correct, none_p, none_l = logreg.score_on_device(d_x, c["eval_rows"], c["eval_true"], c["eval_offsets"], fit.d_coef, fit.d_intercept)
    assert none_p is None and none_l is None and np.array_equal(only_pred.cpu().numpy(), pred) and np.array_equal(only_correct.cpu().numpy(), correct)
    ev = c["eval_offsets"]
    for p, (_, _, _, ev_rows, ev_true) in enumerate(problems(c)):
        lo, hi = int(ev[p]), int(ev[p + 1])
        w, b = fit.coef[p], fit.intercept[p]
        z64 = c["x"][ev_rows].astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
        bound = dot_bound(c["x"][ev_rows], w, b)
        assert np.all(np.abs(logits[lo:hi].astype(np.float64) - z64) <= bound), (name, p, np.abs(logits[lo:hi] - z64).max(), bound.min())
        top = np.sort(z64, axis=1)
        clear = top[:, -1] - top[:, -2] > 2 * bound.max(axis=1)
        assert clear.mean() >= 0.9, (name, p, clear.mean())
        assert np.array_equal(pred[lo:hi][clear], z64.argmax(axis=1)[clear])
        assert np.array_equal(pred[lo:hi], logits[lo:hi].argmax(axis=1))                       # the first argmax of its own logits
        assert correct[p] == int((pred[lo:hi] == ev_true).sum())
        z32 = logits[lo:hi].astype(np.float64)
        soft = np.exp(z32 - z32.max(axis=1, keepdims=True))
        assert np.abs(probs[lo:hi] - soft / soft.sum(axis=1, keepdims=True)).max() <= 1e-6


@pytest.mark.gpu
def test_score_lists_are_each_problems_own_and_bad_entries_are_not_read():
    torch = pytest.importorskip("torch")
    c, fit = case("ragged_50_20_64"), fitted("ragged_50_20_64")
    d_x = torch.from_numpy(c["x"].copy()).cuda()
    n_bank = c["x"].shape[0]
    _, _, _, ev0, t0 = problems(c)[0]
    _, _, _, ev2, t2 = problems(c)[2]
    # two leading entries that no list names; problem 0 scored on four rows, problem 1 on none, problem 2 on three of which one is outside the bank
    rows = np.asarray([5, 10 ** 9, ev0[0], ev0[1], ev0[2], ev0[3], ev2[0], n_bank, ev2[1]], np.int32)
    true = np.asarray([0, 0, t0[0], t0[1], 99, t0[3], t2[0], t2[0], -1], np.int32)
    pred, correct, probs, _ = logreg.score_on_device(d_x, rows, true, [2, 6, 6, 9], fit.d_coef, fit.d_intercept, want_probs=True)
    pred, correct, probs = pred.cpu().numpy(), correct.cpu().numpy(), probs.cpu().numpy()
    want0 = logreg.predict_host(c["x"], ev0[:4], fit.coef[0], fit.intercept[0])[0]
    want2 = logreg.predict_host(c["x"], ev2[:2], fit.coef[2], fit.intercept[2])[0]
    assert pred.tolist() == [-1, -1] + want0.tolist() + [want2[0], -1, want2[1]]
    assert np.isnan(probs[[0, 1, 7]]).all() and not np.isnan(probs[[2, 3, 4, 5, 6, 8]]).any()
    assert correct.tolist() == [int(want0[0] == t0[0]) + int(want0[1] == t0[1]) + int(want0[3] == t0[3]), 0, int(want2[0] == t2[0])]
    # no entry at all: the counts are still zeroed by the call
    _, correct, _, _ = logreg.score_on_device(d_x, [], [], [0, 0, 0, 0], fit.d_coef, fit.d_intercept)
    assert correct.cpu().tolist() == [0, 0, 0]
