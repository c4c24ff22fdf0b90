"""K RBF support-vector classifiers on the device (mkws_svc_prepare / _kernel / _fit / _score, multilingual_kws_amd/svc.py) against the
golden fixture tests/golden/svc_golden.npz (made on the CPU by tests/golden/make_svc_golden.py; this file reads only it plus NumPy).

The dual is convex and the decision function unique, so the yardstick is the float64 optimum f*: the model the device returns (float32
coefficients, rho, gamma, centre, scale), evaluated in float64 on the host, must satisfy

    |f_dev - f*| <= max(e_sk, 2^-23 * (sum_t |c*_t| k_t + |rho*|))

on every evaluation row and pair, e_sk = max |f_sklearn - f*| of sklearn's default run: the device is at least as converged as the
classifier it replaces, with no further margin; the second term is the float32 storage of the optimum itself and only matters where
sklearn is exact (every alpha at its bound, a handful of rows).  The kernel is held to a forward bound formed from its operands, the
scorer to that bound summed over the coefficients plus the float32 dot-product bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from svc_cases import CASES, U, case, fit_bound, kernel_bound, present_columns, problems, score_bound, x_hash  # noqa: E402

from multilingual_kws_amd import svc  # noqa: E402

TOL, MAX_ITER = 1e-5, 100000
_GOLDEN, _FIT, _SCORE = [], {}, {}


def golden(golden_dir):
    if not _GOLDEN:
        _GOLDEN.append(dict(np.load(os.path.join(golden_dir, "svc_golden.npz"))))
    return _GOLDEN[0]


def fit_case(c, **kw):
    args = dict(C=c["C"], standardize=c["standardize"], tol=TOL, max_iter=MAX_ITER)
    args.update(kw)
    return svc.fit_on_device(c["x"], c["rows"], c["labels"], c["offsets"], c["n_classes"], **args)


def fitted(name):
    """One fit_on_device call per case (all its problems side by side), shared by the tests and left unchanged."""
    if name not in _FIT:
        _FIT[name] = fit_case(case(name))
    return _FIT[name]


def scored(name):
    """-> (pred, correct, decision) as numpy arrays: one score_on_device call per case on the model of fitted(name)."""
    import torch
    if name not in _SCORE:
        c, fit = case(name), fitted(name)
        d_x = torch.from_numpy(c["x"].copy()).cuda()
        out = svc.score_on_device(d_x, c["eval_rows"], c["eval_true"], c["eval_offsets"], c["rows"], c["labels"], c["offsets"], c["n_classes"],
                                  fit.d_coef, fit.d_rho, fit.d_gamma, fit.d_centre, fit.d_inv_scale, info=fit.d_info, want_decision=True)
        _SCORE[name] = tuple(t.cpu().numpy() for t in out)
    return _SCORE[name]


# ------------------------------------------------------------------------------------------------ the kernel

@pytest.mark.gpu
@pytest.mark.parametrize("name,standardize", [("k6_n200_raw", False), ("k6_n200_scaled", True), ("n12_k3_dim37", False)])
def test_kernel_within_its_forward_bound(name, standardize):
    torch = pytest.importorskip("torch")
    c = case(name)
    rows = c["rows"][int(c["offsets"][0]):int(c["offsets"][1])].astype(np.int64)
    centre, inv, gamma = svc.scaling(c["x"], rows, standardize)
    centre, inv, gamma = centre.astype(np.float32), inv.astype(np.float32), float(np.float32(gamma))
    d_x = torch.from_numpy(c["x"].copy()).cuda()
    n = len(rows)
    lists = [(rows[:min(n, 70)], rows[:min(n, 70)])]                                   # A = B: the diagonal
    if n >= 130:
        lists += [(rows[:33], rows[20:37]), (rows[:130], rows[60:130]), (rows[100:117], rows[3:36])]   # longer than one tile, both ways
    else:
        lists += [(rows[:7], rows[3:12])]
    for ra, rb in lists:
        got = svc.kernel_on_device(d_x, ra, rb, centre, inv, gamma).cpu().numpy()
        want, bound = kernel_bound(c["x"], ra, rb, centre, inv, gamma)
        assert got.shape == want.shape and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - want)
        print(f"{name} {len(ra)} x {len(rb)}: max err {err.max():.3e}, largest share of the bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), (name, len(ra), len(rb), err.max(), (err / bound).max())
        if ra is rb or np.array_equal(ra, rb):
            assert np.diag(got).max() <= 1.0 and np.array_equal(got, got.T)
    # a row outside the bank is not read: NaN in its row or column, the others untouched
    ra, rb = np.asarray([rows[0], c["x"].shape[0], rows[1]]), np.asarray([rows[2], -1])
    got = svc.kernel_on_device(d_x, ra, rb, centre, inv, gamma).cpu().numpy()
    assert np.isnan(got[1]).all() and np.isnan(got[:, 1]).all() and not np.isnan(got[[0, 2], 0]).any()
    assert svc.kernel_on_device(d_x, [], rb, centre, inv, gamma).shape == (0, 2)


# ------------------------------------------------------------------------------------------------ the fit

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_is_at_least_as_converged_as_sklearn(name, golden_dir):
    pytest.importorskip("torch")
    g, c = golden(golden_dir), case(name)
    assert str(g[name + "/x_sha1"]) == x_hash(c)
    K, dim = c["n_classes"], c["x"].shape[1]
    fit = fitted(name)
    P, npairs = len(c["offsets"]) - 1, K * (K - 1) // 2
    assert fit.coef.shape == (len(c["rows"]), K - 1) and fit.coef.dtype == np.float32 and fit.rho.shape == (P, npairs)
    assert fit.gamma.shape == (P,) and fit.centre.shape == (P, dim) and fit.inv_scale.shape == (P, dim) and fit.info.shape == (P, 4) and fit.gap.shape == (P,)
    worst, most = 0.0, 0
    for p, (rows, y, C, ev_rows, _) in enumerate(problems(c)):
        lo, elo, ehi = int(c["offsets"][p]), int(c["eval_offsets"][p]), int(c["eval_offsets"][p + 1])
        cols = present_columns(y, K)
        status, n_pairs, n_cut, n_iter = fit.info[p].tolist()
        assert status == 0 and n_pairs == len(cols) and n_cut == 0 and 1 <= n_iter <= MAX_ITER and 0 <= fit.gap[p] < TOL, (name, p, fit.info[p], fit.gap[p])
        mu, inv, gamma = svc.scaling(c["x"], rows, c["standardize"])
        assert abs(gamma - g[name + "/gamma_star"][p]) <= 1e-12 * gamma
        assert abs(float(fit.gamma[p]) - gamma) <= 2 * U * gamma
        assert np.abs(fit.centre[p] - mu).max() <= U * max(np.abs(mu).max(), 1e-30) and np.abs(fit.inv_scale[p] - inv).max() <= 2 * U * np.abs(inv).max()
        coef = fit.coef[lo:lo + len(rows)]
        f_dev = svc.decision_host(c["x"], ev_rows, rows, y, K, coef, fit.rho[p], fit.gamma[p], fit.centre[p], fit.inv_scale[p])
        f_star, e_sk = g[name + "/f_star"][elo:ehi], float(g[name + "/e_sk"][p])
        bound = fit_bound(c["x"], rows, y, K, g[name + "/coef_star"][lo:lo + len(rows)], g[name + "/rho_star"][p], ev_rows, e_sk, c["standardize"])
        err = np.abs(f_dev - f_star)
        if P <= 3:
            print(f"{name} problem {p}: iterations {n_iter}, gap {fit.gap[p]:.2e}, max |f_dev - f*| {err.max():.3e} (sklearn {e_sk:.3e}), "
                  f"largest share of the bound {(err[:, cols] / bound[:, cols]).max():.3f}")
        worst, most = max(worst, float((err[:, cols] / bound[:, cols]).max())), max(most, n_iter)
        assert (err[:, cols] <= bound[:, cols]).all(), (name, p, err.max(), e_sk, (err[:, cols] / bound[:, cols]).max())
        # the layout: a pair with an absent class carries nothing; y'alpha = 0 per pair; 0 <= alpha <= C with class i positive
        absent = [q for q in range(npairs) if q not in cols]
        assert not f_dev[:, absent].any() and not fit.rho[p][absent].any()
        for i, j in svc.pairs(K):
            ci, cj = coef[y == i, svc._slot(i, j)].astype(np.float64), coef[y == j, svc._slot(j, i)].astype(np.float64)
            assert (ci >= 0).all() and (ci <= np.float32(C)).all() and (cj <= 0).all() and (cj >= -np.float32(C)).all()
            assert abs(ci.sum() + cj.sum()) <= 4 * U * (np.abs(ci).sum() + np.abs(cj).sum()) + 1e-30
    print(f"{name}: P = {P}, largest share of the bound {worst:.3f}, most iterations of a pair {most}")
    # what no offset names is not written
    named = np.zeros(len(c["rows"]), bool)
    for a, b in zip(c["offsets"][:-1], c["offsets"][1:]):
        named[a:b] = True
    assert not fit.coef[~named].any()                 # (zero prefill; on canary-filled outputs: tests/test_dataperf_fenced_gpu.py)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged_50_20_64", "65_problems_of_8_dim16", "k6_n200_scaled", "caps_n1024_k8_dim1024"])
def test_two_calls_write_equal_bytes(name):
    pytest.importorskip("torch")
    first, again = fitted(name), fit_case(case(name))
    for a, b in zip(first[:7], again[:7]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name,budget", [("65_problems_of_8_dim16", 8 * 8 * 4 * 7), ("ragged_50_20_64", 1), ("c_0p01_1_100", 60 * 60 * 4 * 2)])
def test_chunked_calls_give_what_one_call_gives(name, budget):
    pytest.importorskip("torch")
    c = case(name)
    n_chunks = len(svc.chunks(c["offsets"], budget))
    assert n_chunks == {"65_problems_of_8_dim16": 10, "ragged_50_20_64": 3, "c_0p01_1_100": 2}[name]
    first, again = fitted(name), fit_case(c, work_budget=budget)
    for a, b in zip(first[:7], again[:7]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_one_iteration_is_counted_and_flagged():
    """max_iter = 1: status 0, every pair cut, one iteration counted, a gap above tol, and one two-variable step taken per pair."""
    pytest.importorskip("torch")
    c = case("c_0p01_1_100")
    fit = fit_case(c, max_iter=1)
    for p, (rows, y, C, _, _) in enumerate(problems(c)):
        assert fit.info[p].tolist() == [0, 3, 3, 1] and fit.gap[p] >= TOL
        coef = fit.coef[int(c["offsets"][p]):int(c["offsets"][p + 1])]
        for i, j in svc.pairs(3):
            assert np.count_nonzero(coef[y == i, svc._slot(i, j)]) == 1 and np.count_nonzero(coef[y == j, svc._slot(j, i)]) == 1


@pytest.mark.gpu
def test_bad_problems_get_status_2_beside_unaffected_neighbours():
    torch = pytest.importorskip("torch")
    c, good = case("ragged_50_20_64"), fitted("ragged_50_20_64")
    off = c["offsets"].tolist()
    n_bank = c["x"].shape[0]
    for what in ("empty", "label", "negative label", "row", "negative row", "one class"):
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
        elif what == "negative row":
            rows[off[1]] = -1
        else:
            labels[off[1]:off[2]] = 2
        fit = svc.fit_on_device(c["x"], rows, labels, offsets, c["n_classes"], C=c["C"], tol=TOL, max_iter=MAX_ITER)
        assert fit.info[1].tolist() == [2, 0, 0, 0], (what, fit.info[1])
        lo, hi = offsets[1], offsets[2]
        # (the wrapper's zero prefill is still there; tests/test_dataperf_fenced_gpu.py asks the same of canary-filled outputs, where a written zero shows)
        assert not fit.coef[lo:hi].any() and not fit.rho[1].any() and not fit.centre[1].any() and fit.gamma[1] == 0 and fit.gap[1] == 0, what
        shift = offsets[3] - off[3]
        for p, (a, b) in ((0, (off[0], off[1])), (2, (off[2], off[3]))):
            s = shift if p == 2 else 0
            assert fit.coef[a + s:b + s].tobytes() == good.coef[a:b].tobytes() and fit.info[p].tolist() == good.info[p].tolist(), (what, p)
            assert fit.rho[p].tobytes() == good.rho[p].tobytes() and fit.gamma[p] == good.gamma[p] and fit.gap[p] == good.gap[p]
        if what == "row":
            # the scorer leaves a refused model's rows at -1 and counts nothing for it
            d_x = torch.from_numpy(c["x"].copy()).cuda()
            pred, correct, dec = svc.score_on_device(d_x, c["eval_rows"], c["eval_true"], c["eval_offsets"], rows, labels, offsets, c["n_classes"], fit.d_coef,
                                                     fit.d_rho, fit.d_gamma, fit.d_centre, fit.d_inv_scale, info=fit.d_info, want_decision=True)
            ev = c["eval_offsets"]
            assert (pred[ev[1]:ev[2]] == -1).all().item() and correct[1].item() == 0 and torch.isnan(dec[ev[1]:ev[2]]).all().item()
            assert np.array_equal(pred[:ev[1]].cpu().numpy(), scored("ragged_50_20_64")[0][:ev[1]])


@pytest.mark.gpu
def test_refused_arguments_and_no_problem():
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib
    c = case("n12_k3_dim37")
    empty = svc.fit_on_device(c["x"], [], [], [0], 3)
    assert empty.coef.shape == (0, 2) and empty.info.shape == (0, 4) and empty.rho.shape == (0, 3) and empty.gap.shape == (0,)
    for bad in (dict(C=0.0), dict(C=-1.0), dict(C=float("nan")), dict(max_iter=0), dict(tol=-1.0), dict(gamma=float("inf")), dict(work_budget=0)):
        with pytest.raises(ValueError):
            fit_case(c, **bad)
    with pytest.raises(ValueError):
        svc.fit_on_device(c["x"], c["rows"], c["labels"], c["offsets"], 9)
    with pytest.raises(ValueError):
        svc.fit_on_device(c["x"], c["rows"], c["labels"][:-1], c["offsets"], 3)
    with pytest.raises(ValueError):
        svc.fit_on_device(c["x"], c["rows"], c["labels"], [0, 13], 3)
    L = _lib.lib()
    assert L.mkws_svc_work_bytes(3, 50) == 3 * 50 * 50 * 4 and L.mkws_svc_work_bytes(0, 50) == 0
    d_x = torch.from_numpy(c["x"].copy()).cuda()
    d_rows, d_y, d_off = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("rows", "labels", "offsets"))
    d_C = torch.ones(1, dtype=torch.float64, device="cuda")
    out = torch.zeros(4096, dtype=torch.float32, device="cuda")
    d_info = torch.zeros(4, dtype=torch.int32, device="cuda")
    ptr = lambda k: out.data_ptr() + 4 * k

    def prepare(K=3, dim=37, max_rows=12, standardize=0, gamma=0.0, P=1, centre=ptr(0)):
        return L.mkws_svc_prepare(d_x.data_ptr(), c["x"].shape[0], dim, d_rows.data_ptr(), d_y.data_ptr(), d_off.data_ptr(), P, K, max_rows, standardize, gamma,
                                  centre, ptr(64), ptr(128), d_info.data_ptr(), ptr(129), None)

    def gram(dim=37, max_rows=12, stride=144, P=1, work=ptr(256)):
        return L.mkws_svc_kernel(d_x.data_ptr(), c["x"].shape[0], dim, d_rows.data_ptr(), d_off.data_ptr(), max_rows, d_rows.data_ptr(), d_off.data_ptr(), max_rows,
                                 P, ptr(0), ptr(64), ptr(128), d_info.data_ptr(), work, stride, None)

    def smo(K=3, max_rows=12, tol=1e-5, max_iter=100, stride=144, P=1, coef=ptr(512)):
        return L.mkws_svc_fit(d_y.data_ptr(), d_off.data_ptr(), P, K, max_rows, d_C.data_ptr(), tol, max_iter, ptr(256), stride, coef, ptr(600), d_info.data_ptr(),
                              ptr(129), None)

    assert prepare(K=1) == -1 and prepare(K=9) == -2 and prepare(dim=0) == -1 and prepare(dim=1025) == -2 and prepare(max_rows=0) == -1
    assert prepare(max_rows=1025) == -2 and prepare(standardize=2) == -1 and prepare(gamma=float("nan")) == -1 and prepare(P=-1) == -1 and prepare(centre=None) == -1
    assert gram(dim=0) == -1 and gram(stride=143) == -1 and gram(work=None) == -1 and gram(P=-1) == -1
    assert smo(K=1) == -1 and smo(K=9) == -2 and smo(max_iter=0) == -1 and smo(tol=-1.0) == -1 and smo(tol=float("nan")) == -1 and smo(stride=143) == -1
    assert smo(coef=None) == -1 and smo(max_rows=1025) == -2
    assert prepare(P=0) == 0 and gram(P=0) == 0 and smo(P=0) == 0
    torch.cuda.synchronize()
    assert not out.any().item() and not d_info.any().item()           # a refused call writes nothing
    assert prepare() == 0 and gram() == 0 and smo() == 0
    torch.cuda.synchronize()
    want = fitted("n12_k3_dim37")
    assert d_info.cpu().tolist() == want.info[0].tolist()
    assert out[512:512 + 24].cpu().numpy().tobytes() == want.coef.tobytes() and out[600:603].cpu().numpy().tobytes() == want.rho.tobytes()
    with pytest.raises(ValueError):
        svc.score_on_device(d_x, [0], [0], [0, 1], c["rows"], c["labels"], c["offsets"], 3, want.d_coef, want.d_rho[:, :2], want.d_gamma, want.d_centre,
                            want.d_inv_scale)


# ------------------------------------------------------------------------------------------------ the scorer

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_score_is_the_models_float64_value_within_its_bound_and_votes(name, golden_dir):
    pytest.importorskip("torch")
    g, c, fit = golden(golden_dir), case(name), fitted(name)
    K = c["n_classes"]
    pred, correct, dec = scored(name)
    assert pred.dtype == np.int32 and dec.shape == (len(c["eval_rows"]), K * (K - 1) // 2)
    worst = 0.0
    for p, (rows, y, C, ev_rows, ev_true) in enumerate(problems(c)):
        lo, elo, ehi = int(c["offsets"][p]), int(c["eval_offsets"][p]), int(c["eval_offsets"][p + 1])
        cols = present_columns(y, K)
        coef, rho, gamma, centre, inv = fit.coef[lo:lo + len(rows)], fit.rho[p], fit.gamma[p], fit.centre[p], fit.inv_scale[p]
        f64 = svc.decision_host(c["x"], ev_rows, rows, y, K, coef, rho, gamma, centre, inv)
        s_bound = score_bound(c["x"], rows, y, K, coef, rho, ev_rows, centre, inv, gamma)
        err = np.abs(dec[elo:ehi].astype(np.float64) - f64)
        worst = max(worst, float((err[:, cols] / s_bound[:, cols]).max()))
        assert (err[:, cols] <= s_bound[:, cols]).all(), (name, p, err.max(), (err[:, cols] / s_bound[:, cols]).max())
        absent = [q for q in range(dec.shape[1]) if q not in cols]
        assert not dec[elo:ehi][:, absent].any()
        # the votes: equal to the float64 optimum's on every row clear of every boundary by twice what fit and scorer may differ by
        f_star, e_sk = g[name + "/f_star"][elo:ehi], float(g[name + "/e_sk"][p])
        f_bound = fit_bound(c["x"], rows, y, K, g[name + "/coef_star"][lo:lo + len(rows)], g[name + "/rho_star"][p], ev_rows, e_sk, c["standardize"])
        clear = (np.abs(f_star[:, cols]) > 2 * (f_bound + s_bound)[:, cols]).all(axis=1)
        assert clear.mean() >= 0.9, (name, p, clear.mean())
        want = svc.predict_host(f_star, y, K)
        assert np.array_equal(pred[elo:ehi][clear], want[clear]), (name, p)
        assert np.array_equal(pred[elo:ehi], svc.predict_host(dec[elo:ehi], y, K))             # the vote over its own decision values
        assert np.isin(pred[elo:ehi], np.unique(y)).all()                                       # a class with no row is never predicted
        assert correct[p] == int((pred[elo:ehi] == ev_true).sum())
    print(f"{name}: largest share of the scorer's bound {worst:.3f}")


@pytest.mark.gpu
def test_score_lists_are_each_problems_own_and_bad_entries_are_not_read():
    torch = pytest.importorskip("torch")
    c, fit = case("ragged_50_20_64"), fitted("ragged_50_20_64")
    pred_all = scored("ragged_50_20_64")[0]
    d_x = torch.from_numpy(c["x"].copy()).cuda()
    n_bank = c["x"].shape[0]
    ev = c["eval_offsets"]
    ev0, t0 = c["eval_rows"][ev[0]:ev[1]], c["eval_true"][ev[0]:ev[1]]
    ev2, t2 = c["eval_rows"][ev[2]:ev[3]], c["eval_true"][ev[2]:ev[3]]
    want0, want2 = pred_all[ev[0]:ev[1]], pred_all[ev[2]:ev[3]]
    # two leading entries that no list names; problem 0 scored on four rows, problem 1 on none, problem 2 on three of which one is outside the bank
    rows = np.asarray([5, 10 ** 9, ev0[0], ev0[1], ev0[2], ev0[3], ev2[0], n_bank, ev2[1]], np.int32)
    true = np.asarray([0, 0, t0[0], t0[1], 99, t0[3], t2[0], t2[0], -1], np.int32)
    args = (c["rows"], c["labels"], c["offsets"], c["n_classes"], fit.d_coef, fit.d_rho, fit.d_gamma, fit.d_centre, fit.d_inv_scale)
    pred, correct, dec = svc.score_on_device(d_x, rows, true, [2, 6, 6, 9], *args, want_decision=True)
    pred, correct, dec = pred.cpu().numpy(), correct.cpu().numpy(), dec.cpu().numpy()
    assert pred.tolist() == [-1, -1] + want0[:4].tolist() + [want2[0], -1, want2[1]]
    assert np.isnan(dec[[0, 1, 7]]).all() and not np.isnan(dec[[2, 3, 4, 5, 6, 8]]).any()
    assert correct.tolist() == [int(want0[0] == t0[0]) + int(want0[1] == t0[1]) + int(want0[3] == t0[3]), 0, int(want2[0] == t2[0])]
    only_pred, only_correct, none = svc.score_on_device(d_x, rows, true, [2, 6, 6, 9], *args)
    assert none is None and np.array_equal(only_pred.cpu().numpy(), pred) and np.array_equal(only_correct.cpu().numpy(), correct)
    # no entry at all: the counts are still zeroed by the call
    _, correct, _ = svc.score_on_device(d_x, [], [], [0, 0, 0, 0], *args)
    assert correct.cpu().tolist() == [0, 0, 0]
