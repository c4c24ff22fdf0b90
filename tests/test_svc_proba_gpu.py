"""SVC(probability=True) on the device, given the folds (mkws_svc_fit_cv / _platt / _couple, mkws_soft_vote; multilingual_kws_amd/svc.py)
against tests/golden/svc_proba_golden.npz (made on the CPU by tests/golden/make_svc_proba_golden.py; this file reads only it plus NumPy).

Every stage after the folds is convex with a unique answer, so the yardstick is the float64 specification (cv_decision_host, platt_host,
couple_host) and the slack is the reference's own under the SAME folds, with no further margin:

  cv_decision   |dev - cv*| <= max(e_cv, 2^-23 (sum |c*_t| k_t + |rho*|)), e_cv = sklearn's default-tol sub-fits' distance from cv*;
  platt         the float64 gradient at the device's (A, B), on the device's own cv_decision, is at most 2 eps (eps = 1e-8);
  couple        |dev - couple_host| <= max(e_lib, 2^-23 + d), e_lib = libsvm's iteration at 0.005 / K from the exact solve, d = the
                disagreement of the two float64 host methods on the case;
  end to end    |P_dev - P*| <= e_P = |P_sk - P*|, and the prediction is the argmax of P* wherever its top-two gap exceeds 2 e_P.

One fit_proba_on_device(tol=1e-5) call per case (a call has one bank, class count and fold count), shared by the tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from svc_cases import x_hash  # noqa: E402
from svc_proba_cases import CASES, case, libsvm_proba, pair_entries, pairwise, problems  # noqa: E402

from multilingual_kws_amd import _lib, svc  # noqa: E402

TOL, MAX_ITER, EPS = 1e-5, 100000, 1e-8
_GOLDEN, _FIT, _PROBA = [], {}, {}
NAMES = list(CASES)


def golden(golden_dir, name):
    if not _GOLDEN:
        _GOLDEN.append(dict(np.load(os.path.join(golden_dir, "svc_proba_golden.npz"))))
    g = {k.split("/", 1)[1]: v for k, v in _GOLDEN[0].items() if k.startswith(name + "/")}
    assert str(g["x_sha1"]) == x_hash(case(name)) and np.array_equal(g["folds"], case(name)["folds"]), "the fixture is not this case's"
    return g


def fit_case(c, **kw):
    args = dict(folds=c["folds"], n_folds=c["n_folds"], C=c["C"], standardize=c["standardize"], tol=TOL, max_iter=MAX_ITER, platt_eps=EPS)
    args.update(kw)
    return svc.fit_proba_on_device(c["x"], c["rows"], c["labels"], c["offsets"], c["n_classes"], **args)


def fitted(name):
    if name not in _FIT:
        _FIT[name] = fit_case(case(name))
    return _FIT[name]


def proba(name):
    """-> (pred, correct, probs) as numpy arrays: one proba_on_device call on the model of fitted(name)."""
    import torch
    if name not in _PROBA:
        c, fit = case(name), fitted(name)
        d_x = torch.from_numpy(c["x"].copy()).cuda()
        out = svc.proba_on_device(d_x, c["eval_rows"], c["eval_true"], c["eval_offsets"], c["rows"], c["labels"], c["offsets"], c["n_classes"],
                                  fit.d_coef, fit.d_rho, fit.d_gamma, fit.d_centre, fit.d_inv_scale, fit.d_probA, fit.d_probB, fit.d_present,
                                  info=fit.d_info)
        _PROBA[name] = tuple(t.cpu().numpy() for t in out)
    return _PROBA[name]


def fit_bytes(fit):
    return [np.ascontiguousarray(getattr(fit, f)).tobytes() for f in ("coef", "rho", "probA", "probB", "cv_decision", "cv_info", "present", "info")]


# ------------------------------------------------------------------------------------------------ the cross-validated decision values

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_cv_decision_within_the_references_own_slack(name, golden_dir):
    c, g, fit = case(name), golden(golden_dir, name), fitted(name)
    assert (fit.info[:, 0] == 0).all() and (fit.cv_info[:, 0] == 0).all() and (fit.cv_info[:, 2] == 0).all()
    worst = 0.0
    for p, (rows, y, C, _, _, folds, (a, b), _) in enumerate(problems(c)):
        bound = np.maximum(g["e_cv"][p], 2.0 ** -23 * g["cv_weight"][a:b])
        err = np.abs(fit.cv_decision[a:b].astype(np.float64) - g["cv_star"][a:b])
        worst = max(worst, float((err / bound).max()))
        print(f"{name} problem {p}: max error {err.max():.3e}, e_cv {g['e_cv'][p]:.3e}, worst error / bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), (name, p, float(err.max()), float(g["e_cv"][p]))
    # entries that no list names are not written
    outside = np.ones(len(c["rows"]), bool)
    outside[int(c["offsets"][0]):int(c["offsets"][-1])] = False
    assert not fit.cv_decision[outside].any()


@pytest.mark.gpu
def test_all_three_rules_for_a_sub_fit_without_a_class(golden_dir):
    name = "degenerate_1_2_1_10"
    g, fit = golden(golden_dir, name), fitted(name)
    assert (g["rules"] > 0).all()
    ruled = g["cv_weight"] == 0
    assert np.array_equal(fit.cv_decision[ruled].astype(np.float64), g["cv_star"][ruled])
    assert set(np.unique(g["cv_star"][ruled])) == {-1.0, 0.0, 1.0}


# ------------------------------------------------------------------------------------------------ the sigmoids

def host_gradient(dec, sign, A, B):
    return np.abs(svc.platt_objective(dec, sign, A, B)[1]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_platt_gradient_on_the_devices_own_values(name):
    c, fit = case(name), fitted(name)
    K = c["n_classes"]
    worst = 0.0
    for p, (rows, y, C, _, _, folds, (a, b), _) in enumerate(problems(c)):
        seen = set()
        for q, idx, dec, sign, slot in pair_entries(y, K, fit.cv_decision[a:b].astype(np.float64)):
            g = host_gradient(dec, sign, fit.probA[p, q], fit.probB[p, q])
            worst = max(worst, g)
            assert g <= 2 * EPS, (name, p, q, g)
            seen.add(q)
        absent = [q for q in range(K * (K - 1) // 2) if q not in seen]
        assert not fit.probA[p, absent].any() and not fit.probB[p, absent].any()
        assert fit.present[p] == sum(1 << int(k) for k in np.unique(y))
    print(f"{name}: largest |g|_inf {worst:.3e}")


def platt_alone(labels, offsets, K, cv, eps=EPS):
    import torch
    P, npairs = len(offsets) - 1, K * (K - 1) // 2
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (np.asarray(labels, np.int32), np.asarray(offsets, np.int32), np.asarray(cv, np.float32))]
    A, B = torch.full((P, npairs), 7.0, dtype=torch.float64, device="cuda"), torch.full((P, npairs), 7.0, dtype=torch.float64, device="cuda")
    present = torch.zeros(P, dtype=torch.int32, device="cuda")
    biggest = int(np.diff(offsets).max())
    _lib.check(_lib.lib().mkws_svc_platt(d[0].data_ptr(), d[1].data_ptr(), P, K, biggest, d[2].data_ptr(), None, None, eps, A.data_ptr(), B.data_ptr(),
                                         present.data_ptr(), _lib.current_stream_ptr()))
    return A.cpu().numpy(), B.cpu().numpy(), present.cpu().numpy()


@pytest.mark.gpu
def test_platt_alone_on_equal_values_single_entries_and_large_values():
    rng = np.random.default_rng(5)
    probs = []                                                              # (labels, values of the entries in the other class's slot)
    probs.append((np.asarray([0] * 9 + [1] * 4), np.full(13, 0.75)))        # all values equal: only A dec + B is unique
    probs.append((np.asarray([1, 0]), np.asarray([-1.25, 2.0])))            # one entry per class
    y = rng.integers(0, 2, 700)
    probs.append((y, np.where(y == 0, 1.0, -1.0) * rng.uniform(0, 50, 700) + rng.normal(0, 8, 700)))    # |dec| up to 50 and beyond, overlapping
    y = np.arange(300) % 2
    probs.append((y, np.where(y == 0, 30.0, -30.0) + rng.normal(0, 1, 300)))        # separable by a wide margin
    labels = np.concatenate([p[0] for p in probs])
    offsets = np.concatenate([[0], np.cumsum([len(p[0]) for p in probs])])
    cv = np.concatenate([p[1] for p in probs]).astype(np.float32)[:, None]
    A, B, present = platt_alone(labels, offsets, 2, cv)
    assert (present == 3).all()
    for p, (y, _) in enumerate(probs):
        dec = cv[offsets[p]:offsets[p + 1], 0].astype(np.float64)
        sign = np.where(y == 0, 1.0, -1.0)
        g = host_gradient(dec, sign, A[p, 0], B[p, 0])
        As, Bs = svc.platt_host(dec, sign)
        print(f"problem {p}: |g|_inf {g:.3e}, max |z - z*| {np.abs(A[p, 0] * dec + B[p, 0] - (As * dec + Bs)).max():.3e}")
        assert np.isfinite([A[p, 0], B[p, 0]]).all() and g <= 2 * EPS, (p, g)


# ------------------------------------------------------------------------------------------------ pairwise coupling

def couple_alone(decision, true, offsets, probA, probB, present):
    import torch
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    out = svc.couple_on_device(t(decision, np.float32), true, offsets, t(probA, np.float64), t(probB, np.float64), t(present, np.int32))
    return tuple(o.cpu().numpy() for o in out)


@pytest.mark.gpu
@pytest.mark.parametrize("K,present", [(2, 0b11), (3, 0b111), (8, 0xff), (8, 0b10110101), (4, 0b1010)])
def test_couple_alone_against_both_host_methods(K, present):
    rng = np.random.default_rng(K * 1000 + present)
    npairs, n = K * (K - 1) // 2, 80
    classes = np.nonzero([(present >> k) & 1 for k in range(K)])[0]
    live = np.asarray([(present >> i) & 1 and (present >> j) & 1 for i, j in svc.pairs(K)], bool)
    probA, probB = np.where(live, -rng.uniform(0.5, 3.0, npairs), 0.0), np.where(live, rng.normal(0, 0.5, npairs), 0.0)
    dec = (rng.normal(0, 1.5, (n, npairs)) * live).astype(np.float32)
    dec[:20] *= 40.0                                                        # both clip ends: |A f + B| far beyond log(1e7)
    dec[20, :] = np.where(live, 1e4, 0.0)
    dec[21, :] = np.where(live, -1e4, 0.0)
    dec[22, 0] = np.nan
    true = rng.integers(0, K, n)
    pred, correct, probs = couple_alone(dec, true, [0, n], probA[None], probB[None], [present])
    ok = np.ones(n, bool)
    ok[22] = False
    want = svc.couple_host(dec[ok].astype(np.float64), probA, probB, [(present >> k) & 1 for k in range(K)])
    e_lib = np.abs(libsvm_proba(dec[ok].astype(np.float64), probA, probB, classes, K) - want).max(axis=1)
    d = np.zeros(ok.sum())
    for t, row in enumerate(dec[ok].astype(np.float64)):
        if len(classes) > 2:
            d[t] = np.abs(svc.couple_iterative(pairwise(row, probA, probB, classes, K), eps=1e-14)[0] - want[t, classes]).max()
    err = np.abs(probs[ok].astype(np.float64) - want).max(axis=1)
    bound = np.maximum(e_lib, 2.0 ** -23 + d)
    print(f"K {K} present {present:#b}: max error {err.max():.3e}, largest d {d.max():.3e}, smallest bound {bound.min():.3e}")
    assert (err <= bound).all(), (float(err.max()), int(np.argmax(err - bound)))
    assert np.isnan(probs[22]).all() and pred[22] == -1
    assert not probs[ok][:, [k for k in range(K) if k not in classes]].any()
    assert np.array_equal(pred[ok], probs[ok].argmax(axis=1)) and correct[0] == int((pred == true).sum())
    assert np.abs(probs[ok].sum(axis=1) - 1.0).max() <= K * 2.0 ** -23


# ------------------------------------------------------------------------------------------------ end to end

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_probabilities_and_predictions_within_the_references_own_slack(name, golden_dir):
    c, g = case(name), golden(golden_dir, name)
    pred, correct, probs = proba(name)
    assert probs.dtype == np.float32 and pred.dtype == np.int32
    for p, (_, _, _, ev, true, _, _, (ea, eb)) in enumerate(problems(c)):
        P_star, e_p = g["p_star"][ea:eb], float(g["e_p"][p])
        err = np.abs(probs[ea:eb].astype(np.float64) - P_star).max()
        top = np.sort(P_star, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 2 * e_p
        print(f"{name} problem {p}: max |P_dev - P*| {err:.3e}, e_P {e_p:.3e}, clear rows {clear.mean():.2f}")
        assert err <= e_p, (name, p, float(err), e_p)
        assert clear.mean() >= 0.9
        assert np.array_equal(pred[ea:eb][clear], P_star.argmax(axis=1)[clear])
        assert correct[p] == int((pred[ea:eb] == true).sum())


@pytest.mark.gpu
def test_soft_vote_is_the_first_argmax_of_the_mean():
    import torch
    rng = np.random.default_rng(11)
    n, K = 500, 5
    a, b = rng.dirichlet(np.ones(K), n).astype(np.float32), rng.dirichlet(np.ones(K), n).astype(np.float32)
    a[7], b[7] = b[7].copy(), a[7].copy()
    a[3, :], b[3, :] = [0.5, 0.5, 0, 0, 0], [0.5, 0.5, 0, 0, 0]             # an exact tie: the first class
    a[9, 2] = np.nan
    true = rng.integers(0, K, n)
    offsets = [2, 200, 200, 490]                                            # entries in front and behind that no problem owns, an empty problem
    pred, correct, mean = (t.cpu().numpy() for t in svc.soft_vote_on_device(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), true, offsets, True))
    want, mean64 = svc.soft_vote_host(a, b)
    inside = np.zeros(n, bool)
    inside[2:490] = True
    top = np.sort(np.nan_to_num(mean64), axis=1)
    clear = inside & ((top[:, -1] - top[:, -2]) > 2.0 ** -22) & (want >= 0)
    assert clear.sum() > 400 and np.array_equal(pred[clear], want[clear])
    assert pred[3] == 0 and pred[9] == -1 and (pred[~inside] == -1).all()
    assert np.abs(mean[clear].astype(np.float64) - mean64[clear]).max() <= 2.0 ** -24
    assert correct.tolist() == [int((pred[2:200] == true[2:200]).sum()), 0, int((pred[200:490] == true[200:490]).sum())]


# ------------------------------------------------------------------------------------------------ the contract's edges

@pytest.mark.gpu
def test_max_iter_1_is_counted_and_bounded():
    c = case("n12_k3_dim37_f3")
    fit = fit_case(c, max_iter=1)
    assert fit.cv_info[0, 0] == 0 and fit.cv_info[0, 1] > 0 and fit.cv_info[0, 2] == fit.cv_info[0, 1] and fit.cv_info[0, 3] == 1
    assert np.isfinite(fit.cv_decision).all() and np.isfinite(fit.probA).all() and np.isfinite(fit.probB).all()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["label", "fold"])
def test_a_refused_problem_beside_unaffected_neighbours(what):
    c = case("ragged_50_20_64")
    good = fitted("ragged_50_20_64")
    off = c["offsets"]
    labels, folds = c["labels"].copy(), c["folds"].copy()
    if what == "label":
        labels[off[1] + 5] = c["n_classes"]
    else:
        folds[off[1] + 5] = c["n_folds"]
    fit = svc.fit_proba_on_device(c["x"], c["rows"], labels, off, c["n_classes"], folds=folds, n_folds=c["n_folds"], C=c["C"], tol=TOL,
                                  max_iter=MAX_ITER, platt_eps=EPS)
    assert fit.cv_info[:, 0].tolist() == [0, 2, 0] and fit.info[:, 0].tolist() == ([0, 2, 0] if what == "label" else [0, 0, 0])
    assert not fit.cv_decision[off[1]:off[2]].any() and not fit.probA[1].any() and not fit.probB[1].any() and fit.present[1] == 0
    for p in (0, 2):
        for f in ("cv_decision", "coef"):
            assert getattr(fit, f)[off[p]:off[p + 1]].tobytes() == getattr(good, f)[off[p]:off[p + 1]].tobytes()
        for f in ("probA", "probB", "cv_info", "present", "rho"):
            assert getattr(fit, f)[p].tobytes() == getattr(good, f)[p].tobytes()
    if what == "fold":                                                     # the plain fit of the problem is untouched
        assert fit.coef[off[1]:off[2]].tobytes() == good.coef[off[1]:off[2]].tobytes() and fit.rho[1].tobytes() == good.rho[1].tobytes()


@pytest.mark.gpu
def test_two_calls_write_the_same_bytes_and_chunks_change_nothing():
    name = "65_problems_of_8_dim16"
    c, first = case(name), fitted(name)
    assert fit_bytes(fit_case(c)) == fit_bytes(first)
    assert fit_bytes(fit_case(c, work_budget=7 * 8 * 8 * 4)) == fit_bytes(first)       # chunks of seven problems
    import torch
    plain = svc.fit_on_device(c["x"], c["rows"], c["labels"], c["offsets"], c["n_classes"], C=c["C"], tol=TOL, max_iter=MAX_ITER)
    assert plain.coef.tobytes() == first.coef.tobytes() and plain.rho.tobytes() == first.rho.tobytes() and torch.equal(plain.d_info, first.d_info)


@pytest.mark.gpu
def test_no_problem_at_all():
    import torch
    x = np.zeros((4, 8), np.float32)
    fit = svc.fit_proba_on_device(x, [], [], [0], 3)
    assert fit.probA.shape == (0, 3) and fit.cv_decision.shape == (0, 2) and fit.cv_info.shape == (0, 4)
    out = svc.proba_on_device(torch.from_numpy(x).cuda(), [], [], [0], [], [], [0], 3, fit.d_coef, fit.d_rho, fit.d_gamma, fit.d_centre, fit.d_inv_scale,
                              fit.d_probA, fit.d_probB, fit.d_present)
    assert out[0].numel() == 0 and out[1].numel() == 0 and tuple(out[2].shape) == (0, 3)
    e = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
    assert svc.soft_vote_on_device(e, e, [], [0])[0].numel() == 0
