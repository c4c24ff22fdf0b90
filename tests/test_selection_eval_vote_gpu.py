"""selection_eval.experiment_run_many(classifier="vote") end to end on the device: 2 experiments x 3 splits on the bank of
tests/test_selection_eval_gpu.py, against the same flow through logreg_host / svc_proba_host / proba_host / soft_vote_host under the same
folds.  The chosen split and the scores are compared with == after asserting that every compared row is clear of its boundary: the
top-two gap of the host's mean probability exceeds twice what the two routes' mean probabilities differ by on that row."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_selection_eval_gpu import N_TRAIN, _bank  # noqa: E402

from multilingual_kws_amd import logreg, svc  # noqa: E402
from multilingual_kws_amd.embedding import selection_eval as se  # noqa: E402


@pytest.mark.gpu
def test_device_flow_equals_the_host_flow():
    torch = pytest.importorskip("torch")
    d_bank = _bank(torch)
    bank = d_bank.cpu().numpy()
    word_rows = [np.arange(w * 9, w * 9 + 9) for w in range(4)]
    ut, ue = np.arange(36, 42), np.arange(42, 48)
    exps = [dict(words=[f"w{w}" for w in ws], train_rows=[word_rows[w][:N_TRAIN] for w in ws], dev_rows=[word_rows[w][N_TRAIN:] for w in ws])
            for ws in ((0, 1, 2), (1, 2, 3))]
    splits = [se.stratified_shuffle_splits(np.repeat([1, 2, 3], N_TRAIN), 3, train_size=12, seed=s) for s in (5, 6)]
    K, fit_l, val_l, dev_l, n_splits = se._lists(exps, ut, ue, splits)
    folds = svc.cv_folds(fit_l[1], fit_l[2], 5, 0)
    lr, sv = se._vote_fit(d_bank, fit_l, K, 1.0, False, None, 1e-6, 1e-5, folds=folds)
    assert (sv.info[:, 0] == 0).all() and (sv.cv_info[:, 0] == 0).all() and (sv.cv_info[:, 2] == 0).all() and K == 4 and n_splits == [3, 3]
    tightest = np.inf
    for p in range(6):
        a, b = fit_l[2][p], fit_l[2][p + 1]
        tr, ty = fit_l[0][a:b], fit_l[1][a:b]
        rows = np.concatenate([val_l[0][val_l[2][p]:val_l[2][p + 1]], dev_l[0][dev_l[2][p // 3]:dev_l[2][p // 3 + 1]]])
        h_lr, h_sv = logreg.logreg_host(bank, tr, ty, K), svc.svc_proba_host(bank, tr, ty, K, folds[a:b], 5)
        mean_host = svc.soft_vote_host(svc.proba_host(bank, rows, tr, ty, K, None, model=h_sv), logreg.predict_host(bank, rows, h_lr.coef, h_lr.intercept)[1])[1]
        lists = (rows, np.zeros(len(rows), np.int64), np.asarray([0, len(rows)]))
        p_lr = logreg.score_on_device(d_bank, *lists, lr.d_coef[p:p + 1].contiguous(), lr.d_intercept[p:p + 1].contiguous(), want_probs=True)[2]
        p_sv = svc.proba_on_device(d_bank, *lists, tr, ty, [0, len(tr)], K, sv.d_coef[a:b].contiguous(), *(t[p:p + 1].contiguous() for t in (
            sv.d_rho, sv.d_gamma, sv.d_centre, sv.d_inv_scale, sv.d_probA, sv.d_probB, sv.d_present)))[2]
        mean_dev = svc.soft_vote_on_device(p_sv, p_lr, lists[1], lists[2], want_mean=True)[2].cpu().numpy().astype(np.float64)
        top = np.sort(mean_host, axis=1)
        gap, apart = top[:, -1] - top[:, -2], np.abs(mean_dev - mean_host).max(axis=1)
        tightest = min(tightest, float((gap / np.maximum(2 * apart, 1e-300)).min()))
        assert np.all(gap > 2 * apart), (p, float(gap.min()), float(apart.max()))
    print(f"the closest row clears its boundary {tightest:.1f} times over")
    on_dev = se.experiment_run_many(d_bank, exps, ut, ue, splits, classifier="vote", folds=folds)
    on_host = se.experiment_run_many(bank, exps, ut, ue, splits, classifier="vote", on_device=False, folds=folds)
    assert on_dev == on_host, (on_dev, on_host)
    assert se.experiment_run_many(bank, exps, ut, ue, splits, classifier="vote", on_device=True) == on_dev       # folds=None draws the same folds
    with pytest.raises(ValueError, match="refused"):
        bad = folds.copy()
        bad[3] = 5
        se.experiment_run_many(d_bank, exps, ut, ue, splits, classifier="vote", folds=bad)
