"""selection_eval.experiment_run_many with the SVC classifiers end to end on the device: 2 experiments x 3 splits on embeddings the
synthetic handle makes of seeded clips (the bank of tests/test_selection_eval_gpu.py), against the same flow through svc_host /
decision_host / predict_host.  The chosen split and the scores are compared with == after asserting that every compared row is clear of
every pairwise boundary by more than the two routes can differ."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from svc_cases import score_bound  # noqa: E402
from test_selection_eval_gpu import N_TRAIN, _bank  # noqa: E402

from multilingual_kws_amd import svc  # noqa: E402
from multilingual_kws_amd.embedding import selection_eval as se  # noqa: E402


@pytest.mark.gpu
def test_device_flow_equals_the_host_flow():
    torch = pytest.importorskip("torch")
    d_bank = _bank(torch)
    bank = d_bank.cpu().numpy()
    assert bank.shape == (48, 1024) and np.isfinite(bank).all()
    word_rows = [np.arange(w * 9, w * 9 + 9) for w in range(4)]
    ut, ue = np.arange(36, 42), np.arange(42, 48)
    exps = [dict(words=[f"w{w}" for w in ws], train_rows=[word_rows[w][:N_TRAIN] for w in ws], dev_rows=[word_rows[w][N_TRAIN:] for w in ws])
            for ws in ((0, 1, 2), (1, 2, 3))]
    # (these tones embed close together: the word sets and split seeds are ones at which no validation or dev row sits on a boundary)
    splits = [se.stratified_shuffle_splits(np.repeat([1, 2, 3], N_TRAIN), 3, train_size=12, seed=s) for s in (5, 6)]
    for classifier in ("svc", "svc_scaled"):
        std = se.CLASSIFIERS[classifier]
        K, fit_l, val_l, dev_l, n_splits = se._lists(exps, ut, ue, splits)
        fit = svc.fit_on_device(d_bank, *fit_l, K, standardize=std, tol=1e-5)
        assert (fit.info[:, 0] == 0).all() and (fit.info[:, 2] == 0).all() and K == 4 and n_splits == [3, 3]
        # every compared row: |f| of the host optimum above twice (the distance between the device's model and the optimum, both in
        # float64, plus the float32 scorer's bound on the device's model), for every pair
        for p in range(6):
            a, b = fit_l[2][p], fit_l[2][p + 1]
            tr, ty = fit_l[0][a:b], fit_l[1][a:b]
            host = svc.svc_host(bank, tr, ty, K, 1.0, std)
            rows = np.concatenate([val_l[0][val_l[2][p]:val_l[2][p + 1]], dev_l[0][dev_l[2][p // 3]:dev_l[2][p // 3 + 1]]])
            f_host = svc.decision_host(bank, rows, tr, ty, K, host.coef, host.rho, host.gamma, host.centre, host.inv_scale)
            model = (fit.coef[a:b], fit.rho[p], fit.gamma[p], fit.centre[p], fit.inv_scale[p])
            f_dev = svc.decision_host(bank, rows, tr, ty, K, *model)
            bound = np.abs(f_dev - f_host) + score_bound(bank, tr, ty, K, model[0], model[1], rows, *model[3:], model[2])
            assert np.all(np.abs(f_host) > 2 * bound), (classifier, p, np.abs(f_host).min(), bound.max())
        on_dev = se.experiment_run_many(d_bank, exps, ut, ue, splits, classifier=classifier)
        on_host = se.experiment_run_many(bank, exps, ut, ue, splits, classifier=classifier, on_device=False)
        assert on_dev == on_host, (classifier, on_dev, on_host)
        assert se.experiment_run_many(bank, exps, ut, ue, splits, classifier=classifier, on_device=True) == on_dev      # a host bank is uploaded
    with pytest.raises(ValueError, match="refused"):
        se.experiment_run_many(d_bank, exps, np.asarray([36, 48]), ue, splits, classifier="svc")      # a training row outside the bank
