"""selection_eval.experiment_run_many end to end on the device: 2 experiments x 3 splits on embeddings the synthetic handle makes of
seeded clips, against the same flow through logreg_host / predict_host.  The chosen split and the scores are compared with == after
asserting that every compared row is clear of a decision boundary by more than the two routes can differ."""
import numpy as np
import pytest

from multilingual_kws_amd import logreg
from multilingual_kws_amd.embedding import selection_eval as se

N_TRAIN, N_DEV, N_UNKNOWN = 6, 3, 6
U = 2.0 ** -24


def _bank(torch):
    """Four "words" (a tone each, nine noisy takes) and twelve unknown clips of other tones -> float32 [48, 1024] on the device."""
    from multilingual_kws_amd import synth, weights
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    from multilingual_kws_amd.frontend import Frontend
    takes = [w + 128 * j for w in (5, 30, 60, 100) for j in range(N_TRAIN + N_DEV)] + [10 + 9 * u + 128 * 20 for u in range(2 * N_UNKNOWN)]
    audio = np.concatenate([synth.clips_float32(1, first_clip=t) for t in takes])
    dev = torch.device("cuda:0")
    em = EmbeddingModel(weights.synthetic_blob(), max_batch=len(takes), device=dev)
    emb = em.forward(Frontend().forward(torch.from_numpy(audio).to(dev))).clone()
    em.close()
    return emb


@pytest.mark.gpu
def test_device_flow_equals_the_host_flow():
    torch = pytest.importorskip("torch")
    d_bank = _bank(torch)
    bank = d_bank.cpu().numpy()
    assert bank.shape == (48, 1024) and np.isfinite(bank).all()
    word_rows = [np.arange(w * 9, w * 9 + 9) for w in range(4)]
    ut, ue = np.arange(36, 42), np.arange(42, 48)
    exps = [dict(words=[f"w{w}" for w in ws], train_rows=[word_rows[w][:N_TRAIN] for w in ws], dev_rows=[word_rows[w][N_TRAIN:] for w in ws])
            for ws in ((0, 1, 2), (3, 1, 0))]
    splits = [se.stratified_shuffle_splits(np.repeat([1, 2, 3], N_TRAIN), 3, train_size=12, seed=s) for s in (1, 2)]
    for classifier in ("lr", "lr_scaled"):
        std = se.CLASSIFIERS[classifier]
        # every compared row: clear under the float32 dot-product bound on the device's weights, and clear of the boundary by more than
        # twice the largest logit difference between the device's weights and the host optimum
        K, fit_l, val_l, dev_l, n_splits = se._lists(exps, ut, ue, splits)
        fit = logreg.fit_on_device(d_bank, *fit_l, K, standardize=std, max_iter=300, gtol=1e-6)
        assert (fit.info[:, 0] == 0).all() and K == 4 and n_splits == [3, 3]
        for p in range(6):
            a, b = fit_l[2][p], fit_l[2][p + 1]
            host = logreg.logreg_host(bank, fit_l[0][a:b], fit_l[1][a:b], K, 1.0, std)
            rows = np.concatenate([val_l[0][val_l[2][p]:val_l[2][p + 1]], dev_l[0][dev_l[2][p // 3]:dev_l[2][p // 3 + 1]]])
            x = bank[rows].astype(np.float64)
            z_host = x @ host.coef.T + host.intercept
            z_dev = x @ fit.coef[p].astype(np.float64).T + fit.intercept[p].astype(np.float64)
            gamma = 1025 * U / (1 - 1025 * U)
            bound = gamma * ((np.abs(x)[:, None, :] * np.abs(fit.coef[p].astype(np.float64))[None]).sum(-1) + np.abs(fit.intercept[p])).max(axis=1)
            top_dev, top_host = np.sort(z_dev, axis=1), np.sort(z_host, axis=1)
            # (the intercepts are fixed only up to a constant per problem: differences of logits are what is compared)
            delta = np.abs((z_dev - z_dev[:, :1]) - (z_host - z_host[:, :1])).max(axis=1)
            assert np.all(top_dev[:, -1] - top_dev[:, -2] > 2 * bound), (classifier, p)
            assert np.all(top_host[:, -1] - top_host[:, -2] > 2 * delta), (classifier, p, (top_host[:, -1] - top_host[:, -2]).min(), delta.max())
        on_dev = se.experiment_run_many(d_bank, exps, ut, ue, splits, classifier=classifier)
        on_host = se.experiment_run_many(bank, exps, ut, ue, splits, classifier=classifier, on_device=False)
        assert on_dev == on_host, (classifier, on_dev, on_host)
        assert se.experiment_run_many(bank, exps, ut, ue, splits, classifier=classifier, on_device=True) == on_dev      # a host bank is uploaded
    with pytest.raises(ValueError, match="refused"):
        se.experiment_run_many(d_bank, exps, np.asarray([36, 48]), ue, splits)      # a training row outside the bank
