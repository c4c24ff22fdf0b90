"""The k-means restatement and the host side of the device k-means (multilingual_kws_amd/kmeans.py,
distance_filtering.cluster_and_sort_many) without a GPU: kmeans_host against sklearn, the draws, the wrapper's refusals, the
K-keyword consumer on stub embeddings, the C symbols."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from kmeans_cases import family_case  # noqa: E402

from multilingual_kws_amd import _lib, kmeans  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# largest |sklearn centre - kmeans_host centre| / max |centre| measured over the 40 cases (sklearn 1.7.2, float32 arithmetic there)
MEASURED_CENTRE_DEVIATION = 1.52e-7


@pytest.mark.parametrize("i", range(40))
def test_kmeans_host_is_sklearn(i):
    """Labels, n_iter_ and the k-means++ indices equal sklearn's with ==.  Centres: sklearn works in float32 and adds in another order;
    the largest deviation measured over these 40 cases is 1.52e-7 of max |centre|, and ten times that is allowed."""
    cluster = pytest.importorskip("sklearn.cluster")
    X, k, seed = family_case(i)
    km = cluster.KMeans(n_clusters=k, random_state=seed).fit(X)
    _, indices = cluster.kmeans_plusplus(X, k, random_state=seed)
    got = kmeans.kmeans_host(X, k, seed)
    assert not got.empty and got.smallest >= 1 and got.reason in (0, 1)
    assert got.init.tolist() == indices.tolist()
    assert got.labels.tolist() == km.labels_.tolist() and got.labels.dtype == np.int32
    assert got.n_iter == km.n_iter_
    assert got.centers.dtype == np.float64 and got.centers.shape == (k, X.shape[1])
    deviation = np.abs(km.cluster_centers_ - got.centers).max() / np.abs(got.centers).max()
    print(f"case {i}: centre deviation {deviation:.3e}, min_margin {got.min_margin:.3e}")
    assert deviation <= 10 * MEASURED_CENTRE_DEVIATION
    assert got.min_margin >= 1e-9                  # the condition under which the device run must take the same decisions


def test_draws_are_the_random_state_sequence():
    want = [0.6964691855978616, 0.28613933495037946, 0.2268514535642031, 0.5513147690828912, 0.7194689697855631, 0.42310646012446096,
            0.9807641983846155, 0.6848297385848633, 0.48093190148436094, 0.3921175181941505, 0.3431780161508694, 0.7290497073840416,
            0.4385722446796244]
    got = kmeans.kmeans_draws(123, 5)                                  # 2 + int(log 5) = 3 trials for each of 4 further centres
    assert got.dtype == np.float64 and got.tolist() == want
    assert kmeans.kmeans_draws(123, 1).tolist() == want[:1]
    assert kmeans.kmeans_draws(123, 2).tolist() == want[:3]            # 2 + int(log 2) = 2 trials
    assert [kmeans.n_local_trials(k) for k in (1, 2, 3, 7, 8, 16)] == [2, 2, 3, 3, 4, 4]
    assert kmeans.kmeans_draws(124, 5).tolist() != want


def test_host_stop_reasons_and_empty_cluster():
    X, k, seed = family_case(0)
    one = kmeans.kmeans_host(X, k, seed, max_iter=1)
    assert (one.n_iter, one.reason, one.empty) == (1, 2, False)
    same = kmeans.kmeans_host(np.ones((6, 8), np.float32), 2, 3)
    assert same.empty and same.n_iter == 1 and same.min_margin == 0.0
    every = kmeans.kmeans_host(np.eye(5, 4, dtype=np.float32) + np.arange(5, dtype=np.float32)[:, None], 5, 123)
    assert sorted(every.init.tolist()) == [0, 1, 2, 3, 4] and every.labels.tolist() == np.argsort(every.init).tolist()
    assert (every.n_iter, every.reason) == (1, 1)    # every point is a centre: the labels change from -1, the centres do not move
    with pytest.raises(ValueError):
        kmeans.kmeans_host(X[:4], 5, seed)


def test_wrapper_refusals_come_before_any_upload():
    """numpy input: a refused call never reaches torch.cuda (this test runs without a GPU)."""
    x = np.zeros((40, 8), np.float32)
    fit = kmeans.kmeans_fit_on_device
    for offsets in ([0, 20, 10, 40], [-1, 40], [0, 41], [[0, 40]], [0.0, 40.0], []):
        with pytest.raises(ValueError, match="offsets"):
            fit(x, offsets, 2, 123)
    with pytest.raises(ValueError, match="1 points for 2 clusters"):
        fit(x, [0, 20, 21, 40], 2, 123)                                 # n < k
    with pytest.raises(ValueError, match="at most 1024"):
        fit(np.zeros((1025, 2), np.float32), [0, 1025], 2, 123)
    with pytest.raises(ValueError, match="n_clusters"):
        fit(x, [0, 40], 17, 123)
    with pytest.raises(ValueError, match="n_clusters"):
        fit(x, [0, 40], 0, 123)
    with pytest.raises(ValueError, match="above"):
        fit(np.zeros((40, 1025), np.float32), [0, 40], 16, 123)         # n_clusters * dim
    with pytest.raises(ValueError, match="above"):
        fit(np.zeros((40, 4000), np.float32), [0, 40], 4, 123)          # (n_clusters + 1) * dim
    with pytest.raises(ValueError, match="seeds"):
        fit(x, [0, 20, 40], 2, [1, 2, 3])
    with pytest.raises(ValueError, match="float32"):
        fit(x.astype(np.float64), [0, 40], 2, 123)
    assert kmeans.check_groups([0, 20, 40], 40, 8, 2).dtype == np.int32
    assert (kmeans.MAX_POINTS, kmeans.MAX_CLUSTERS, kmeans.MAX_CENTER_VALUES) == (1024, 16, 16384)


def test_nearest_host_is_the_float64_expression():
    rng = np.random.default_rng(2)
    x, c = rng.standard_normal((9, 33)).astype(np.float32), rng.standard_normal((4, 33)).astype(np.float32)
    c[2] = c[1]
    x[3] = c[1]
    dist, which = kmeans.nearest_host(x, c)
    want = np.sqrt(((c[None].astype(np.float64) - x[:, None].astype(np.float64)) ** 2).sum(-1))
    assert dist.dtype == np.float32 and np.array_equal(dist, want.min(1).astype(np.float32)) and which.tolist() == want.argmin(1).tolist()
    assert dist[3] == 0.0 and which[3] == 1
    assert kmeans.nearest_host(x[:0], c)[0].shape == (0,)


# ------------------------------------------------------------------------------------------------ the K-keyword consumer on stubs

class _StubEmbedding:
    """No device `forward`: cluster_and_sort_many takes the host flow.  feature = fixed random projection of per-channel mean / std."""
    def __init__(self):
        self.P = np.random.default_rng(5).standard_normal((80, 1024)).astype(np.float32)

    def predict(self, specs):
        specs = np.asarray(specs, dtype=np.float32).reshape(len(specs), 49, 40)
        return np.concatenate([specs.mean(1), specs.std(1)], axis=1) @ self.P


def _stub_specs(files, model_settings):
    """One pseudo-spectrogram per file name: 3 families by the number in the name, the spread growing with it (wide distance gaps)."""
    out = []
    for f in files:
        i = int("".join(ch for ch in os.path.basename(str(f)) if ch.isdigit()))
        rng = np.random.default_rng(i)
        out.append(np.full((49, 40), 5.0 + 7.0 * (i % 3), np.float32) + (0.2 + 0.01 * i) * rng.standard_normal((49, 40)).astype(np.float32))
    return np.stack(out) if out else np.zeros((0, 49, 40), np.float32)


def _keywords():
    return [np.array([f"/data/kw{k}/clip{1000 * k + i}.wav" for i in range(n)]) for k, n in enumerate((80, 61, 75))]


def test_cluster_and_sort_many_contract(monkeypatch):
    pytest.importorskip("sklearn")
    from multilingual_kws_amd.embedding import distance_filtering as dfl
    monkeypatch.setattr(dfl, "_specs_for_files", _stub_specs)
    emb, kws, seeds = _StubEmbedding(), _keywords(), [123, 7, 123]
    many = dfl.cluster_and_sort_many(kws, emb, seed=seeds, n_train=50, n_clusters=5)
    assert len(many) == 3
    for files, seed, r in zip(kws, seeds, many):
        assert set(r) == {"sorted_clips", "cluster_centers", "distances", "train_clips", "labels", "n_iter", "nearest", "fallback"}
        single = dfl.cluster_and_sort(files, emb, seed=seed, n_train=50, n_clusters=5)
        assert list(r["train_clips"]) == list(single["train_clips"]) == list(np.random.RandomState(seed).permutation(files)[:50])
        assert set(r["sorted_clips"]) | set(r["train_clips"]) == set(files) and len(r["sorted_clips"]) == len(files) - 50
        assert type(r["sorted_clips"]) is type(single["sorted_clips"]) and r["sorted_clips"].dtype == single["sorted_clips"].dtype
        assert r["cluster_centers"].shape == (5, 1024) and r["cluster_centers"].dtype == single["cluster_centers"].dtype == np.float32
        assert r["distances"].dtype == single["distances"].dtype == np.float32 and np.all(np.diff(r["distances"]) >= 0)
        assert r["labels"].shape == (50,) and r["nearest"].shape == r["distances"].shape and r["fallback"] is False and r["n_iter"] >= 1
        # the distances are the min L2 to the returned centres, the centres are sklearn's on these vectors
        ev = emb.predict(_stub_specs(r["sorted_clips"], None))
        d = np.linalg.norm(r["cluster_centers"][None] - ev[:, None], axis=-1)
        assert np.allclose(d.min(1), r["distances"], rtol=1e-5) and d.argmin(1).tolist() == r["nearest"].tolist()
        assert np.abs(r["cluster_centers"] - single["cluster_centers"]).max() <= 1e-5 * np.abs(single["cluster_centers"]).max()
    again = dfl.cluster_and_sort_many(kws, emb, seed=seeds, n_train=50, n_clusters=5)
    for a, b in zip(many, again):                                                                  # deterministic
        assert list(a["sorted_clips"]) == list(b["sorted_clips"]) and np.array_equal(a["distances"], b["distances"])
    assert dfl.cluster_and_sort_many([], emb) == []
    with pytest.raises(AssertionError):
        dfl.cluster_and_sort_many([kws[0][:50]], emb, n_train=50)
    with pytest.raises(ValueError, match="seeds"):
        dfl.cluster_and_sort_many(kws, emb, seed=[1, 2])


def test_one_keyword_sorts_as_cluster_and_sort(monkeypatch):
    pytest.importorskip("sklearn")
    from multilingual_kws_amd.embedding import distance_filtering as dfl
    monkeypatch.setattr(dfl, "_specs_for_files", _stub_specs)
    emb, files = _StubEmbedding(), _keywords()[0]
    single = dfl.cluster_and_sort(files, emb, seed=123, n_train=50, n_clusters=5)
    gaps = np.diff(single["distances"].astype(np.float64)) / single["distances"][1:]
    assert gaps.min() >= 1e-4                      # wide against float32 rounding (6e-8) and the centre deviation (1.5e-6): no near-tie
    (one,) = dfl.cluster_and_sort_many([files], emb, seed=123, n_train=50, n_clusters=5)
    assert list(one["sorted_clips"]) == list(single["sorted_clips"])
    assert np.allclose(one["distances"], single["distances"], rtol=1e-5)


def test_empty_cluster_goes_through_sklearn(monkeypatch):
    pytest.importorskip("sklearn")
    from multilingual_kws_amd.embedding import distance_filtering as dfl
    monkeypatch.setattr(dfl, "_specs_for_files", lambda files, settings: np.ones((len(files), 49, 40), np.float32))
    files = np.array([f"/data/kw/clip{i}.wav" for i in range(12)])
    with pytest.warns(Warning):                    # sklearn: fewer distinct points than clusters
        (r,) = dfl.cluster_and_sort_many([files], _StubEmbedding(), seed=1, n_train=8, n_clusters=2)
    assert r["fallback"] is True and r["cluster_centers"].shape == (2, 1024) and np.all(r["distances"] < 1e-3)


# ------------------------------------------------------------------------------------------------ the C symbols

def test_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mkws.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, n_args in (("mkws_kmeans_fit", 15), ("mkws_kmeans_nearest", 11)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(L, name), name
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == n_args
        assert getattr(_lib.lib(), name).argtypes == bound[name][1]
    assert bound["mkws_kmeans_fit"][1][8] is ctypes.c_double           # tol
    for macro, value in (("MKWS_KMEANS_MAX_POINTS", 1024), ("MKWS_KMEANS_MAX_CLUSTERS", 16)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", src), macro
    assert _lib.lib().mkws_abi_version() == 5
