"""k-means on the device (mkws_kmeans_fit / mkws_kmeans_nearest, multilingual_kws_amd/kmeans.py,
distance_filtering.cluster_and_sort_many) against the float64 specification kmeans_host.

Every input first passes test_inputs_leave_wide_margins: kmeans_host took each of its decisions by a relative gap of at least 1e-9 and
met no empty cluster.  A float64 run that adds in another order differs by about dim * 1.1e-16 (1.1e-13 at dim 1024), so it must take the
same decisions: labels, k-means++ indices, iteration counts and stop reasons compare with ==, and the float64 centres within 1e-12 of
max |centre|."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from kmeans_cases import blobs, family_case  # noqa: E402

from multilingual_kws_amd import kmeans  # noqa: E402


def _case(name):
    """-> (groups = [(X float32 [n, dim], seed)], n_clusters, max_iter, tol, rows in front of the first group)."""
    if name == "every_point_a_centre":
        return [(np.eye(5, 4, dtype=np.float32) + np.arange(5, dtype=np.float32)[:, None], 123)], 5, 300, 1e-4, 0
    if name == "n7_k2_dim64":
        X, k, seed = family_case(2)
        return [(X, seed)], k, 300, 1e-4, 0
    if name == "ragged_50_20_64":                                   # offsets 3, 53, 73, 137: no multiple of 64
        return [(blobs(50, 1024, 4, 0.3, 31), 123), (blobs(20, 1024, 2, 1.0, 32), 124), (blobs(64, 1024, 6, 0.05, 33), 7)], 5, 300, 1e-4, 3
    if name == "65_groups_of_8":
        return [(blobs(8, 16, 1, 1.0, 3000 + g), g) for g in range(65)], 2, 300, 1e-4, 0
    if name == "dim37":
        return [(blobs(30, 37, 3, 0.3, 11), 11), (blobs(9, 37, 1, 1.0, 12), 12)], 3, 300, 1e-4, 1
    if name == "caps_n1024_k16_dim1024":
        return [(blobs(1024, 1024, 16, 0.3, 77), 77)], 16, 300, 1e-4, 0
    if name == "stops_on_the_shift":                                # reason 1, after four iterations
        return [(blobs(200, 64, 1, 1.0, 5), 9)], 4, 300, 0.5, 0
    if name == "stops_on_max_iter":                                 # reason 2
        return [(blobs(200, 64, 1, 1.0, 5), 9)], 4, 1, 1e-4, 0
    raise KeyError(name)


CASES = ["every_point_a_centre", "n7_k2_dim64", "ragged_50_20_64", "65_groups_of_8", "dim37", "caps_n1024_k16_dim1024", "stops_on_the_shift",
         "stops_on_max_iter"]
_HOST = {}


def host(name):
    """The specification's answer for every group of a case; computed once and left unchanged."""
    if name not in _HOST:
        groups, k, max_iter, tol, _ = _case(name)
        _HOST[name] = [kmeans.kmeans_host(X, k, seed, max_iter=max_iter, tol=tol) for X, seed in groups]
    return _HOST[name]


def packed(name):
    groups, k, max_iter, tol, lead = _case(name)
    dim = groups[0][0].shape[1]
    x = np.concatenate([np.full((lead, dim), 1e6, np.float32)] + [X for X, _ in groups] + [np.full((2, dim), -1e6, np.float32)])
    offsets = lead + np.concatenate([[0], np.cumsum([len(X) for X, _ in groups])])
    T = kmeans.n_local_trials(k)
    draws = np.stack([kmeans.kmeans_draws(seed, k) for _, seed in groups])
    return x, offsets.astype(np.int32), k, draws, T, max_iter, tol


def raw_fit(torch, x, offsets, k, draws, T, max_iter=300, tol=1e-4, with_optional=True):
    """mkws_kmeans_fit on unchecked arguments -> (code, dict of outputs); every output starts at -9."""
    from multilingual_kws_amd import _lib
    G, (rows, dim) = len(offsets) - 1, x.shape
    d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    d_off = torch.from_numpy(np.asarray(offsets, np.int32)).cuda()
    d_draws = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.float64)).cuda()
    out = dict(centers=torch.full((G, k, dim), -9.0, dtype=torch.float32, device="cuda"),
               centers_f64=torch.full((G, k, dim), -9.0, dtype=torch.float64, device="cuda"),
               labels=torch.full((rows,), -9, dtype=torch.int32, device="cuda"),
               init=torch.full((G, k), -9, dtype=torch.int32, device="cuda"),
               info=torch.full((G, 4), -9, dtype=torch.int32, device="cuda"))
    code = _lib.lib().mkws_kmeans_fit(d_x.data_ptr(), dim, d_off.data_ptr(), G, k, d_draws.data_ptr(), T, max_iter, tol,
                                      out["centers"].data_ptr(), out["centers_f64"].data_ptr() if with_optional else None,
                                      out["labels"].data_ptr(), out["init"].data_ptr() if with_optional else None, out["info"].data_ptr(),
                                      _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return code, {name: t.cpu().numpy() for name, t in out.items()}


def assert_group_is_the_specification(out, g, lo, hi, want):
    assert out["info"][g].tolist() == [0, want.n_iter, want.reason, want.smallest], (g, out["info"][g], want.n_iter, want.reason)
    assert out["init"][g].tolist() == want.init.tolist(), g
    assert out["labels"][lo:hi].tolist() == want.labels.tolist(), g
    scale = np.abs(want.centers).max()
    deviation = np.abs(out["centers_f64"][g] - want.centers).max() / scale
    assert deviation <= 1e-12, (g, deviation)
    rounded = want.centers.astype(np.float32)
    assert np.array_equal(out["centers"][g], out["centers_f64"][g].astype(np.float32)), g       # the float64 result rounded once
    assert np.all(np.abs(out["centers"][g] - rounded) <= np.spacing(np.abs(rounded))), g           # within one ulp of the specification's


# ------------------------------------------------------------------------------------------------ the inputs are worth comparing with ==

@pytest.mark.parametrize("name", CASES)
def test_inputs_leave_wide_margins(name):
    """Host only."""
    want = host(name)
    assert min(w.min_margin for w in want) >= 1e-9 and not any(w.empty for w in want)
    if name == "stops_on_the_shift":
        assert (want[0].n_iter, want[0].reason) == (4, 1)
    if name == "stops_on_max_iter":
        assert (want[0].n_iter, want[0].reason) == (1, 2)
    if name == "every_point_a_centre":
        assert sorted(want[0].init.tolist()) == [0, 1, 2, 3, 4]
    if name == "ragged_50_20_64":
        assert packed(name)[1].tolist() == [3, 53, 73, 137] and {w.reason for w in want} == {0}


# ------------------------------------------------------------------------------------------------ the fit

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_fit_takes_the_decisions_of_kmeans_host(name):
    torch = pytest.importorskip("torch")
    want = host(name)
    assert min(w.min_margin for w in want) >= 1e-9 and not any(w.empty for w in want)
    x, offsets, k, draws, T, max_iter, tol = packed(name)
    code, out = raw_fit(torch, x, offsets, k, draws, T, max_iter, tol)
    assert code == 0
    for g, w in enumerate(want):
        assert_group_is_the_specification(out, g, offsets[g], offsets[g + 1], w)
    assert (out["labels"][:offsets[0]] == -9).all() and (out["labels"][offsets[-1]:] == -9).all()      # rows of no group are not written


@pytest.mark.gpu
def test_wrapper_makes_one_call_of_it():
    torch = pytest.importorskip("torch")
    name = "ragged_50_20_64"
    groups, k, _, _, _ = _case(name)
    x, offsets, _, _, _, _, _ = packed(name)
    want = host(name)
    fit = kmeans.kmeans_fit_on_device(torch.from_numpy(x).cuda(), offsets, k, [s for _, s in groups], want_f64=True)
    out = dict(centers=fit.centers, centers_f64=fit.centers_f64, labels=fit.labels, init=fit.init, info=fit.info)
    for g, w in enumerate(want):
        assert_group_is_the_specification(out, g, offsets[g], offsets[g + 1], w)
    assert (fit.labels[:3] == -1).all() and (fit.labels[137:] == -1).all()
    assert fit.d_centers.is_cuda and np.array_equal(fit.d_centers.cpu().numpy(), fit.centers)
    plain = kmeans.kmeans_fit_on_device(x, offsets, k, [s for _, s in groups])                      # numpy in, no float64 copy
    assert plain.centers_f64 is None and np.array_equal(plain.centers, fit.centers) and np.array_equal(plain.info, fit.info)
    none = kmeans.kmeans_fit_on_device(x, [5], k, [])
    assert none.centers.shape == (0, k, 1024) and none.info.shape == (0, 4) and (none.labels == -1).all()


@pytest.mark.gpu
def test_optional_outputs_may_be_left_out():
    torch = pytest.importorskip("torch")
    x, offsets, k, draws, T, max_iter, tol = packed("dim37")
    code, full = raw_fit(torch, x, offsets, k, draws, T, max_iter, tol)
    code2, lean = raw_fit(torch, x, offsets, k, draws, T, max_iter, tol, with_optional=False)
    assert code == code2 == 0
    for name in ("centers", "labels", "info"):
        assert np.array_equal(full[name], lean[name]), name
    assert (lean["init"] == -9).all() and (lean["centers_f64"] == -9).all()


@pytest.mark.gpu
def test_two_calls_write_the_same_bytes():
    torch = pytest.importorskip("torch")
    for name in ("ragged_50_20_64", "65_groups_of_8"):
        args = packed(name)
        (_, a), (_, b) = raw_fit(torch, *args), raw_fit(torch, *args)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), (name, key)


# ------------------------------------------------------------------------------------------------ status 1 and 2

@pytest.mark.gpu
def test_empty_cluster_and_short_group_are_reported_and_leave_their_neighbours_alone():
    torch = pytest.importorskip("torch")
    name = "dim37"
    groups, k, _, _, _ = _case(name)
    want = host(name)
    same = np.full((6, 37), 2.5, np.float32)                           # identical points: both centres equal, cluster 1 stays empty
    short = blobs(2, 37, 1, 1.0, 13)                                   # 2 points for 3 clusters
    assert kmeans.kmeans_host(same, k, 5).empty
    parts = [groups[0][0], same, short, groups[1][0]]
    x = np.concatenate(parts)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    draws = np.stack([kmeans.kmeans_draws(s, k) for s in (groups[0][1], 5, 6, groups[1][1])])
    code, out = raw_fit(torch, x, offsets, k, draws, kmeans.n_local_trials(k))
    assert code == 0
    assert out["info"][1].tolist() == [1, 1, 0, 0]
    assert out["info"][2].tolist() == [2, 0, 0, 0]
    assert (out["labels"][offsets[2]:offsets[3]] == -9).all() and (out["centers"][2] == -9).all() and (out["init"][2] == -9).all()
    assert_group_is_the_specification(out, 0, offsets[0], offsets[1], want[0])
    assert_group_is_the_specification(out, 3, offsets[3], offsets[4], want[1])
    too_many = np.zeros((1025, 2), np.float32)
    code, out = raw_fit(torch, too_many, [0, 1025], 2, kmeans.kmeans_draws(1, 2)[None], 2)
    assert code == 0 and out["info"][0].tolist() == [2, 0, 0, 0] and (out["labels"] == -9).all()
    code, out = raw_fit(torch, too_many, [7, 3], 2, kmeans.kmeans_draws(1, 2)[None], 2)           # a negative count is a short group
    assert code == 0 and out["info"][0].tolist() == [2, 0, 0, 0] and (out["labels"] == -9).all()


def _write_tone_keyword(tmp_path, name, freqs, n, rng):
    from util_data import tone_clip, write_wav
    files = []
    for i in range(n):
        files.append(str(tmp_path / "clips" / name / f"{name}{i:02d}.wav"))
        write_wav(files[-1], tone_clip(freqs[i % len(freqs)], rng, burst=(2000, 12000)))
    return files


@pytest.mark.gpu
def test_keyword_with_an_empty_cluster_falls_back_to_sklearn(tmp_path):
    pytest.importorskip("sklearn")
    pytest.importorskip("torch")
    import shutil
    from multilingual_kws_amd.embedding import distance_filtering as dfl
    rng = np.random.default_rng(4)
    good = _write_tone_keyword(tmp_path, "good", (500, 900, 1300), 14, rng)
    same = _write_tone_keyword(tmp_path, "same", (700,), 1, rng)
    for i in range(1, 12):                                             # twelve copies of one clip: identical embeddings
        same.append(str(tmp_path / "clips" / "same" / f"copy{i:02d}.wav"))
        shutil.copyfile(same[0], same[-1])
    real = dfl.embedding_model("synthetic", max_batch=16)

    class OneClipPerPass:
        """The real handle, a clip per forward pass: copies of one clip then have equal vectors by construction, whatever a clip's place
        in a batch does to the last bit."""
        max_batch, device, output_dim, checked, predict = real.max_batch, real.device, real.output_dim, real.checked, real.predict

        @staticmethod
        def forward(spec, out):
            for i in range(spec.shape[0]):
                real.forward(spec[i:i + 1], out=out[i:i + 1])
            return out

    emb = OneClipPerPass()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # sklearn: fewer distinct points than clusters
        r_good, r_same = dfl.cluster_and_sort_many([np.array(good), np.array(same)], emb, seed=[1, 2], n_train=8, n_clusters=2)
    assert r_good["fallback"] is False and r_same["fallback"] is True
    assert r_same["cluster_centers"].shape == (2, 1024) and len(r_same["sorted_clips"]) == 4
    vec = dfl.embed_files(r_same["sorted_clips"], emb)
    d = np.linalg.norm(r_same["cluster_centers"][None] - vec[:, None], axis=-1).min(1)
    assert np.allclose(d, r_same["distances"], rtol=1e-5, atol=1e-4 * np.abs(vec).max())
    assert np.all(np.diff(r_good["distances"]) >= 0) and len(r_good["sorted_clips"]) == 6
    real.close()


# ------------------------------------------------------------------------------------------------ nearest

def raw_nearest(torch, x, group, centers, n_groups=None, k=None):
    """mkws_kmeans_nearest on unchecked arguments -> (code, dist, which, invalid); the outputs start at -9."""
    from multilingual_kws_amd import _lib
    rows, dim = x.shape
    G = centers.shape[0] if n_groups is None else n_groups
    k = centers.shape[1] if k is None else k
    d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() if rows else torch.zeros(1, device="cuda")
    d_g = torch.from_numpy(np.asarray(list(group) + [0], np.int32)).cuda()
    d_c = torch.from_numpy(np.ascontiguousarray(centers, dtype=np.float32)).cuda() if centers.size else torch.zeros(1, device="cuda")
    d_dist = torch.full((rows + 1,), -9.0, dtype=torch.float32, device="cuda")
    d_which = torch.full((rows + 1,), -9, dtype=torch.int32, device="cuda")
    d_invalid = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    code = _lib.lib().mkws_kmeans_nearest(d_x.data_ptr(), dim, rows, d_g.data_ptr(), d_c.data_ptr(), G, k, d_dist.data_ptr(),
                                          d_which.data_ptr(), d_invalid.data_ptr(), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    dist, which = d_dist.cpu().numpy(), d_which.cpu().numpy()
    assert dist[rows] == -9 and which[rows] == -9                      # nothing past the last row
    return code, dist[:rows], which[:rows], int(d_invalid.cpu().numpy()[0])


def float64_nearest(x, group, centers):
    """-> (all distances float64 [rows, k], min as float32, first argmin)."""
    c = centers.astype(np.float64)[np.asarray(group)]
    d = np.sqrt(((c - x.astype(np.float64)[:, None]) ** 2).sum(-1))
    return d, d.min(1).astype(np.float32), d.argmin(1).astype(np.int32)


_NEAREST = {}


def nearest_case(rows, k, dim, G=3):
    if (rows, k, dim) not in _NEAREST:
        rng = np.random.default_rng(rows + 7 * k + dim)
        G = 1 if rows == 1 else G
        centers = rng.standard_normal((G, k, dim)).astype(np.float32)
        group = rng.integers(0, G, rows).astype(np.int32)              # shuffled group ids
        x = (centers[group, rng.integers(0, k, rows)] + 0.5 * rng.standard_normal((rows, dim))).astype(np.float32)
        _NEAREST[(rows, k, dim)] = (x, group, centers)
    return _NEAREST[(rows, k, dim)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,k,dim", [(1, 1, 1), (63, 5, 1024), (1025, 5, 1024), (300, 16, 37)])
def test_nearest_is_the_float64_expression(rows, k, dim):
    torch = pytest.importorskip("torch")
    x, group, centers = nearest_case(rows, k, dim)
    d, want, arg = float64_nearest(x, group, centers)
    if k > 1:
        two = np.partition(d, 1, axis=1)[:, :2]
        assert ((two[:, 1] - two[:, 0]) / two[:, 1]).min() >= 1e-9     # no near-tie: the index compares with ==
        assert len(set(group.tolist())) == 3
    code, dist, which, invalid = raw_nearest(torch, x, group, centers)
    assert code == 0 and invalid == 0
    assert which.tolist() == arg.tolist()
    assert np.all(np.abs(dist - want) <= np.spacing(want)), float(np.abs(dist - want).max())
    d_dist, d_which, d_invalid = kmeans.nearest_on_device(torch.from_numpy(x).cuda(), group, torch.from_numpy(centers).cuda())
    assert np.array_equal(d_dist.cpu().numpy(), dist) and np.array_equal(d_which.cpu().numpy(), which) and int(d_invalid.cpu()[0]) == 0
    host_dist, host_which = kmeans.nearest_host(x[group == group[0]], centers[group[0]])
    assert np.all(np.abs(host_dist - dist[group == group[0]]) <= np.spacing(host_dist)) and host_which.tolist() == which[group == group[0]].tolist()


@pytest.mark.gpu
def test_nearest_edges():
    torch = pytest.importorskip("torch")
    x, group, centers = (a.copy() for a in nearest_case(63, 5, 1024))
    centers[1, 3] = centers[1, 2]                                       # two identical centres: the first index
    x[10], group[10] = centers[1, 2], 1
    x[11], group[11] = centers[2, 4], 2                                 # a row equal to a centre: exactly 0.0
    clean = raw_nearest(torch, x, group, centers)
    assert clean[0] == 0 and clean[3] == 0
    assert clean[1][10] == 0.0 and clean[2][10] == 2 and clean[1][11] == 0.0 and clean[2][11] == 4
    bad = group.copy()
    bad[5], bad[40] = -1, 3                                             # group ids -1 and n_groups
    code, dist, which, invalid = raw_nearest(torch, x, bad, centers)
    assert code == 0 and invalid == 2
    assert np.isnan(dist[[5, 40]]).all() and which[[5, 40]].tolist() == [-1, -1]
    keep = np.ones(63, bool)
    keep[[5, 40]] = False
    assert np.array_equal(dist[keep], clean[1][keep]) and np.array_equal(which[keep], clean[2][keep])      # nothing else disturbed
    code, dist, which, invalid = raw_nearest(torch, x, group, centers[:0], n_groups=0, k=5)                 # no group at all
    assert code == 0 and invalid == 63 and np.isnan(dist).all()


# ------------------------------------------------------------------------------------------------ arguments

@pytest.mark.gpu
def test_refused_arguments_and_empty_calls():
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib
    L, s = _lib.lib(), _lib.current_stream_ptr()
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = d.data_ptr()

    def fit(dim=4, n_groups=1, k=2, T=2, max_iter=3, tol=1e-4, holes=()):
        a = [None if i in holes else p for i in range(8)]               # x, offsets, draws, centers, centers_f64, labels, init, info
        return L.mkws_kmeans_fit(a[0], dim, a[1], n_groups, k, a[2], T, max_iter, tol, a[3], a[4], a[5], a[6], a[7], s)

    def nearest(dim=4, rows=1, n_groups=1, k=2, holes=()):
        a = [None if i in holes else p for i in range(6)]               # x, group, centers, dist, which, invalid
        return L.mkws_kmeans_nearest(a[0], dim, rows, a[1], a[2], n_groups, k, a[3], a[4], a[5], s)

    assert fit() == 0                                                   # offsets 0, 0: a group of no points, status 2
    torch.cuda.synchronize()
    assert d[:2].cpu().tolist() == [2, 0]                               # (info is the last buffer written: int32 {2, 0, 0, 0})
    d.zero_()
    for kw in (dict(dim=0), dict(n_groups=-1), dict(k=0), dict(T=0), dict(max_iter=0), dict(tol=-1e-9), dict(tol=float("nan"))):
        assert fit(**kw) == -1, kw
    for hole in (0, 1, 2, 3, 5, 7):
        assert fit(holes=(hole,)) == -1, hole
    assert fit(holes=(4, 6)) == 0                                       # the optional outputs
    assert fit(k=17) == -2 and fit(k=16, dim=1025) == -2 and fit(k=4, dim=4000) == -2 and fit(T=65) == -2
    assert fit(k=16, dim=1024) == 0 and fit(T=64) == 0
    assert fit(n_groups=0, holes=range(8)) == 0                         # nothing launched: the buffers may be NULL
    for kw in (dict(dim=0), dict(rows=-1), dict(n_groups=-1), dict(k=0)):
        assert nearest(**kw) == -1, kw
    for hole in range(6):
        assert nearest(holes=(hole,)) == -1, hole
    assert nearest(n_groups=0, holes=(2,)) == 0                         # no groups: no centres to point at
    assert nearest(k=17) == -2
    assert nearest(rows=0, holes=range(6)) == 0
    assert nearest() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ graph capture

@pytest.mark.gpu
def test_captured_behind_the_embedding_forward():
    """mkws_embed_forward -> mkws_kmeans_nearest recorded in a torch.cuda.graph and replayed twice on changed spectrograms: the eager
    distances."""
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib, weights
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    rng = np.random.default_rng(12)
    B, G, k = 21, 3, 5
    em = EmbeddingModel(weights.synthetic_blob(), max_batch=32)
    first, second = ((rng.integers(0, 670, size=(B, 49, 40)).astype(np.float32) * np.float32(10 / 256)) for _ in range(2))
    base = em.forward(torch.from_numpy(first).cuda())
    d_centers = (base[rng.integers(0, B, G * k)] * 1.01).reshape(G, k, 1024).contiguous()
    d_group = torch.from_numpy(rng.integers(0, G, B).astype(np.int32)).cuda()
    d_spec = torch.from_numpy(first).cuda()
    d_emb = torch.zeros((B, 1024), dtype=torch.float32, device="cuda")
    d_dist = torch.zeros(B, dtype=torch.float32, device="cuda")
    d_which = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_invalid = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def chain():
        s = _lib.current_stream_ptr()
        assert L.mkws_embed_forward(em.h, d_spec.data_ptr(), B, d_emb.data_ptr(), s) == 0
        assert L.mkws_kmeans_nearest(d_emb.data_ptr(), 1024, B, d_group.data_ptr(), d_centers.data_ptr(), G, k, d_dist.data_ptr(),
                                     d_which.data_ptr(), d_invalid.data_ptr(), s) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    seen = []
    for spec in (second, first):
        d_spec.copy_(torch.from_numpy(spec))
        d_dist.fill_(-1)
        d_invalid.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        eager = kmeans.nearest_on_device(em.forward(torch.from_numpy(spec).cuda()), d_group, d_centers)
        assert torch.equal(d_dist, eager[0]) and torch.equal(d_which, eager[1]) and int(d_invalid.cpu()[0]) == 0
        seen.append(d_dist.cpu().numpy())
    assert not np.array_equal(seen[0], seen[1]) and np.isfinite(seen[0]).all() and seen[1].min() > 0
    em.close()


# ------------------------------------------------------------------------------------------------ end to end

@pytest.mark.gpu
def test_cluster_and_sort_many_end_to_end(tmp_path):
    """3 keywords x 24 synthetic WAVs, three tone families each."""
    pytest.importorskip("sklearn")                                      # (the per-keyword cluster_and_sort it is compared with)
    pytest.importorskip("torch")
    from multilingual_kws_amd.embedding import distance_filtering as dfl
    rng = np.random.default_rng(3)
    keywords = [np.array(_write_tone_keyword(tmp_path, f"kw{j}", (500 + 60 * j, 900 + 60 * j, 1300 + 60 * j), 24, rng)) for j in range(3)]
    emb = dfl.embedding_model("synthetic", max_batch=16)               # 45 train clips and 27 eval clips: ragged batches that straddle keywords
    seeds = [1, 2, 3]
    many = dfl.cluster_and_sort_many(keywords, emb, seed=seeds, n_train=15, n_clusters=3)
    assert len(many) == 3
    for files, seed, r in zip(keywords, seeds, many):
        single = dfl.cluster_and_sort(files, emb, seed=seed, n_train=15, n_clusters=3)
        assert list(r["train_clips"]) == list(single["train_clips"])
        assert set(r["sorted_clips"]) | set(r["train_clips"]) == set(files) and len(r["sorted_clips"]) == 9
        assert r["cluster_centers"].shape == (3, 1024) and r["cluster_centers"].dtype == np.float32 and r["distances"].dtype == np.float32
        assert np.all(np.diff(r["distances"]) >= 0)
        vec = dfl.embed_files(r["sorted_clips"], emb)
        d = np.linalg.norm(r["cluster_centers"][None] - vec[:, None], axis=-1)
        assert np.allclose(d.min(1), r["distances"], rtol=1e-5)
        # sorted_clips are the argsort of the returned distances: the eval clips in the split's order, sorted again, give the same list
        perm = np.random.RandomState(seed).permutation(files)[15:]
        by_clip = dict(zip(r["sorted_clips"], r["distances"]))
        assert list(perm[np.argsort(np.asarray([by_clip[c] for c in perm], np.float32))]) == list(r["sorted_clips"])
        assert r["labels"].shape == (15,) and r["nearest"].shape == (9,) and r["fallback"] is False and r["n_iter"] >= 1
    one = dfl.cluster_and_sort_many(keywords[1:2], emb, seed=2, n_train=15, n_clusters=3)[0]
    assert list(one["sorted_clips"]) == list(many[1]["sorted_clips"]) and np.array_equal(one["distances"], many[1]["distances"])
    emb.close()
