"""k-means of the MSWC outlier filter: the specification (kmeans_host) and the host wrappers over mkws_kmeans_fit / mkws_kmeans_nearest
(include/mkws.h).

kmeans_host restates, in float64 NumPy on widened float32 points, what sklearn.cluster.KMeans(n_clusters=k, random_state=seed).fit(X)
does: mean-centring, greedy k-means++ with 2 + int(log k) local trials drawn from RandomState(seed), Lloyd with sklearn's two stopping
rules, the final E-step (tests/test_kmeans_cpu.py holds it to sklearn).  The random draws do not depend on the data, so the host makes
them (kmeans_draws) and the device runs everything else.  An empty cluster in a Lloyd step is not restated -- sklearn relocates a centre
there -- it is reported, and the caller runs sklearn for that group.

Every decision kmeans_host takes has a margin: the relative gap by which it was taken.  A float64 run that adds in another order (the
device's wave butterflies; error about dim * 1.1e-16 relative) takes the same decisions whenever min_margin is far above that, which is
why tests/test_kmeans_gpu.py compares labels, indices and iteration counts with == after asserting min_margin >= 1e-9."""
from collections import namedtuple

import numpy as np

from . import _lib, problems

MAX_POINTS = 1024             # MKWS_KMEANS_MAX_POINTS
MAX_CLUSTERS = 16             # MKWS_KMEANS_MAX_CLUSTERS
MAX_CENTER_VALUES = 16384     # MKWS_KMEANS_MAX_CENTER_VALUES: n_clusters * dim
MAX_LDS_VALUES = 17408        # MKWS_KMEANS_MAX_LDS_VALUES: (n_clusters + 1) * dim
MAX_TRIALS = 64               # MKWS_KMEANS_MAX_TRIALS

KMeansHost = namedtuple("KMeansHost", "centers labels init n_iter reason empty min_margin smallest")
KMeansFit = namedtuple("KMeansFit", "centers centers_f64 labels init info d_centers")


def n_local_trials(n_clusters):
    return 2 + int(np.log(n_clusters))


def kmeans_draws(seed, n_clusters):
    """The uniforms KMeans(random_state=seed) consumes, in its order: float64 [1 + (n_clusters - 1) * trials] = u0 (the first centre),
    then for every further centre its `trials` candidates."""
    rs = np.random.RandomState(seed)
    trials = n_local_trials(n_clusters)
    out = [np.asarray([rs.random_sample()])]
    for _ in range(1, n_clusters):
        out.append(rs.uniform(size=trials))
    return np.concatenate(out).astype(np.float64)


def _gap(lower, upper):
    """Relative gap of a decision lower <= upper."""
    scale = max(abs(float(lower)), abs(float(upper)))
    return 1.0 if scale == 0.0 and lower == upper else 0.0 if scale == 0.0 else (float(upper) - float(lower)) / scale


def _assign(Xc, C):
    """(labels = first argmin of |Xc - C|^2, smallest relative gap between a point's nearest and second-nearest centre)."""
    D = np.stack([((Xc - c) ** 2).sum(axis=1) for c in C], axis=1)
    labels = D.argmin(axis=1)
    margin = 1.0
    if C.shape[0] > 1:
        two = np.partition(D, 1, axis=1)[:, :2]
        scale = np.maximum(two[:, 1], np.finfo(np.float64).tiny)
        margin = float(((two[:, 1] - two[:, 0]) / scale).min())
    return labels, margin


def kmeans_host(X, n_clusters, seed, max_iter=300, tol=1e-4):
    """-> KMeansHost(centers float64 [k, dim], labels, init (the rows k-means++ picked), n_iter, reason (0 labels unchanged, 1 centre
    shift <= tolerance, 2 max_iter), empty (a Lloyd step met an empty cluster: the other fields are then not sklearn's), min_margin (the
    smallest relative gap of any decision taken: assignment argmins, candidate-potential argmins over distinct candidates, searchsorted
    boundaries relative to the potential, the shift <= tolerance tests), smallest (cluster size))."""
    X = np.asarray(X, dtype=np.float64)
    n, k = X.shape[0], int(n_clusters)
    if X.ndim != 2 or k < 1 or n < k:
        raise ValueError(f"{X.shape} points for {k} clusters")
    draws = kmeans_draws(seed, k)
    T = n_local_trials(k)
    mean = X.mean(axis=0)
    Xc = X - mean
    tol_abs = np.mean(np.var(Xc, axis=0)) * tol
    margin = 1.0
    # greedy k-means++.  The first index: RandomState.choice(n, p = 1 / n); the device forms the same bits in the same order, so this
    # boundary has no margin to take
    cdf = np.cumsum(np.full(n, 1.0 / n))
    cdf /= cdf[-1]
    first = min(int(np.searchsorted(cdf, draws[0], side="right")), n - 1)
    init = [first]
    closest = ((Xc - Xc[first]) ** 2).sum(axis=1)
    pot = closest.sum()
    for c in range(1, k):
        vals = draws[1 + (c - 1) * T:1 + c * T] * pot
        cs = np.cumsum(closest)                                      # sequential, float64
        raw = np.searchsorted(cs, vals)                              # side="left"
        for v, i in zip(vals, raw):
            below = cs[i - 1] if i > 0 else -np.inf
            above = cs[i] if i < n else np.inf
            if pot > 0:
                margin = min(margin, (min(above - v, v - below)) / pot)
            else:
                margin = 0.0
        cand = np.minimum(raw, n - 1)
        dc = [np.minimum(closest, ((Xc - Xc[j]) ** 2).sum(axis=1)) for j in cand]
        pots = np.asarray([d.sum() for d in dc])
        b = int(pots.argmin())
        distinct = sorted({int(j): float(p) for j, p in zip(cand, pots)}.values())
        if len(distinct) > 1:
            margin = min(margin, _gap(distinct[0], distinct[1]))
        init.append(int(cand[b]))
        closest, pot = dc[b], pots[b]
    C = Xc[init].copy()
    # Lloyd
    labels_old = np.full(n, -1)
    labels, n_iter, reason, empty = labels_old, 0, 2, False
    for it in range(int(max_iter)):
        labels, m = _assign(Xc, C)
        margin = min(margin, m)
        n_iter = it + 1
        counts = np.bincount(labels, minlength=k)
        if (counts == 0).any():
            empty = True
            break
        Cn = np.stack([Xc[labels == c].sum(axis=0) / counts[c] for c in range(k)])
        shift = ((Cn - C) ** 2).sum()
        C = Cn
        if np.array_equal(labels, labels_old):
            reason = 0
            break
        margin = min(margin, _gap(*sorted((float(shift), float(tol_abs)))))
        if shift <= tol_abs:
            reason = 1
            break
        labels_old = labels
    if not empty:
        labels, m = _assign(Xc, C)
        margin = min(margin, m)
    smallest = int(np.bincount(labels, minlength=k).min())
    return KMeansHost(C + mean, labels.astype(np.int32), np.asarray(init, np.int32), n_iter, 0 if empty else reason, empty, float(margin), smallest)


def nearest_host(x, centers):
    """The expression mkws_kmeans_nearest evaluates, for one group: x float32 [rows, dim], centers float32 [k, dim]
    -> (float32 distances to the nearest centre, its first index); the minimum is taken on the float64 values."""
    x, c = np.asarray(x, np.float32).astype(np.float64), np.asarray(centers, np.float32).astype(np.float64)
    d = np.sqrt(np.stack([((cc - x) ** 2).sum(axis=1) for cc in c], axis=1)) if len(x) else np.zeros((0, len(c)))
    which = d.argmin(axis=1).astype(np.int32) if len(x) else np.zeros(0, np.int32)
    return d[np.arange(len(x)), which].astype(np.float32), which


def check_groups(offsets, n_rows, dim, n_clusters):
    """The refusals of kmeans_fit_on_device, made before anything is uploaded -> int32 offsets."""
    k = int(n_clusters)
    if not 1 <= k <= MAX_CLUSTERS:
        raise ValueError(f"n_clusters {k} outside [1, {MAX_CLUSTERS}]")
    if dim < 1 or k * dim > MAX_CENTER_VALUES or (k + 1) * dim > MAX_LDS_VALUES:
        raise ValueError(f"n_clusters * dim = {k * dim} above {MAX_CENTER_VALUES}, or (n_clusters + 1) * dim = {(k + 1) * dim} above {MAX_LDS_VALUES}")
    off = problems.check_offsets(offsets, n_rows, "group")
    sizes = np.diff(off)
    for g in np.nonzero(sizes < k)[0][:1]:
        raise ValueError(f"group {int(g)} has {int(sizes[g])} points for {k} clusters")
    for g in np.nonzero(sizes > MAX_POINTS)[0][:1]:
        raise ValueError(f"group {int(g)} has {int(sizes[g])} points: at most {MAX_POINTS}")
    return off.astype(np.int32)


def kmeans_fit_on_device(x, offsets, n_clusters, seeds, max_iter=300, tol=1e-4, want_f64=False):
    """x: CUDA tensor or numpy array [rows, dim] float32; group g = rows offsets[g] .. offsets[g + 1]; seeds: an int or one per group.
    -> KMeansFit(centers float32 [G, k, dim], centers_f64 (want_f64) or None, labels int32 [rows] (-1 outside every group), init int32
    [G, k], info int32 [G, 4] = {status, n_iter, stop reason, smallest cluster size}, d_centers = the centres still on the device).
    One upload (offsets and draws), one launch, one copy back.  Bad offsets, a group smaller than n_clusters or larger than MAX_POINTS
    and shapes above the caps are refused before anything is uploaded."""
    import torch
    rows, dim = problems.bank_shape(x)
    k = int(n_clusters)
    off = check_groups(offsets, rows, dim, k)
    G = off.size - 1
    seeds = [int(seeds)] * G if np.ndim(seeds) == 0 else [int(s) for s in seeds]
    if len(seeds) != G:
        raise ValueError(f"{len(seeds)} seeds for {G} groups")
    if int(max_iter) < 1 or not float(tol) >= 0:
        raise ValueError("max_iter must be at least 1 and tol non-negative")
    T = n_local_trials(k)
    draws = np.stack([kmeans_draws(s, k) for s in seeds]) if G else np.zeros((0, 1 + (k - 1) * T))
    x = problems.device_bank(x)
    dev = x.device
    with torch.cuda.device(dev):
        # one upload of 8-byte words: the draws, then the offsets in pairs
        d_in, (p_draws, p_off) = _lib.upload_words([draws, off], dev)
        out = _lib.OutputWords([("centers_f64", np.float64, (G, k, dim))] * bool(want_f64) +
                               [("centers", np.float32, (G, k, dim)), ("labels", np.int32, (rows,)), ("init", np.int32, (G, k)),
                                ("info", np.int32, (G, 4))], dev, fill={"labels": -1})
        if G:
            _lib.check(_lib.lib().mkws_kmeans_fit(x.data_ptr(), dim, p_off, G, k, p_draws, T, int(max_iter), float(tol), out.ptr("centers"),
                                                  out.ptr("centers_f64") if want_f64 else None, out.ptr("labels"), out.ptr("init"),
                                                  out.ptr("info"), _lib.current_stream_ptr()))
        out.fetch()                                                    # the call's one synchronisation
    return KMeansFit(out.host("centers"), out.host("centers_f64") if want_f64 else None, out.host("labels"), out.host("init"), out.host("info"),
                     out.device("centers"))


def check_nearest_out(rows, device, out):
    """What nearest_on_device refuses of `out`, decided before any device call: three tensors on `device` -- dist contiguous float32 and
    which contiguous int32 of `rows` elements each, invalid int32 of one element.  ValueError otherwise."""
    import torch
    if not isinstance(out, (tuple, list)) or len(out) != 3 or not all(torch.is_tensor(t) for t in out):
        raise ValueError("out must be the three tensors (dist, which, invalid)")
    for name, t, dtype, n in (("dist", out[0], torch.float32, int(rows)), ("which", out[1], torch.int32, int(rows)), ("invalid", out[2], torch.int32, 1)):
        if t.dtype != dtype or t.numel() != n or not t.is_contiguous() or t.device != device:
            raise ValueError(f"out: {name} must be a contiguous {dtype} tensor of {n} elements on {device}, got {t.dtype} {tuple(t.shape)} "
                             f"(strides {t.stride()}) on {t.device}")


def nearest_on_device(x, group, centers, out=None):
    """x: CUDA tensor [rows, dim] float32; group: CUDA tensor or array int32 [rows]; centers: CUDA tensor [G, k, dim] float32.
    -> (dist float32 [rows], which int32 [rows], invalid int32 [1]) CUDA tensors (`out`: the three to write into).  Asynchronous: nothing
    is copied and nothing waits; a row whose group is outside [0, G) gets NaN / -1 and is counted in `invalid`."""
    import torch
    x = problems.device_bank(x, upload=False)
    if not (torch.is_tensor(centers) and centers.is_cuda and centers.dtype == torch.float32 and centers.dim() == 3):
        raise ValueError("centers must be a CUDA tensor [groups, clusters, dim] of float32")
    rows, dim = (int(v) for v in x.shape)
    G, k = int(centers.shape[0]), int(centers.shape[1])
    if int(centers.shape[2]) != dim:
        raise ValueError(f"centers of {int(centers.shape[2])} columns for rows of {dim}")
    if not 1 <= k <= MAX_CLUSTERS:
        raise ValueError(f"n_clusters {k} outside [1, {MAX_CLUSTERS}]")
    dev = x.device
    if centers.device != dev:
        raise ValueError(f"centers must live on the device of x ({dev}), not {centers.device}")
    if out is not None:
        check_nearest_out(rows, dev, out)
    if not torch.is_tensor(group):                 # (uploaded only once everything else the caller gave has been accepted)
        if np.size(group) != rows:
            raise ValueError("group must hold one int32 per row, on the device of x")
        group = torch.from_numpy(np.ascontiguousarray(group, dtype=np.int32)).to(dev, non_blocking=True)
    if group.dtype != torch.int32 or group.numel() != rows or group.device != dev:
        raise ValueError("group must hold one int32 per row, on the device of x")
    group, centers = group.contiguous(), centers.contiguous()
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(rows, dtype=torch.float32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                   torch.zeros(1, dtype=torch.int32, device=dev))
        dist, which, invalid = out
        _lib.check(_lib.lib().mkws_kmeans_nearest(x.data_ptr(), dim, rows, group.data_ptr(), centers.data_ptr() if G else None, G, k,
                                                  dist.data_ptr(), which.data_ptr(), invalid.data_ptr(), _lib.current_stream_ptr()))
    return dist, which, invalid
