"""Typed fenced buffers and the written sets of the dataperf solvers (tests/test_dataperf_fenced_cpu.py, tests/test_dataperf_fenced_gpu.py).

A fenced buffer is ONE allocation [PAD | n elements | PAD] whose every 4-byte word starts as the canary of tests/util_train_ops.py (a
quiet NaN as a float32, 2.25e307 as the two halves of a float64, a large positive integer): a store into a pad is seen, an output element that
was never written is seen, a read of a pad or of an unwritten slot poisons what is computed from it.

The written-set builders are pure NumPy: from a call's lists and the statuses the header (include/mkws.h) gives its problems they
return one bool mask per output, True where the header says the call writes.  The header is the only source: nothing here looks at what
a kernel does."""
import numpy as np

from util_train_ops import CANARY, PAD

DTYPES = ("float32", "int32", "float64", "int64")
assert PAD % 2 == 0                      # the middle of an 8-byte buffer starts on an 8-byte boundary


def canary_array(shape, dtype):
    """A host array of `dtype` whose every 4-byte word is the canary."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64))
    return np.full(n * (dtype.itemsize // 4), CANARY, np.int32).view(dtype).reshape(shape)


def holds_canary(a):
    """bool per element of a host array: every 4-byte word of the element is the canary."""
    a = np.ascontiguousarray(a)
    words = a.reshape(-1).view(np.int32).reshape(a.size, a.dtype.itemsize // 4)
    return (words == CANARY).all(axis=1).reshape(a.shape)


def canaried(values, written):
    """`values` where `written`, the canary elsewhere: what a call that honours its written set leaves in a canary-filled buffer."""
    values = np.ascontiguousarray(values)
    out = canary_array(values.shape, values.dtype)
    out[written] = values[written]
    return out


def same_bits(a, b):
    """bool per element: equal bytes (a NaN equals itself, -0.0 differs from 0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    k = a.dtype.itemsize // 4
    return (a.reshape(-1).view(np.int32).reshape(a.size, k) == b.reshape(-1).view(np.int32).reshape(b.size, k)).all(axis=1).reshape(a.shape)


class FencedBuffer:
    """[PAD | n elements of `dtype` | PAD] in one allocation on `device`.  whole: the int32 view of all of it; words: the int32 view of
    the middle; mid: the middle as `dtype`.  fill = None leaves the canary in the middle (outputs, workspaces)."""

    def __init__(self, n, dtype="float32", fill=None, device="cuda"):
        import torch
        self.dtype = np.dtype(dtype)
        if self.dtype.name not in DTYPES:
            raise TypeError(f"a fenced buffer of {self.dtype}")
        self.n, self.k = int(n), self.dtype.itemsize // 4
        self.whole = torch.full((PAD + self.n * self.k + PAD,), CANARY, dtype=torch.int32, device=device)
        self.words = self.whole[PAD:PAD + self.n * self.k]
        self.mid = self.words.view(getattr(torch, self.dtype.name))
        if fill is not None:
            self.fill(fill)

    def ptr(self):
        """Address of the first middle element (also for n = 0, where it is the address of the rear pad)."""
        return self.whole.data_ptr() + 4 * PAD

    def fill(self, array):
        """The middle becomes the bytes of `array` (n elements of the buffer's dtype: NaN payloads survive)."""
        import torch
        a = np.ascontiguousarray(array).reshape(-1)
        if a.dtype != self.dtype or a.size != self.n:
            raise ValueError(f"{a.size} elements of {a.dtype} for a buffer of {self.n} of {self.dtype}")
        if self.n:
            self.words.copy_(torch.from_numpy(a.view(np.int32).copy()))

    def reset(self):
        """Canary everywhere again."""
        self.whole.fill_(CANARY)

    def host(self):
        """The middle as a host array of the buffer's dtype."""
        return self.words.cpu().numpy().view(self.dtype)

    def pads_intact(self):
        return bool((self.whole[:PAD] == CANARY).all()) and bool((self.whole[PAD + self.n * self.k:] == CANARY).all())

    def canary_mask(self):
        """bool [n]: the middle elements that still hold the canary in every word."""
        return holds_canary(self.host())

    def snapshot(self):
        """A copy of the whole allocation, pads included."""
        return self.whole.clone()

    def unchanged_since(self, snapshot):
        import torch
        return torch.equal(self.whole, snapshot)


INVALID_ARG = -1                         # MKWS_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ the protocol of tests/test_dataperf_fenced_gpu.py (its docstring numbers the assertions)

class Out:
    """One output argument: want (its dtype and shape are the buffer's; the reference values where written), written (bool mask), nan
    (bool mask: the contract says NaN there), start (in-out arguments: the content before the call; None = the canary), unspecified
    (bool mask: nothing may be asserted there)."""

    def __init__(self, want, written, nan=None, start=None, unspecified=None):
        self.want = np.ascontiguousarray(want)
        none = np.zeros(self.want.shape, bool)
        self.written = np.broadcast_to(written, self.want.shape)
        self.nan = none if nan is None else np.broadcast_to(nan, self.want.shape)
        self.unspecified = none if unspecified is None else np.broadcast_to(unspecified, self.want.shape)
        self.start = canary_array(self.want.shape, self.want.dtype) if start is None else np.ascontiguousarray(start, dtype=self.want.dtype)
        self.inout = start is not None
        assert self.start.shape == self.want.shape and not (self.nan & ~self.written).any()


def _where(mask):
    idx = np.argwhere(mask)
    return f"{len(idx)} elements, the first at {tuple(int(v) for v in idx[0])}" if len(idx) else "none"


def check_output(tag, name, got, o):
    held = ~o.written & ~o.unspecified
    bad = held & ~same_bits(got, o.start)
    assert not bad.any(), f"{tag}: {name} was written outside its written set: {_where(bad)}"                      # 4
    w = o.written & ~o.unspecified
    if not o.inout:
        bad = w & holds_canary(got)
        assert not bad.any(), f"{tag}: {name} holds the canary (never written, or computed from a canary NaN, whose payload travels) inside its written set: {_where(bad)}"   # 3
    plain = w & ~o.nan
    if got.dtype.kind == "f":
        bad = plain & ~np.isfinite(got)
        assert not bad.any(), f"{tag}: {name} is not finite: {_where(bad)}, {got[bad][:4]}"                        # 5
        bad = o.nan & (~np.isnan(got) | holds_canary(got))
        assert not bad.any(), f"{tag}: {name} is not a NaN of the call's own where the contract says NaN: {_where(bad)}"
    else:
        assert not o.nan.any()
    bad = plain & ~same_bits(got, o.want)
    assert not bad.any(), f"{tag}: {name} differs from the reference: {_where(bad)}, {got[bad][:4]} for {o.want[bad][:4]}"   # 3


def protocol(call, inputs, outputs, work_floats=None, refused=None, other_shape=None, device="cuda"):
    """call(p) -> the C call's return code, p = {argument name: device address}.  inputs {name: host array}, outputs {name: Out};
    work_floats: the float32 workspace "work" (None = the call has none); refused(p): the same call with one workspace element too few;
    other_shape(p): a call of another shape that uses this call's workspace allocation (it may also renew inputs that ARE that
    workspace: it returns {name: host array} of the inputs to fill again)."""
    import torch
    sync = torch.cuda.synchronize if str(device).startswith("cuda") else (lambda: None)
    b = {k: FencedBuffer(np.asarray(v).size, np.asarray(v).dtype, fill=v, device=device) for k, v in inputs.items()}
    for k, o in outputs.items():
        b[k] = FencedBuffer(o.want.size, o.want.dtype, fill=o.start, device=device)
    if work_floats is not None:
        b["work"] = FencedBuffer(work_floats, "float32", device=device)
    p = {k: v.ptr() for k, v in b.items()}
    if refused is not None:                                                                                       # 7
        before = {k: v.snapshot() for k, v in b.items()}
        rc = refused(p)
        sync()
        assert rc == INVALID_ARG, rc
        for k, v in b.items():
            assert v.unchanged_since(before[k]), f"the refused call changed {k}"
    snaps = {k: b[k].snapshot() for k in inputs}

    def run(tag):
        for k, o in outputs.items():
            if o.inout:
                b[k].fill(o.start)
        rc = call(p)
        sync()
        assert rc == 0, (tag, rc)                                                                                  # 1
        for k, v in b.items():
            assert v.pads_intact(), f"{tag}: a pad of {k} was written"
        for k in inputs:
            assert b[k].unchanged_since(snaps[k]), f"{tag}: the input {k} changed"                                 # 2
        got = {k: b[k].host().reshape(o.want.shape) for k, o in outputs.items()}
        for k, o in outputs.items():
            check_output(tag, k, got[k], o)
        return got

    first = run("first call")
    runs = [("the same call again", run("second call"))]                                                           # 6
    if other_shape is not None:
        renewed = other_shape(p) or {}
        sync()
        for k, v in renewed.items():
            b[k].fill(v)
            snaps[k] = b[k].snapshot()
        runs.append(("the call after another shape", run("call after another shape")))
    for tag, got in runs:
        for k, o in outputs.items():
            bad = ~same_bits(got[k], first[k]) & ~o.unspecified
            assert not bad.any(), f"{tag} changed {k}: {_where(bad)}"
    return first


# ------------------------------------------------------------------------------------------------ the written sets (include/mkws.h)

def _sizes(offsets):
    return np.diff(np.asarray(offsets, np.int64))


def logreg_fit_written(offsets, status, n_classes, dim):
    """status 0: coef[p], intercept[p], stats[p], info[p]; status 2: info[p] alone."""
    ok = np.asarray(status) == 0
    P, K = len(ok), int(n_classes)
    return dict(coef=np.broadcast_to(ok[:, None, None], (P, K, dim)).copy(), intercept=np.broadcast_to(ok[:, None], (P, K)).copy(),
                stats=np.broadcast_to(ok[:, None], (P, 2)).copy(), info=np.ones((P, 4), bool))


def svc_prepare_written(offsets, status, dim):
    """status 0: centre[p], inv_scale[p], gamma[p], info[p], gap[p]; status 2: info[p] alone."""
    ok = np.asarray(status) == 0
    P = len(ok)
    return dict(centre=np.broadcast_to(ok[:, None], (P, dim)).copy(), inv_scale=np.broadcast_to(ok[:, None], (P, dim)).copy(), gamma=ok.copy(),
                info=np.ones((P, 4), bool), gap=ok.copy())


def svc_kernel_written(offsets_a, offsets_b, status, out_stride):
    """out [P * out_stride]: exactly na_p * nb_p floats at p * out_stride for a problem that is not skipped (status 0)."""
    na, nb = _sizes(offsets_a), _sizes(offsets_b)
    out = np.zeros((len(na), int(out_stride)), bool)
    for p in np.nonzero(np.asarray(status) == 0)[0]:
        assert na[p] * nb[p] <= out_stride
        out[p, :na[p] * nb[p]] = True
    return dict(out=out.reshape(-1))


def svc_kernel_nan(rows_a, offsets_a, rows_b, offsets_b, status, n_bank, out_stride):
    """out [P * out_stride]: the entries of a written matrix whose row of list A or of list B is outside [0, n_bank): NaN by contract."""
    ra, rb = np.asarray(rows_a, np.int64), np.asarray(rows_b, np.int64)
    oa, ob = np.asarray(offsets_a, np.int64), np.asarray(offsets_b, np.int64)
    out = np.zeros((len(oa) - 1, int(out_stride)), bool)
    for p in np.nonzero(np.asarray(status) == 0)[0]:
        a, b = ra[oa[p]:oa[p + 1]], rb[ob[p]:ob[p + 1]]
        bad = ((a < 0) | (a >= n_bank))[:, None] | ((b < 0) | (b >= n_bank))[None, :]
        out[p, :bad.size] = bad.reshape(-1)
    return out.reshape(-1)


def svc_fit_written(offsets, status, n_list, n_classes):
    """A fitted problem: all n_p * (K - 1) coefficients of its list entries, all K (K - 1) / 2 entries of rho[p], info[p][2:4], gap[p].
    A refused one, and list entries that no offset names: nothing."""
    ok = np.asarray(status) == 0
    P, K = len(ok), int(n_classes)
    off = np.asarray(offsets, np.int64)
    coef = np.zeros((int(n_list), K - 1), bool)
    for p in np.nonzero(ok)[0]:
        coef[off[p]:off[p + 1]] = True
    info = np.zeros((P, 4), bool)
    info[ok, 2:] = True
    return dict(coef=coef, rho=np.broadcast_to(ok[:, None], (P, K * (K - 1) // 2)).copy(), info=info, gap=ok.copy())


def outside_entries(rows, offsets, n_bank, status=None):
    """bool [total]: the entries a scorer never dereferences and answers with -1 / NaN -- in front of offsets[0], behind offsets[P], a
    row outside [0, n_bank), and (status given) every entry of a problem whose status is not 0."""
    rows, off = np.asarray(rows, np.int64), np.asarray(offsets, np.int64)
    out = (rows < 0) | (rows >= n_bank)
    out[:off[0]] = True
    out[off[-1]:] = True
    if status is not None:
        for p in np.nonzero(np.asarray(status) != 0)[0]:
            out[off[p]:off[p + 1]] = True
    return out


def score_written(total, n_problems, width, second=None):
    """mkws_svc_score (width = K (K - 1) / 2: decision) and mkws_logreg_score (width = K: probs and, with second, logits): all of pred,
    of the per-entry values and of correct."""
    out = dict(pred=np.ones(int(total), bool), values=np.ones((int(total), int(width)), bool), correct=np.ones(int(n_problems), bool))
    if second:
        out[second] = np.ones((int(total), int(width)), bool)
    return out


def kmeans_fit_written(offsets, status, n_clusters, dim, n_rows):
    """status 0: centres, float64 centres, the labels of the group's rows, init and info; status 2: info alone; status 1: info, the rest of
    the group is `unspecified` (second dict: neither written nor unwritten may be asserted there).  Rows outside every group: nothing."""
    status = np.asarray(status)
    G, k = len(status), int(n_clusters)
    off = np.asarray(offsets, np.int64)
    ok, loose = status == 0, status == 1
    labels, loose_labels = np.zeros(int(n_rows), bool), np.zeros(int(n_rows), bool)
    for g in range(G):
        (labels if ok[g] else loose_labels if loose[g] else np.zeros(int(n_rows), bool))[off[g]:off[g + 1]] = True
    wide = lambda m, shape: np.broadcast_to(m.reshape((G,) + (1,) * (len(shape) - 1)), shape).copy()
    written = dict(centers=wide(ok, (G, k, dim)), centers_f64=wide(ok, (G, k, dim)), labels=labels, init=wide(ok, (G, k)), info=np.ones((G, 4), bool))
    unspecified = dict(centers=wide(loose, (G, k, dim)), centers_f64=wide(loose, (G, k, dim)), labels=loose_labels, init=wide(loose, (G, k)),
                       info=np.zeros((G, 4), bool))
    return written, unspecified


def kmeans_nearest_written(n_rows):
    """dist and which of every row, and invalid[0], which every launching call sets."""
    return dict(dist=np.ones(int(n_rows), bool), which=np.ones(int(n_rows), bool), invalid=np.ones(1, bool))


def roc_written(n_heads, n_thr):
    """All of counts [H, n_thr, 2] and of invalid [H], also for a head whose ranges are both empty."""
    return dict(counts=np.ones((int(n_heads), int(n_thr), 2), bool), invalid=np.ones(int(n_heads), bool))


def named_rows(n_bank, *lists):
    """bool [n_bank]: the bank rows that one of the (rows, offsets, status or None) lists names from a problem with status 0."""
    out = np.zeros(int(n_bank), bool)
    for rows, offsets, status in lists:
        rows, off = np.asarray(rows, np.int64), np.asarray(offsets, np.int64)
        for p in range(len(off) - 1):
            if status is None or status[p] == 0:
                r = rows[off[p]:off[p + 1]]
                out[r[(r >= 0) & (r < n_bank)]] = True
    return out


def poisoned_bank(x, named):
    """A copy of the bank in which every row that `named` does not mark is the canary NaN."""
    x = np.array(x, dtype=np.float32, copy=True)
    x.view(np.int32)[~np.asarray(named)] = CANARY
    return x


# ------------------------------------------------------------------------------------------------ the cases of the two test files

SVC_CASES = ["ragged_50_20_64", "ragged_50_20_64+label", "ragged_50_20_64+row", "65_problems_of_8_dim16", "absent_class", "c_0p01_1_100",
             "n12_k3_dim37", "k6_n200_scaled", "n150_k2_dim37"]
LOGREG_CASES = ["ragged_50_20_64", "ragged_50_20_64+label", "ragged_50_20_64+row", "65_problems_of_8_dim16", "absent_class", "c_0p01_1_100",
                "n7_k3_dim37", "k6_n200_scaled"]
N150_SEED = 204

_FENCED_CASES = {}


def solver_case(family, name):
    """A case of tests/svc_cases.py (family "svc") or tests/logreg_cases.py ("logreg") as the fenced tests call it, built once and left
    unchanged.  "+label" / "+row": the middle problem refused as in test_bad_problems_get_status_2_beside_unaffected_neighbours (a label
    equal to n_classes, a row equal to the bank's row count).  n150_k2_dim37 is new: one pair of 150 rows, more than the 128 rows whose
    sub-matrix SMO keeps in LDS, three tiles (64, 64, 22) per side of the Gram matrix.
    Added to the case's keys: status int [P] = what include/mkws.h gives each problem, and score_rows / score_true / score_offsets = the
    evaluation lists with two entries in front of offsets[0] and two behind offsets[P] that no list names (rows -7, 0, 2**30, n_bank) and
    the last entry of problem 0's list replaced by the row n_bank, outside the bank."""
    key = (family, name)
    if key not in _FENCED_CASES:
        import logreg_cases
        base, _, bad = name.partition("+")
        if base == "n150_k2_dim37":
            c = logreg_cases._build([150], 37, 2, N150_SEED)
        elif family == "svc":
            import svc_cases
            c = dict(svc_cases.case(base))
        else:
            c = dict(logreg_cases.case(base))
        c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        off = c["offsets"]
        n_bank = c["x"].shape[0]
        status = np.zeros(len(off) - 1, np.int32)
        if bad == "label":
            c["labels"][off[1] + 5] = c["n_classes"]
            status[1] = 2
        elif bad == "row":
            c["rows"][off[2] - 1] = n_bank
            status[1] = 2
        elif bad:
            raise KeyError(name)
        c["status"] = status
        c["score_rows"] = np.concatenate([[-7, 0], c["eval_rows"], [2 ** 30, n_bank]]).astype(np.int32)
        c["score_rows"][c["eval_offsets"][1] + 1] = n_bank             # and the last entry of problem 0's own list is a row outside the bank
        c["score_true"] = np.concatenate([[0, 0], c["eval_true"], [0, 0]]).astype(np.int32)
        c["score_offsets"] = (c["eval_offsets"] + 2).astype(np.int32)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FENCED_CASES[key] = c
    return _FENCED_CASES[key]


KMEANS_CASES = {
    # name: (dim, n_clusters, [(kind, points)]): "good" = a blob set of tests/kmeans_cases.py, "short" = fewer points than clusters
    # (status 2), "same" = identical points (the first Lloyd step meets an empty cluster: status 1), "loose" = rows outside every group
    "k2_dim64": (64, 2, [("loose", 3), ("good", 7), ("short", 1), ("good", 9), ("same", 5), ("loose", 2)]),
    "k3_dim1024": (1024, 3, [("loose", 1), ("good", 20), ("short", 2), ("good", 50), ("loose", 4)]),
}


def kmeans_case(name):
    """-> dict(x float32 [rows, dim], offsets int32 [G + 1], k, status int [G], seeds [G], group int32 [rows] for mkws_kmeans_nearest: the
    row's own group where that group is fitted, otherwise one of -1, G and 2**30)."""
    key = ("kmeans", name)
    if key not in _FENCED_CASES:
        import kmeans_cases
        dim, k, parts = KMEANS_CASES[name]
        rng = np.random.default_rng(len(name))
        x, offsets, status, group, g = [], [], [], [], 0
        at = 0
        for i, (kind, n) in enumerate(parts):
            if kind == "good":
                x.append(kmeans_cases.blobs(n, dim, k, 0.3, 500 + i))
            elif kind == "same":
                x.append(np.repeat(rng.standard_normal((1, dim)).astype(np.float32), n, axis=0))
            else:
                x.append(rng.standard_normal((n, dim)).astype(np.float32))
            if kind == "loose":
                if offsets and len(offsets) == len(status):          # the gap closes the previous group
                    offsets.append(at)
                group += [[-1, len(parts), 2 ** 30][j % 3] for j in range(n)]
            else:
                if len(offsets) == len(status):
                    offsets.append(at)
                status.append({"good": 0, "short": 2, "same": 1}[kind])
                offsets.append(at + n)
                group += [g if kind == "good" else -1] * n
                g += 1
            at += n
        # groups are contiguous in the header's layout (group g = rows offsets[g] .. offsets[g + 1]): loose rows sit only in front and behind
        offsets = sorted(set(offsets))
        G = len(status)
        assert len(offsets) == G + 1, (offsets, status)
        group = np.asarray(group, np.int64)
        group[group == len(parts)] = G
        c = dict(x=np.concatenate(x), offsets=np.asarray(offsets, np.int32), k=k, status=np.asarray(status, np.int32),
                 seeds=[700 + j for j in range(G)], group=group.astype(np.int32))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FENCED_CASES[key] = c
    return _FENCED_CASES[key]


ROC_THRESHOLDS = [1, 257, 4096]


def roc_case():
    """The (3, 63) raw-call vectors of tests/test_roc_gpu.py (head 0 without negatives, head 1 without positives, duplicates, a list longer
    than the plane) and a fourth head whose lists are both empty -> (probs float32 [4, 63, 3], positives, negatives)."""
    key = ("roc", "")
    if key not in _FENCED_CASES:
        from test_roc_gpu import yardstick_case
        probs, pos, neg = yardstick_case(3, 63)
        probs = np.concatenate([probs, probs[:1]])
        probs.setflags(write=False)
        _FENCED_CASES[key] = (probs, [list(p) for p in pos] + [[]], [list(n) for n in neg] + [[]])
    return _FENCED_CASES[key]


def roc_thresholds(n_thr):
    return np.asarray([0.37]) if n_thr == 1 else np.linspace(0.0, 1.0, n_thr)
