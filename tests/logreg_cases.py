"""Inputs shared by tests/test_logreg_cpu.py, tests/test_logreg_gpu.py and tests/golden/make_logreg_golden.py: embedding-like banks
(selu of low-rank class clusters plus noise) and row lists, regenerated from seeds, built once and left unchanged.

case(name) -> dict(x float32 [bank rows, dim], rows / labels int32 (one flat list), offsets int32 [P + 1] into those lists, n_classes,
C float64 [P], standardize, eval_rows / eval_offsets: the rows every problem is evaluated on = its own training rows, then held-out rows
of the same classes)."""
import hashlib

import numpy as np

CASES = ["n10_k2_dim1024", "n7_k3_dim37", "ragged_50_20_64", "65_problems_of_8_dim16", "k6_n200_raw", "k6_n200_scaled",
         "constant_column_scaled", "c_0p01_1_100", "absent_class", "caps_n1024_k8_dim1024"]

_CACHE = {}


def _selu(v):
    return 1.0507009873554805 * np.where(v > 0, v, 1.6732632423543772 * np.expm1(np.minimum(v, 0.0)))


def embedding_like(rng, labels, dim, n_classes, spread=1.0, rank=12, centres=None):
    """float32 [len(labels), dim]: selu(class centre in a `rank`-dimensional subspace + noise), scaled like dense_2 outputs."""
    if centres is None:
        centres = make_centres(rng, dim, n_classes, rank)
    low = rng.standard_normal((len(labels), centres[1].shape[0])) * 0.6 * spread
    pre = (centres[0][labels] + low) @ centres[1] + 0.35 * spread * rng.standard_normal((len(labels), dim))
    return (0.5 * _selu(pre)).astype(np.float32)


def make_centres(rng, dim, n_classes, rank=12):
    return rng.standard_normal((n_classes, rank)), rng.standard_normal((rank, dim)) / np.sqrt(rank)


def _build(sizes, dim, K, seed, C=1.0, standardize=False, n_eval=16, lead=0, tail=0, present=None, spread=1.0):
    """One problem per entry of `sizes`: its training rows and n_eval held-out rows, all in one bank (lead / tail: poisoned rows that no
    list names), the row lists shuffled."""
    rng = np.random.default_rng(seed)
    present = list(range(K)) if present is None else present
    bank = [np.full((lead, dim), 1e6, np.float32)]
    rows, labels, offsets, ev_rows, ev_true, ev_off, at = [], [], [0], [], [], [0], lead
    for n in sizes:
        centres = make_centres(rng, dim, K)
        y = np.asarray([present[i % len(present)] for i in range(n)])
        y_ev = np.asarray([present[i % len(present)] for i in range(n_eval)])
        bank.append(embedding_like(rng, y, dim, K, spread, centres=centres))
        bank.append(embedding_like(rng, y_ev, dim, K, spread, centres=centres))
        order = rng.permutation(n)
        rows.append(at + order)
        labels.append(y[order])
        offsets.append(offsets[-1] + n)
        ev_rows.append(np.concatenate([at + np.arange(n), at + n + np.arange(n_eval)]))
        ev_true.append(np.concatenate([y, y_ev]))
        ev_off.append(ev_off[-1] + n + n_eval)
        at += n + n_eval
    bank.append(np.full((tail, dim), -1e6, np.float32))
    P = len(sizes)
    return dict(x=np.concatenate(bank), rows=np.concatenate(rows).astype(np.int32), labels=np.concatenate(labels).astype(np.int32),
                offsets=np.asarray(offsets, np.int32), n_classes=K, C=np.full(P, C, np.float64) if np.ndim(C) == 0 else np.asarray(C, np.float64),
                standardize=standardize, eval_rows=np.concatenate(ev_rows).astype(np.int32), eval_true=np.concatenate(ev_true).astype(np.int32),
                eval_offsets=np.asarray(ev_off, np.int32))


def _make(name):
    if name == "n10_k2_dim1024":
        return _build([10], 1024, 2, 101)
    if name == "n7_k3_dim37":
        return _build([7], 37, 3, 102)
    if name == "ragged_50_20_64":
        # the row lists sit at 3 .. 137 of the flat list (three leading and two trailing entries that no offset names and that point
        # outside the bank); problem 1 shares a row with problem 0; problem 2 names one of its rows twice
        c = _build([50, 20, 64], 1024, 4, 103, lead=3, tail=2)
        rows, labels = c["rows"].copy(), c["labels"].copy()
        rows[50 + 4], labels[50 + 4] = rows[7], labels[7]
        rows[70 + 11], labels[70 + 11] = rows[70 + 30], labels[70 + 30]
        c["rows"] = np.concatenate([[-7, 2 ** 30, 0], rows, [-1, 10 ** 9]]).astype(np.int32)
        c["labels"] = np.concatenate([[99, 99, 99], labels, [99, 99]]).astype(np.int32)
        c["offsets"] = (c["offsets"] + 3).astype(np.int32)
        return c
    if name == "65_problems_of_8_dim16":
        return _build([8] * 65, 16, 3, 104, n_eval=4)
    if name in ("k6_n200_raw", "k6_n200_scaled"):
        # the harness's shape: 5 target words of 20 rows and 100 rows of "unknown" (class 0)
        c = _build([200], 1024, 6, 105, standardize=name.endswith("scaled"), n_eval=60)
        lo, hi = int(c["offsets"][0]), int(c["offsets"][1])
        y = np.concatenate([np.zeros(100, np.int64), np.repeat(np.arange(1, 6), 20)])
        rng = np.random.default_rng(1105)
        centres = make_centres(rng, 1024, 6)
        x = c["x"].copy()
        base = int(c["rows"][lo:hi].min())
        x[base:base + 200] = embedding_like(rng, y, 1024, 6, centres=centres)
        y_ev = np.arange(60) % 6
        x[base + 200:base + 260] = embedding_like(rng, y_ev, 1024, 6, centres=centres)
        c["x"] = x
        c["labels"] = y[c["rows"][lo:hi] - base].astype(np.int32)
        c["eval_true"] = np.concatenate([y, y_ev]).astype(np.int32)
        return c
    if name == "constant_column_scaled":
        c = _build([40], 64, 3, 106, standardize=True)
        x = c["x"].copy()
        x[:, 5], x[:, 9] = 0.75, 0.0
        c["x"] = x
        return c
    if name == "c_0p01_1_100":
        c = _build([60], 64, 3, 107)
        for key in ("rows", "labels", "eval_rows", "eval_true"):
            c[key] = np.tile(c[key], 3)
        c["offsets"] = np.asarray([0, 60, 120, 180], np.int32)
        c["eval_offsets"] = (np.arange(4) * int(c["eval_offsets"][1])).astype(np.int32)
        c["C"] = np.asarray([0.01, 1.0, 100.0])
        return c
    if name == "absent_class":
        return _build([30], 48, 4, 108, present=[0, 1, 3])
    if name == "caps_n1024_k8_dim1024":
        return _build([1024], 1024, 8, 109, C=0.05, n_eval=64, spread=1.5)
    raise KeyError(name)


def case(name):
    if name not in _CACHE:
        c = _make(name)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


def problems(c):
    """-> [(rows, labels, C, eval rows, eval labels)] of a case, problem by problem."""
    off, ev = c["offsets"], c["eval_offsets"]
    return [(c["rows"][off[p]:off[p + 1]], c["labels"][off[p]:off[p + 1]], float(c["C"][p]), c["eval_rows"][ev[p]:ev[p + 1]],
             c["eval_true"][ev[p]:ev[p + 1]]) for p in range(len(off) - 1)]


def x_hash(c):
    return hashlib.sha1(np.ascontiguousarray(c["x"]).tobytes()).hexdigest()
