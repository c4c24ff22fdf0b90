"""The case table of the point scorer (mkws_score_accumulate, multilingual_kws_amd/scoring.py), shared by tests/test_score_cpu.py (the
table's own claims, the bound constants) and tests/test_score_gpu.py (the kernel against scoring.score_host on every case).

GRID: every class count x every row count, both modes; the model count, shared / per-model labels and the group count cycle through the
grid so that every value of each meets every class count and every row count.  Class counts sit on both sides of the kernel's
LDS / wave-per-row boundary (32 | 33) and of a wave's width (64 | 65); row counts on both sides of a wave (63, 64, 65), past one
workgroup's tile (257 > 256; 65 > 32 for the wave-per-row kernel) and past two tiles (513 = 2 * 256 + 1).
NAMED: hand-made rows -- ties, NaNs, infinities, probabilities at and beyond the clip, logits of magnitude 80 and 100, labels and groups
outside their range -- each with what it claims about itself, which tests/test_score_cpu.py checks on the float32 bits.

The loss bound (how it was arrived at: tests/test_score_cpu.py::test_bound_constants_follow_from_the_table).  The accuracy the ROCm
device library documents for its float64 exp and log is not available in the toolchain's documentation as installed, so the bound is
MEASURED: scoring.score_kernel_order evaluates the kernel's formulas in float64 in the kernel's order of operations
(numpy's exp / log for the device library's), its distance from an exact evaluation (decimal arithmetic at 40 digits on sampled rows;
math.fsum for the sums) is taken in the units below, and four times the largest distance over the table is allowed.
  row, mode 0: unit = EPS * |loss|                                   -- one log: a relative error
  row, mode 1: unit = EPS * (adds + 1 + |max z| + |z[y]| + |loss|)   -- adds = roundings of the sum of exponentials on the kernel's path
               (classes - 1 in index order; ceil(classes / 64) - 1 + 6 across a wave), each at most EPS / 2 relative to the sum, which
               log() turns into an absolute error; one rounding each for + max z and - z[y]
  sum:         |device - fsum| <= the rows' bounds added up + SUM_BOUND_UNITS * EPS * sum |loss_r|
"""
import math
from decimal import Decimal, getcontext

import numpy as np

from multilingual_kws_amd import scoring

EPS = 2.0 ** -52
ROW_BOUND_UNITS = {0: 1.0, 1: 1.7}    # mode 1: 4 x 0.41, the twin's largest distance from exact, rounded up.  Mode 0: the twin's distance is 0
                                      # (numpy's log rounds these inputs correctly), which allows nothing, and a library log that is not
                                      # correctly rounded is off by at least an ulp where it is off at all: one unit (1 to 2 ulps), no more
SUM_BOUND_UNITS = 4.0                 # 4 x 0.98, the same for the second-stage sum (all three recomputed by tests/test_score_cpu.py)

CLASSES = (2, 3, 7, 32, 33, 64, 65, 761)
ROWS = (0, 1, 63, 64, 65, 257, 513)
MODELS = (1, 3)
GROUPS = (0, 1, 9)
SMALL_TILE, LARGE_TILE = 256, 32      # rows of a workgroup on either path (csrc/mkws_score.hip)


def n_adds(classes):
    return classes - 1 if classes <= scoring.SMALL_CLASSES else -(-classes // 64) - 1 + 6


def grid_cases():
    out, i = [], 0
    for ci, C in enumerate(CLASSES):
        for ri, N in enumerate(ROWS):
            for mode in (0, 1):
                out.append(dict(name=f"grid-C{C}-N{N}-mode{mode}", classes=C, rows=N, mode=mode, models=MODELS[(ci + ri + mode) % 2],
                                per_model=(i // 2) % 2, n_groups=GROUPS[(ci + 2 * ri + mode) % 3], seed=1000 + i, named=None))
                i += 1
    return out


def named_cases():
    return [dict(name=f"named-C{C}-mode{mode}", classes=C, rows=None, mode=mode, models=3, per_model=1, n_groups=9, seed=7 + C + mode, named=True)
            for C in (3, 32, 33, 65, 761) for mode in (0, 1)]


def all_cases():
    return grid_cases() + named_cases()


def _random_scores(rng, K, N, C, mode):
    z = rng.standard_normal((K, N, C)) * (3.0 if mode == 0 else 5.0)
    if mode == 0:
        z = np.exp(z - z.max(axis=2, keepdims=True)) if N else z
        z = z / z.sum(axis=2, keepdims=True) if N else z
    z = z.astype(np.float32)
    for k in range(K):                                    # every seventh row: an exact tie for the maximum at a random second index
        for r in range(3, N, 7):
            z[k, r, rng.integers(0, C)] = z[k, r].max()
    return z


def named_rows(C, mode):
    """[(name, float32 row [C], label, group, claims)].  claims: pred (the index np.argmax must give), tie (indices that hold the maximum,
    bit-equal), kind (0 tallied / 1 ignored / 2 invalid), loss ("nan", "finite" or a float the float64 loss must be close to)."""
    rng = np.random.default_rng(100 + C)
    rows = []
    last = C - 1
    mid = C // 2
    lane63 = 63 + 64 * ((C - 64) // 64) if C >= 64 else last          # the largest index read by a wave's last lane

    def base():
        if mode == 0:
            p = rng.uniform(0.0, 0.01, C)
        else:
            p = rng.uniform(-3.0, 3.0, C)
        return p.astype(np.float32)

    def add(name, row, label, group=0, **claims):
        claims.setdefault("kind", 0)
        rows.append((name, np.asarray(row, np.float32), int(label), int(group), claims))

    top = np.float32(0.5 if mode == 0 else 7.0)
    r = base(); r[[0, last]] = top
    add("two-way tie, first and last index", r, 0, pred=0, tie=(0, last))
    r = base(); r[[mid, last]] = top
    add("two-way tie away from index 0, label the loser", r, last, pred=mid, tie=(mid, last))
    r = base(); r[[0, mid, last]] = top
    add("three-way tie at the first, a middle and the last index", r, last, pred=0, tie=sorted({0, mid, last}))
    if C > 129:
        r = base(); r[[70, 129]] = top                                # lane 6 against lane 1: the lower lane holds the larger index
        add("tie between a lower index in a higher lane and a higher index in a lower lane", r, 129, pred=70, tie=(70, 129))
    if C > 64:
        r = base(); r[[3, 64]] = top
        add("tie between index 3 and index 64 (lanes 3 and 0)", r, 3, pred=3, tie=(3, 64))
    r = base(); r[lane63] = top
    add("the maximum in the last lane's stride", r, lane63, pred=lane63)
    r = base(); r[last] = top
    add("the maximum at the last index", r, last, pred=last)
    r = base(); r[:] = np.float32(-1.0) if mode else np.float32(0.001); r[0] = np.float32(-0.0); r[1] = np.float32(0.0)
    if mode == 1:
        add("-0.0 before +0.0: equal, the first index wins", r, 1, pred=0, tie=(0, 1))
    r = base(); r[mid] = np.nan
    add("one NaN beside larger numbers: the NaN wins", r, mid, pred=mid, loss="nan")
    r = base(); r[mid] = np.nan
    add("one NaN, the label elsewhere", r, 0, pred=mid, loss="finite" if mode == 0 else "nan")
    a, b = (1, last) if C <= 129 else (70, 129)                        # C > 64: the second NaN sits in a lower lane than the first
    r = base(); r[[a, b]] = np.nan
    add("two NaNs: the first wins", r, b, pred=a, loss="nan")
    r = base(); r[:] = np.nan
    add("every score NaN", r, last, pred=0, loss="nan")
    if mode == 1:
        r = base(); r[mid] = np.inf
        add("one +inf logit", r, mid, pred=mid, loss="nan")
        r = base(); r[[mid, last]] = np.inf
        add("two +inf logits: a tie", r, 0, pred=mid, tie=(mid, last), loss="nan")
        r = base(); r[0] = -np.inf
        add("one -inf logit, labelled: an infinite loss", r, 0, pred=int(np.argmax(r)), loss=float("inf"))
        r = base(); r[:] = -np.inf
        add("every logit -inf", r, 0, pred=0, tie=tuple(range(C)) if C <= 8 else (0, last), loss="nan")
        r = base(); r[:] = np.float32(-80.0); r[0] = np.float32(80.0)
        add("logits of magnitude 80, label the minimum", r, last, pred=0, loss=160.0)
        r = (np.float32(80.0) + base()).astype(np.float32)
        add("every logit near +80", r, mid, pred=int(np.argmax(r)), loss="finite")
        r = (np.float32(-80.0) + base()).astype(np.float32)
        add("every logit near -80", r, mid, pred=int(np.argmax(r)), loss="finite")
        r = base(); r[:] = np.float32(-100.0); r[mid] = np.float32(100.0)
        add("logits of magnitude 100: exp overflows in float32", r, 0, pred=mid, loss=200.0, f32_overflow=True)
    else:
        r = base(); r[mid] = np.float32(0.0); r[0] = np.float32(1.0)
        add("p[y] = 0", r, mid, pred=0, loss=-math.log(scoring.PROB_LO), clipped="lo")
        r = base(); r[mid] = np.float32(1.0)
        add("p[y] = 1", r, mid, pred=mid, loss=-math.log(scoring.PROB_HI), clipped="hi")
        r = base(); r[mid] = np.float32(1e-8); r[0] = np.float32(0.9)
        add("p[y] below 1e-7", r, mid, pred=0, loss=-math.log(scoring.PROB_LO), clipped="lo")
        r = base(); r[mid] = np.float32(1e-7); r[0] = np.float32(0.9)
        add("p[y] = float32 1e-7 exactly: not clipped", r, mid, pred=0, loss=-math.log(scoring.PROB_LO), clipped="at lo")
        r = base(); r[mid] = np.nextafter(np.float32(1.0), np.float32(0.0))
        add("p[y] = 1 - 2^-24, above the float32 1 - 1e-7", r, mid, pred=mid, loss=-math.log(scoring.PROB_HI), clipped="hi")
        r = base(); r[mid] = np.float32(-0.25); r[0] = np.float32(2.0)
        add("p[y] negative, another above 1", r, mid, pred=0, loss=-math.log(scoring.PROB_LO), clipped="lo")
    r = base(); r[mid] = top
    add("label -1: ignored", r, -1, pred=mid, kind=1)
    add("label -1 with a group outside its range: still ignored", r, -1, group=9, pred=mid, kind=1)
    add("label = classes: invalid", r, C, pred=mid, kind=2)
    add("label -2: invalid", r, -2, pred=mid, kind=2)
    add("label 2^31 - 1: invalid", r, 2 ** 31 - 1, pred=mid, kind=2)
    add("group = n_groups: invalid", r, mid, group=9, pred=mid, kind=2)
    add("group -1: invalid", r, mid, group=-1, pred=mid, kind=2)
    add("the last group, the last class", np.where(np.arange(C) == last, top, r * 0), last, group=8, pred=last)
    return rows


def build(case):
    """-> scores float32 [K, N, C], labels int32 [N] or [K, N], groups int32 [N] or None, and (named cases) the rows' claims."""
    rng = np.random.default_rng(case["seed"])
    K, C, mode, G = case["models"], case["classes"], case["mode"], case["n_groups"]
    if not case["named"]:
        N = case["rows"]
        scores = _random_scores(rng, K, N, C, mode)
        labels = rng.integers(0, C, (K, N) if case["per_model"] else (N,)).astype(np.int32)
        labels[..., 5::11] = -1                                       # padding rows here and there
        groups = rng.integers(0, G, N).astype(np.int32) if G else None
        return scores, labels, groups, None
    named = named_rows(C, mode)
    N = len(named)
    scores = np.stack([np.stack([row for _, row, _, _, _ in named])] * K)
    labels = np.stack([np.asarray([lab for _, _, lab, _, _ in named], np.int64).astype(np.int32)] * K)
    for k in range(1, K):                                             # models 1, 2: the same rows under other labels
        ok = (labels[0] >= 0) & (labels[0] < C)
        labels[k] = np.where(ok, (labels[0] + k) % C, labels[0])
    groups = np.asarray([g for _, _, _, g, _ in named], np.int32)
    return scores, labels, groups, named


def units(case, scores, want):
    """The error unit of every row's loss, [K, N] (see the module's docstring); NaN where the row is not tallied or its loss is not finite."""
    K, N, C = scores.shape
    loss = want.row_loss
    if case["mode"] == 0:
        unit = EPS * np.abs(loss)
    else:
        z = scores.astype(np.float64)
        labels = np.where(want.kind == 0, want.labels, 0)
        with np.errstate(all="ignore"):
            top = z.max(axis=2) if N else np.zeros((K, 0))
            zy = np.take_along_axis(z, labels[:, :, None], axis=2)[:, :, 0] if N else np.zeros((K, 0))
            unit = EPS * (n_adds(C) + 1 + np.abs(top) + np.abs(zy) + np.abs(loss))
    return np.where(np.isfinite(loss), unit, np.nan)


def host(case, scores, labels, groups):
    """scoring.score_host of the case, with the broadcast labels kept beside it."""
    want = scoring.score_host(scores, labels, groups, case["mode"], case["n_groups"])
    want.labels = np.broadcast_to(np.asarray(labels, np.int64), want.pred.shape) if np.asarray(labels).ndim == 1 else np.asarray(labels, np.int64)
    return want


def loss_bounds(case, scores, want):
    """-> (row bound [K, N], sum bound [K]): what |device - score_host| may be, for finite losses (others must agree as NaN / inf)."""
    row = ROW_BOUND_UNITS[case["mode"]] * units(case, scores, want)
    finite = np.isfinite(want.row_loss)
    total = np.where(finite, row, 0.0).sum(axis=1) + SUM_BOUND_UNITS * EPS * np.where(finite, np.abs(want.row_loss), 0.0).sum(axis=1)
    return row, total


def measure_bounds(rows_per_model=3):
    """The kernel-order twin against exact arithmetic over the whole table -> ({mode: the largest row distance in units}, the largest
    distance of the second-stage sum in units of EPS * sum |loss_r|).  Rows: up to rows_per_model tallied finite rows of every model of
    every case, evenly spaced (the exact evaluation is slow); sums: every model of every case whose losses are all finite."""
    worst_row, worst_sum = {0: 0.0, 1: 0.0}, 0.0
    for case in all_cases():
        scores, labels, groups, _ = build(case)
        if scores.shape[1] == 0:
            continue
        want = host(case, scores, labels, groups)
        twin = scoring.score_kernel_order(scores, labels, groups, case["mode"], case["n_groups"])
        unit = units(case, scores, want)
        for k in range(scores.shape[0]):
            rows = np.nonzero(np.isfinite(unit[k]))[0]
            for r in rows[np.unique(np.linspace(0, rows.size - 1, min(rows_per_model, rows.size)).astype(int))] if rows.size else []:
                exact = exact_row_loss(scores[k, r], int(want.labels[k, r]), case["mode"])
                worst_row[case["mode"]] = max(worst_row[case["mode"]], abs(twin.row_loss[k, r] - exact) / unit[k, r])
            tallied = np.where(want.kind[k] == 0, twin.row_loss[k], 0.0)           # in place: zeros where the kernel's workspace holds them
            if np.isfinite(tallied).all() and np.abs(tallied).sum() > 0:
                worst_sum = max(worst_sum, abs(scoring.sum_kernel_order(tallied) - math.fsum(tallied)) / (EPS * np.abs(tallied).sum()))
    return worst_row, worst_sum


def exact_row_loss(z_row, y, mode):
    """One row's loss at 40 decimal digits, rounded once to float64 (finite inputs only)."""
    getcontext().prec = 40
    if mode == 0:
        p = min(max(float(z_row[y]), scoring.PROB_LO), scoring.PROB_HI)
        return float(-Decimal(p).ln())
    zs = [Decimal(float(v)) for v in z_row]
    top = max(zs)
    total = sum(((v - top).exp() for v in zs), Decimal(0))
    return float(total.ln() + top - zs[y])
