"""Point scores of classification evaluation on the device: host wrapper over mkws_score_accumulate (include/mkws.h), the counterpart of
roc.py (the curve half) for what Keras' model.evaluate and tf.math.confusion_matrix report.

A Scorer owns zeroed accumulators for K classifiers -- loss sum, {rows, correct, ignored, invalid}, confusion matrices, per-group
tallies -- and add() queues one kernel call per batch; nothing crosses to the host until result(), the one copy of a whole dataset.
score_host is the float64 numpy specification the tests hold the kernel to (integers with ==, losses within a derived bound);
score_kernel_order restates the float64 arithmetic in the kernel's order of operations, which is how that bound is measured."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np

from . import _lib

MAX_CLASSES = 4096          # MKWS_SCORE_MAX_CLASSES (include/mkws.h)
SMALL_CLASSES = 32          # up to here a thread takes a row staged in LDS; above, a wave takes a row (csrc/mkws_score.hip)
SUM_THREADS = 256           # the loss sum: thread t adds rows t, t + 256, ...; then a halving tree over the 256 partial sums
PROB_LO = float(np.float32(1e-7))                                   # Keras' float32 epsilon, widened
PROB_HI = float(np.float32(1.0) - np.float32(1e-7))                 # its float32 1 - epsilon = 1 - 2^-23, widened
_LABEL_DTYPES = ("torch.int32", "torch.int64", "torch.int16", "torch.int8", "torch.uint8")


def _got(t):
    import torch
    return f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__


def check_add(device, n_models, classes, n_groups, scores, labels, groups=None):
    """What Scorer.add refuses, decided before any device call (attribute reads and integer compares only): scores a float32 tensor
    [n_models, N, classes] -- or [N, classes] for one model -- on `device`; labels an integer tensor [N] (shared) or [n_models, N] on
    `device`; groups an integer tensor [N] on `device` exactly when the scorer has groups.  A strided view is made contiguous and other
    integer widths are converted to int32 by the wrapper.  -> (N, labels_per_model).  ValueError naming the argument otherwise."""
    import torch
    shape = (n_models, "N", classes) if n_models != 1 else f"({n_models}, N, {classes}) or (N, {classes})"
    if not torch.is_tensor(scores) or scores.dtype != torch.float32 or scores.device != device or scores.dim() not in (2, 3):
        raise ValueError(f"Scorer.add: scores must be a float32 tensor {shape} on {device}, got {_got(scores)}")
    if scores.dim() == 2 and n_models != 1:
        raise ValueError(f"Scorer.add: scores of rank 2 for {n_models} models: must be {shape}, got {_got(scores)}")
    if int(scores.shape[-1]) != classes or (scores.dim() == 3 and int(scores.shape[0]) != n_models):
        raise ValueError(f"Scorer.add: scores must be {shape}, got {_got(scores)}")
    N = int(scores.shape[-2])
    if not torch.is_tensor(labels) or str(labels.dtype) not in _LABEL_DTYPES or labels.device != device or labels.dim() not in (1, 2):
        raise ValueError(f"Scorer.add: labels must be an integer tensor [N] or [{n_models}, N] on {device}, got {_got(labels)}")
    if tuple(labels.shape) not in ((N,), (n_models, N)):
        raise ValueError(f"Scorer.add: labels {tuple(labels.shape)} for scores of {N} rows and {n_models} models")
    if n_groups == 0:
        if groups is not None:
            raise ValueError("Scorer.add: groups given to a scorer made with n_groups = 0")
    else:
        if not torch.is_tensor(groups) or str(groups.dtype) not in _LABEL_DTYPES or groups.device != device or groups.dim() != 1:
            raise ValueError(f"Scorer.add: groups must be an integer vector [N] on {device} (the scorer has {n_groups} groups), got {_got(groups)}")
        if int(groups.shape[0]) != N:
            raise ValueError(f"Scorer.add: {int(groups.shape[0])} groups for the {N} rows of scores")
    return N, int(labels.dim() == 2)


def _as_int32(t):
    import torch
    return t.to(torch.int32).contiguous()


class Scorer:
    """Accumulators for `n_models` classifiers of `classes` classes.  mode 0: the scores are probabilities (Keras' from_logits=False);
    mode 1: logits.  add() is asynchronous and allocates only when a batch is larger than every one before it (reserve() sizes the
    workspace ahead, e.g. before a graph capture); result() is the one synchronisation."""

    def __init__(self, n_models, classes, mode, n_groups=0, confusion=True, device=None):
        import torch
        n_models, classes, mode, n_groups = int(n_models), int(classes), int(mode), int(n_groups)
        if n_models < 1:
            raise ValueError(f"Scorer: n_models = {n_models}")
        if not 2 <= classes <= MAX_CLASSES:
            raise ValueError(f"Scorer: classes = {classes} outside [2, {MAX_CLASSES}]")
        if mode not in (0, 1):
            raise ValueError(f"Scorer: mode {mode}: 0 (probabilities) or 1 (logits)")
        if n_groups < 0:
            raise ValueError(f"Scorer: n_groups = {n_groups}")
        self.device = _lib.indexed_device(device)
        if self.device.type != "cuda":
            raise ValueError(f"Scorer: device {self.device}: the scorer runs on a GPU only")
        self.n_models, self.classes, self.mode, self.n_groups, self.confusion = n_models, classes, mode, n_groups, bool(confusion)
        K, C, G = n_models, classes, n_groups
        sizes = [("loss", K), ("tally", K * 4), ("confusion", K * C * C if self.confusion else 0), ("groups", K * G * 2)]
        self._at, at = {}, 0
        for name, n in sizes:
            self._at[name] = (at, at + n)
            at += n
        self.L = _lib.lib()
        self._acc = torch.zeros(at, dtype=torch.int64, device=self.device)          # 8-byte words: the loss sums as their bit patterns
        self._work = None

    def _ptr(self, name):
        a, b = self._at[name]
        return ctypes.c_void_p(self._acc.data_ptr() + 8 * a) if b > a else None

    def reserve(self, n_rows):
        """Sizes the workspace for batches of up to n_rows rows."""
        import torch
        need = self.L.mkws_score_work_bytes(self.n_models, int(n_rows))
        if self._work is None or self._work.numel() * 8 < need:
            self._work = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)

    def add(self, scores, labels, groups=None, row_loss=None, pred=None):
        """Queues one batch.  row_loss (float64 [n_models, N]) / pred (int32 [n_models, N]): optional contiguous device tensors the kernel
        writes every row's loss and prediction into."""
        import torch
        N, per_model = check_add(self.device, self.n_models, self.classes, self.n_groups, scores, labels, groups)
        for name, t, dtype in (("row_loss", row_loss, torch.float64), ("pred", pred, torch.int32)):
            if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or t.device != self.device or not t.is_contiguous() or
                                  t.numel() != self.n_models * N):
                raise ValueError(f"Scorer.add: {name} must be a contiguous {dtype} tensor of {self.n_models} x {N} elements on {self.device}, got {_got(t)}")
        if N == 0:
            return
        with torch.cuda.device(self.device):
            self.reserve(N)
            scores, labels = scores.contiguous(), _as_int32(labels)
            groups = _as_int32(groups) if groups is not None else None
            _lib.check(self.L.mkws_score_accumulate(
                scores.data_ptr(), self.n_models, N, self.classes, self.mode, labels.data_ptr(), per_model,
                groups.data_ptr() if groups is not None else None, self.n_groups, self._ptr("loss"), self._ptr("tally"), self._ptr("confusion"),
                self._ptr("groups"), row_loss.data_ptr() if row_loss is not None else None, pred.data_ptr() if pred is not None else None,
                self._work.data_ptr(), _lib.current_stream_ptr()))

    def reset(self):
        self._acc.zero_()

    def raw(self):
        """The accumulators as they stand (the one copy; it synchronises) -> loss_sum float64 [K], tally int64 [K, 4],
        confusion int64 [K, C, C] or None, group_tally int64 [K, G, 2]."""
        words = self._acc.cpu().numpy()
        K, C, G = self.n_models, self.classes, self.n_groups
        part = lambda name: words[self._at[name][0]:self._at[name][1]]
        return SimpleNamespace(loss_sum=part("loss").view(np.float64).copy(), tally=part("tally").reshape(K, 4).copy(),
                               confusion=part("confusion").reshape(K, C, C).copy() if self.confusion else None,
                               group_tally=part("groups").reshape(K, G, 2).copy())

    def result(self):
        """-> loss (mean over the tallied rows), accuracy, rows, correct, ignored [K]; confusion_matrix int64 [K, C, C] (None without
        it); group_accuracy float64 / group_rows int64 [K, G] (NaN accuracy for a group without rows); loss_sum.  RuntimeError when a
        label or group outside its range reached the device."""
        raw = self.raw()
        bad = np.nonzero(raw.tally[:, 3])[0]
        if bad.size:
            k = int(bad[0])
            raise RuntimeError(f"model {k}: {int(raw.tally[k, 3])} rows with a label outside [0, {self.classes}) (and not -1) or a group outside "
                               f"[0, {self.n_groups}) reached the device")
        return summarise(raw.loss_sum, raw.tally, raw.confusion, raw.group_tally)


def summarise(loss_sum, tally, confusion, group_tally):
    """The accumulators -> what Scorer.result returns (shared with score_host's callers)."""
    rows = tally[:, 0].astype(np.int64)
    denom = np.maximum(rows, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        group_acc = group_tally[:, :, 1] / group_tally[:, :, 0].astype(np.float64)
    return SimpleNamespace(loss=loss_sum / denom, accuracy=tally[:, 1] / denom, rows=rows, correct=tally[:, 1].astype(np.int64),
                           ignored=tally[:, 2].astype(np.int64), confusion_matrix=confusion, group_accuracy=group_acc,
                           group_rows=group_tally[:, :, 0].astype(np.int64), loss_sum=loss_sum)


def precision_recall_f1(confusion):
    """int [.., C, C] (row = true class) -> (precision, recall, f1), float64 [.., C] per class, with the convention of
    sklearn.metrics.precision_recall_fscore_support(zero_division=0): a ratio with a zero denominator is 0."""
    cm = np.asarray(confusion, dtype=np.float64)
    tp = np.diagonal(cm, axis1=-2, axis2=-1)
    predicted, actual = cm.sum(axis=-2), cm.sum(axis=-1)
    ratio = lambda a, b: np.divide(a, b, out=np.zeros_like(a, dtype=np.float64), where=b != 0)
    precision, recall = ratio(tp, predicted), ratio(tp, actual)
    return precision, recall, ratio(2 * tp, predicted + actual)


def _normalise(scores, labels, groups):
    scores = np.asarray(scores)
    if scores.dtype != np.float32:
        raise ValueError("scores must be float32: the prediction is a function of the float32 bits")
    if scores.ndim == 2:
        scores = scores[None]
    K, N, C = scores.shape
    labels = np.asarray(labels).astype(np.int64)
    labels = np.broadcast_to(labels, (K, N)) if labels.ndim == 1 else labels
    if labels.shape != (K, N):
        raise ValueError(f"labels {labels.shape} for scores {scores.shape}")
    groups = None if groups is None else np.asarray(groups).astype(np.int64).reshape(N)
    return scores, labels, groups


def _kinds(labels, groups, C, n_groups):
    """0 tallied / 1 ignored / 2 invalid, [K, N]."""
    kind = np.where(labels == -1, 1, np.where((labels < 0) | (labels >= C), 2, 0))
    if groups is not None:
        kind = np.where((kind == 0) & ((groups < 0) | (groups >= n_groups))[None], 2, kind)
    return kind


def _tallies(pred, labels, groups, kind, C, n_groups, confusion):
    K = pred.shape[0]
    ok = kind == 0
    tally = np.stack([ok.sum(1), (ok & (pred == labels)).sum(1), (kind == 1).sum(1), (kind == 2).sum(1)], axis=1).astype(np.int64)
    cm = np.zeros((K, C, C), np.int64) if confusion else None
    gt = np.zeros((K, n_groups, 2), np.int64)
    for k in range(K):
        if confusion:
            np.add.at(cm[k], (labels[k][ok[k]], pred[k][ok[k]]), 1)
        if groups is not None:
            np.add.at(gt[k, :, 0], groups[ok[k]], 1)
            np.add.at(gt[k, :, 1], groups[ok[k] & (pred[k] == labels[k])], 1)
    return tally, cm, gt


def score_host(scores, labels, groups=None, mode=0, n_groups=0, confusion=True):
    """The float64 numpy specification of mkws_score_accumulate on zeroed accumulators.  scores float32 [K, N, C] or [N, C]; labels
    [N] or [K, N]; groups [N] or None.  -> pred int32 [K, N] (np.argmax: first maximum, first NaN wins), row_loss float64 [K, N] (NaN
    for ignored and invalid rows), loss_sum float64 [K] (math.fsum over the tallied rows' losses: the exactly rounded sum), tally
    int64 [K, 4], confusion int64 [K, C, C], group_tally int64 [K, G, 2]."""
    scores, labels, groups = _normalise(scores, labels, groups)
    K, N, C = scores.shape
    pred = np.argmax(scores, axis=2).astype(np.int32) if N else np.zeros((K, 0), np.int32)
    kind = _kinds(labels, groups, C, n_groups)
    ok = kind == 0
    y = np.where(ok, labels, 0)
    z = scores.astype(np.float64)
    zy = np.take_along_axis(z, y[:, :, None], axis=2)[:, :, 0] if N else np.zeros((K, 0))
    with np.errstate(all="ignore"):
        if mode == 0:
            loss = -np.log(np.minimum(np.maximum(zy, PROB_LO), PROB_HI))
            loss = np.where(np.isnan(zy), np.nan, loss)
        else:
            top = z.max(axis=2) if N else np.zeros((K, 0))
            loss = (np.log(np.exp(z - top[:, :, None]).sum(axis=2)) + top) - zy
    row_loss = np.where(ok, loss, np.nan)
    loss_sum = np.asarray([math.fsum(row_loss[k][ok[k]]) if not np.isnan(row_loss[k][ok[k]]).any() else np.nan for k in range(K)], np.float64)
    tally, cm, gt = _tallies(pred, labels, groups, kind, C, n_groups, confusion)
    return SimpleNamespace(pred=pred, row_loss=row_loss, loss_sum=loss_sum, tally=tally, confusion=cm, group_tally=gt, kind=kind)


def sum_kernel_order(values):
    """float64 [N] -> their sum in the order of the device's second stage: 256 strided partial sums, then a halving tree."""
    v = np.asarray(values, np.float64)
    n = -(-max(v.size, 1) // SUM_THREADS) * SUM_THREADS
    part = np.zeros(SUM_THREADS)
    for row in np.concatenate([v, np.zeros(n - v.size)]).reshape(-1, SUM_THREADS):
        part = part + row
    off = SUM_THREADS // 2
    while off:
        part[:off] = part[:off] + part[off:2 * off]
        off //= 2
    return float(part[0])


def score_kernel_order(scores, labels, groups=None, mode=0, n_groups=0):
    """The numpy twin of the kernel's float64 arithmetic: the same formulas as score_host, evaluated in the kernel's order -- classes <=
    32: the exponentials added in index order; above: 64 lane sums over classes l, l + 64, ..., then an xor butterfly; the loss sum as
    sum_kernel_order.  numpy's exp and log stand in for the device library's.  -> row_loss [K, N] (NaN where not tallied), loss_sum [K]."""
    scores, labels, groups = _normalise(scores, labels, groups)
    K, N, C = scores.shape
    kind = _kinds(labels, groups, C, n_groups)
    ok = kind == 0
    y = np.where(ok, labels, 0)
    z = scores.astype(np.float64)
    zy = np.take_along_axis(z, y[:, :, None], axis=2)[:, :, 0]
    with np.errstate(all="ignore"):
        if mode == 0:
            q = np.minimum(np.maximum(zy, PROB_LO), PROB_HI)
            loss = np.where(np.isnan(zy), np.nan, -np.log(q))
        else:
            top = z.max(axis=2)
            e = np.exp(z - top[:, :, None])
            if C <= SMALL_CLASSES:
                total = np.zeros((K, N))
                for c in range(C):
                    total = total + e[:, :, c]
            else:
                steps = -(-C // 64)
                e = np.concatenate([e, np.zeros((K, N, steps * 64 - C))], axis=2).reshape(K, N, steps, 64)
                lanes = np.zeros((K, N, 64))
                for s in range(steps):
                    lanes = lanes + e[:, :, s]
                for off in (32, 16, 8, 4, 2, 1):
                    lanes = lanes + lanes[:, :, np.arange(64) ^ off]
                total = lanes[:, :, 0]
            loss = (np.log(total) + top) - zy
    row_loss = np.where(ok, loss, np.nan)
    loss_sum = np.asarray([sum_kernel_order(np.where(ok[k], loss[k], 0.0)) for k in range(K)])
    return SimpleNamespace(row_loss=row_loss, loss_sum=loss_sum)


def eval_batches(x, y, batch_size, device):
    """What Keras' evaluate takes -> (spec CUDA [B, 49, 40], labels CUDA integer [B]) batches: a ClipDataset (its own .batch(); y and
    batch_size do not apply, as in Keras) or an array / tensor [N, 49, 40(, 1)] with labels y [N], cut into batches of batch_size."""
    import torch
    if not (torch.is_tensor(x) or isinstance(x, (np.ndarray, list, tuple))):
        if y is not None:
            raise ValueError("evaluate: y must be None when x is a dataset (it yields its own labels)")
        for spec, labels in x:
            yield (spec[..., 0] if spec.dim() == 4 else spec), labels
        return
    if y is None:
        raise ValueError("evaluate: y is required when x is an array")
    x = torch.as_tensor(x if torch.is_tensor(x) else np.asarray(x, dtype=np.float32)).to(device, dtype=torch.float32)
    y = torch.as_tensor(y if torch.is_tensor(y) else np.asarray(y)).to(device)
    if x.dim() == 4:
        x = x[..., 0]
    if y.dim() != 1 or y.shape[0] != x.shape[0] or y.dtype.is_floating_point or y.dtype == torch.bool:
        raise ValueError(f"evaluate: y must be {x.shape[0]} integer labels, got {y.dtype} {tuple(y.shape)}")
    bs = max(int(batch_size or 32), 1)
    for s in range(0, x.shape[0], bs):
        yield x[s:s + bs], y[s:s + bs]


def score_model(predict_device, device, classes, mode, x, y=None, batch_size=32, checked=None):
    """The scoring loop under every model's evaluate: one forward and one Scorer.add per batch, no host synchronisation between them,
    then the one copy -- inside `checked` (EmbeddingModel.checked) where the model has one.  -> Scorer.result()."""
    scorer = Scorer(1, classes, mode, device=device)

    def run():
        scorer.reset()
        for spec, labels in eval_batches(x, y, batch_size, scorer.device):
            scorer.add(predict_device(spec), labels)
        return scorer.result()

    return checked(run) if checked is not None else run()


def keras_metrics(result, names=("loss", "accuracy"), return_dict=False, extra_loss=0.0, model=0):
    """Scorer.result() -> what evaluate returns for a model compiled with one accuracy metric: [loss, accuracy] or {name: value}."""
    values = [float(result.loss[model]) + float(extra_loss), float(result.accuracy[model])]
    return dict(zip(names, values)) if return_dict else values
