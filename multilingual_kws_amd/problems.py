"""What kmeans.py, logreg.py and svc.py share: K small problems given as row lists into ONE bank of embedding vectors.  The refusals made
before anything is uploaded, the StandardScaler statistics, and the one rule by which a bank and an index list reach the device.  No
device code; torch is imported only where a tensor is handled."""
import numpy as np


def check_offsets(offsets, total, what):
    """-> int64 offsets: n + 1 non-decreasing integers inside [0, total] (`what` names the n things in messages)."""
    off = np.asarray(offsets)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"offsets must be a list of n_{what}s + 1 integers")
    off = off.astype(np.int64)
    if off[0] < 0 or off[-1] > total or (np.diff(off) < 0).any():
        raise ValueError(f"offsets must be non-decreasing and inside [0, {int(total)}]")
    return off


def check_lists(rows, labels, offsets, max_rows, what="problem"):
    """-> (rows int32, labels int32, offsets int32).  Refused: lists that are not flat, of integers and of equal length, bad offsets
    (check_offsets), a problem of more than max_rows rows.  What the lists hold is the device's to check."""
    rows, labels = np.asarray(rows), np.asarray(labels)
    if rows.size == 0:
        rows = rows.astype(np.int32)
    if labels.size == 0:
        labels = labels.astype(np.int32)
    for name, a in (("rows", rows), ("labels", labels)):
        if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must be one flat list of integers")
    if rows.shape != labels.shape:
        raise ValueError(f"{rows.size} rows for {labels.size} labels")
    off = check_offsets(offsets, rows.size, what)
    sizes = np.diff(off)
    for p in np.nonzero(sizes > max_rows)[0][:1]:
        raise ValueError(f"{what} {int(p)} has {int(sizes[p])} rows: at most {max_rows}")
    clip = lambda a: np.clip(a, -2 ** 31, 2 ** 31 - 1).astype(np.int32)      # (an index out of int32 stays out of every bank)
    return clip(rows), clip(labels), off.astype(np.int32)


def check_strengths(C, P):
    """-> float64 [P]: one positive finite C, or one per problem."""
    Cs = np.full(P, float(C)) if np.ndim(C) == 0 else np.asarray(C, dtype=np.float64).reshape(-1)
    if Cs.size != P:
        raise ValueError(f"{Cs.size} values of C for {P} problems")
    if not (np.isfinite(Cs).all() and (Cs > 0).all()):
        raise ValueError("C must be positive and finite")
    return Cs.astype(np.float64)


def check_problems(rows, labels, offsets, n_rows, dim, n_classes, C, max_rows, max_classes, max_dim):
    """check_problems of logreg.py and svc.py under the calling module's caps -> (rows int32, labels int32, offsets int32, C float64 [P]).
    Refused: n_classes outside [2, max_classes], dim outside [1, max_dim], and what check_lists and check_strengths refuse."""
    K = int(n_classes)
    if not 2 <= K <= max_classes:
        raise ValueError(f"n_classes {K} outside [2, {max_classes}]")
    if not 1 <= int(dim) <= max_dim:
        raise ValueError(f"dim {int(dim)} outside [1, {max_dim}]")
    if int(n_rows) < 0:
        raise ValueError("a bank of fewer than 0 rows")
    rows, labels, off = check_lists(rows, labels, offsets, max_rows)
    return rows, labels, off, check_strengths(C, off.size - 1)


def standard_scaler(X):
    """(mu, sigma) of StandardScaler over the rows of float64 X: ddof 0, sigma 0 -> 1."""
    mu = X.mean(axis=0)
    sigma = np.sqrt(((X - mu) ** 2).mean(axis=0))
    sigma[sigma == 0.0] = 1.0
    return mu, sigma


def check_one_problem(x, rows, labels, n_classes):
    """The refusals of the host solvers, which take one problem -> (x ndarray, rows int64, labels int64, K)."""
    K = int(n_classes)
    rows, y = np.asarray(rows, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    x = np.asarray(x)
    if x.ndim != 2 or rows.ndim != 1 or rows.shape != y.shape or rows.size == 0:
        raise ValueError("x must be [rows, dim]; rows and labels one non-empty list each, of equal length")
    if K < 2 or y.min() < 0 or y.max() >= K or rows.min() < 0 or rows.max() >= x.shape[0]:
        raise ValueError("n_classes below 2, a label outside [0, n_classes) or a row outside the bank")
    return x, rows, y, K


def bank_shape(x):
    """-> (n_rows, dim) of a bank: a numpy array or a CUDA tensor, float32 [rows, dim].  Uploads nothing."""
    import torch
    if torch.is_tensor(x) and not x.is_cuda:
        raise ValueError("x must be a CUDA tensor or numpy array [rows, dim] of float32")
    x = x if torch.is_tensor(x) else np.asarray(x)
    if x.dtype != (torch.float32 if torch.is_tensor(x) else np.float32):
        raise ValueError("x must be float32")
    if x.ndim != 2:
        raise ValueError("x must be [rows, dim]")
    return int(x.shape[0]), int(x.shape[1])


def device_bank(x, upload=True):
    """The bank on the device, contiguous: a CUDA tensor is taken as it is; a numpy array is uploaded (copied first only if it is
    read-only), or refused where upload is False.  What bank_shape refuses is refused here."""
    import torch
    bank_shape(x)
    if not torch.is_tensor(x):
        if not upload:
            raise ValueError("x must be a CUDA tensor [rows, dim] of float32")
        x = np.ascontiguousarray(x)
        x = torch.from_numpy(x if x.flags.writeable else x.copy()).cuda()
    return x.contiguous()


def device_int_list(a, name, dev):
    """A host list (clipped into int32, uploaded non-blocking) or a CUDA int32 tensor -> flat contiguous int32 on `dev`."""
    import torch
    if not torch.is_tensor(a):
        a = np.asarray(a)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must hold integers")
        a = torch.from_numpy(np.ascontiguousarray(np.clip(a, -2 ** 31, 2 ** 31 - 1), dtype=np.int32).reshape(-1)).to(dev, non_blocking=True)
    if a.dtype != torch.int32 or a.dim() != 1 or a.device != dev:
        raise ValueError(f"{name} must be a flat int32 list on the device of x")
    return a.contiguous()


def ptr_or_none(t):
    """The device pointer of a tensor; None for None and for an empty one."""
    return t.data_ptr() if t is not None and t.numel() else None
