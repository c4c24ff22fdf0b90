"""Device ROC counts: host wrapper over mkws_roc_count (include/mkws.h), the counterpart of detector.py for the classification half.

How many of a keyword head's positive and of its negative clips score above each threshold, for K heads x T thresholds in one launch.
embedding/transfer_learning_analysis.py (roc_single_target, roc_sc) is the specification: the counts are the integers those functions
divide, equal with == (tests/test_roc_gpu.py); there is no tolerance to choose."""
import numpy as np

from . import _lib

MAX_THRESHOLDS = 4096     # MKWS_ROC_MAX_THRESHOLDS (include/mkws.h): thresholds of one C call; longer lists run in pieces


def pack_rows(lists, n_heads, n_rows, what):
    """K lists of row indices (duplicates kept, may be empty) -> (int32 rows back to back, int32 offsets [K + 1]); an index outside
    [0, n_rows) is refused here, before anything is uploaded."""
    lists = list(lists)
    if len(lists) != n_heads:
        raise ValueError(f"{len(lists)} lists of {what} for {n_heads} heads")
    out = []
    for k, rows in enumerate(lists):
        r = np.asarray(rows).reshape(-1)
        if r.size and not np.issubdtype(r.dtype, np.integer):
            raise ValueError(f"{what}[{k}] must hold integer row indices")
        r = r.astype(np.int64)
        bad = np.nonzero((r < 0) | (r >= n_rows))[0]
        if bad.size:
            raise ValueError(f"{what}[{k}][{int(bad[0])}] = {int(r[bad[0]])} outside [0, {n_rows})")
        out.append(r.astype(np.int32))
    rows = np.concatenate(out) if out else np.zeros(0, np.int32)
    if rows.size >= 2 ** 31:
        raise ValueError(f"too many {what} entries")
    offsets = np.zeros(n_heads + 1, np.int32)
    np.cumsum([r.size for r in out], out=offsets[1:])
    return np.ascontiguousarray(rows, dtype=np.int32), offsets


def sorted_thresholds(thresholds):
    """The caller's thresholds -> (float64 [T] as given, the distinct non-NaN ones ascending, for every threshold the index of its
    value in that list or -1 for a NaN).  Duplicates share an entry; +-inf are ordinary values."""
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr.size < 1:
        raise ValueError("at least one threshold")
    ok = ~np.isnan(thr)
    distinct = np.unique(thr[ok])
    where = np.full(thr.size, -1, np.int64)
    where[ok] = np.searchsorted(distinct, thr[ok])
    return thr, distinct, where


def roc_counts_on_device(probs, positives, negatives, thresholds, target_id=2, multiclass=False, negative_class=1):
    """probs: CUDA tensor or numpy array [K, N, C] float32 (what Head.forward_many returns); positives / negatives: K lists of row
    indices into a head's own plane (a row listed twice counts twice); thresholds: T floats in any order.
    -> (counts int32 [K, T, 2] = entries of each list with (float64)score > threshold, totals int32 [K, 2] = the list lengths).
    multiclass=False scores p[row][target_id] (roc_single_target); multiclass=True follows roc_sc on evaluate_files_multiclass dicts:
    a = argmax of the row, a positive takes part when a == target_id, a negative when a != negative_class, the score is p[row][a].
    A NaN threshold gets zeros.  One upload (row lists, offsets, thresholds), one launch, one copy back."""
    import torch
    if not torch.is_tensor(probs):
        probs = np.asarray(probs)
        if probs.dtype != np.float32:
            raise ValueError("probs must be float32: the comparison widens float32 probabilities, as the reference's arrays are")
    if probs.ndim != 3:
        raise ValueError("probs must be [heads, rows, classes]")
    K, N, C = (int(x) for x in probs.shape)
    if C < 1 or not 0 <= int(target_id) < C:
        raise ValueError(f"target_id {target_id} outside [0, {C})")
    if multiclass and not 0 <= int(negative_class) < C:
        raise ValueError(f"negative_class {negative_class} outside [0, {C})")
    pos, pos_off = pack_rows(positives, K, N, "positives")                  # refused before anything is uploaded
    neg, neg_off = pack_rows(negatives, K, N, "negatives")
    thr, distinct, where = sorted_thresholds(thresholds)
    totals = np.stack([np.diff(pos_off), np.diff(neg_off)], axis=1).astype(np.int32)
    T, D = int(thr.size), int(distinct.size)
    counts = np.zeros((K, T, 2), np.int32)
    if K == 0 or D == 0:
        return counts, totals
    if not torch.is_tensor(probs):
        probs = torch.from_numpy(np.ascontiguousarray(probs)).cuda()
    if not probs.is_cuda or probs.dtype != torch.float32:
        raise ValueError("probs must be a CUDA tensor or numpy array [heads, rows, classes] of float32")
    probs = probs.contiguous()
    L = _lib.lib()
    dev = probs.device
    with torch.cuda.device(dev):
        # one upload of 8-byte words: the bit patterns of the float64 thresholds, then the int32 offsets and row lists in pairs
        d_in, (p_thr, p_pos_off, p_neg_off, p_pos, p_neg) = _lib.upload_words([distinct, pos_off, neg_off, pos, neg], dev)
        # counts of every piece of thresholds and the invalid-entry counters in ONE buffer, so that they cross in one copy
        d_out = torch.empty(K * D * 2 + K, dtype=torch.int32, device=dev)
        base, stream, done = d_out.data_ptr(), _lib.current_stream_ptr(), 0
        pieces = []
        for t0 in range(0, D, MAX_THRESHOLDS):
            t = min(MAX_THRESHOLDS, D - t0)
            pieces.append((t0, t, done))
            _lib.check(L.mkws_roc_count(probs.data_ptr() if N else None, K, N, C, p_pos, p_pos_off, p_neg, p_neg_off, p_thr + 8 * t0, t,
                                        int(bool(multiclass)), int(target_id), int(negative_class) if multiclass else 0,
                                        base + 4 * done, base + 4 * K * D * 2, stream))
            done += K * t * 2
        out = d_out.cpu().numpy()                                      # the call's one synchronisation
    invalid = out[K * D * 2:]
    if invalid.any():
        k = int(np.nonzero(invalid)[0][0])
        raise RuntimeError(f"head {k}: {int(invalid[k])} row indices outside [0, {N}) reached the device")
    by_value = np.empty((K, D, 2), np.int32)
    for t0, t, at in pieces:
        by_value[:, t0:t0 + t] = out[at:at + K * t * 2].reshape(K, t, 2)
    ok = where >= 0
    counts[:, ok] = by_value[:, where[ok]]
    return counts, totals
