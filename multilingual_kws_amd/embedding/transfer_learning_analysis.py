"""The ROC functions of multilingual_kws/embedding/transfer_learning_analysis.py (:181-222, :345-404; copied there into quick_viz.py,
band_viz.py and roc_hyperparams.py), and their many-keyword form.

roc_single_target, roc_sc and calc_roc carry the reference's signatures and return values and are the HOST SPECIFICATION of
mkws_roc_count (include/mkws.h): they run without a GPU.  The one thing the reference leaves implicit is made explicit here: its
`scores[scores > threshold]` compares a float32 array with an element of np.arange(0, 1.01, 0.01), an np.float64, and NumPy widens
the array -- the comparison is (float64)score > threshold, never the float32 one.  roc_many scores K heads over shared clips in one
device launch (..roc.roc_counts_on_device) and returns what the host functions return for each head."""
import numpy as np


def default_thresholds():
    """The reference's 101 thresholds."""
    return np.arange(0, 1.01, 0.01)


def _above(scores, threshold):
    """Entries of `scores` (any float dtype, may be empty) strictly above the float64 threshold, compared in float64."""
    return int(np.count_nonzero(np.asarray(scores, dtype=np.float64) > np.float64(threshold)))


def _curve(target_scores, total_positives, unknown_scores, unknown_total, threshs):
    tprs, fprs = [], []
    for threshold in threshs:
        tprs.append(_above(target_scores, threshold) / total_positives)     # ints: an empty side raises ZeroDivisionError, as the reference's division does
        fprs.append(_above(unknown_scores, threshold) / unknown_total)
    return tprs, fprs


def roc_single_target(target_results, unknown_results):
    """target_results / unknown_results: the target-class confidences of the target clips / of the non-target clips
    (evaluate_files_single_target(...)[0]).  -> (tprs, fprs, threshs): the share of each above every threshold.
    _TARGET_ is class 2, _UNKNOWN_ is class 1."""
    threshs = default_thresholds()
    tprs, fprs = _curve(target_results, len(target_results), unknown_results, len(unknown_results), threshs)
    return tprs, fprs, threshs


def _sc_curve(target_resuts, unknown_results, threshs):
    # true positives: target clips classified as the target, by confidence; false positives: non-target clips classified as
    # anything but their own class ("incorrect"), by confidence.  The totals count every clip of a side.
    total_positives = len(target_resuts["correct"]) + len(target_resuts["incorrect"])
    unknown_total = len(unknown_results["correct"]) + len(unknown_results["incorrect"])
    return _curve(target_resuts["correct"], total_positives, unknown_results["incorrect"], unknown_total, threshs)


def roc_sc(target_resuts, unknown_results):
    """Both arguments are evaluate_files_multiclass dicts {"correct": [...], "incorrect": [...]} of argmax confidences: the target
    clips judged against the target class, the non-target clips against the unknown class.  -> (tprs, fprs, threshs)."""
    threshs = default_thresholds()
    tprs, fprs = _sc_curve(target_resuts, unknown_results, threshs)
    return tprs, fprs, threshs


def calc_roc(res):
    """res: {"target_keywords", "oov", "unknown_training", "original_embedding"} -> evaluate_files_multiclass dicts.  The three
    non-target groups are pooled.  -> (tprs, fprs) at the 101 default thresholds."""
    target = res["target_keywords"]
    groups = [res[k] for k in ("oov", "unknown_training", "original_embedding")]
    total_positives = len(target["correct"]) + len(target["incorrect"])
    total_negatives = sum(len(g["correct"]) + len(g["incorrect"]) for g in groups)
    false_positives = np.concatenate([np.asarray(g["incorrect"], dtype=np.float64) for g in groups])
    return _curve(target["correct"], total_positives, false_positives, total_negatives, default_thresholds())


def split_confidences(preds, class_id):
    """evaluate_files_multiclass's dict for the rows of `preds` [n, classes]: the argmax confidence of each row, under "correct" when the
    argmax is class_id (np.argmax: ties go to the lower index, a NaN wins)."""
    correct, incorrect = [], []
    preds = np.asarray(preds)
    for row, col in enumerate(np.argmax(preds, axis=1) if len(preds) else []):
        (correct if col == class_id else incorrect).append(preds[row][col])
    return dict(correct=correct, incorrect=incorrect)


def roc_many(probs, positives, negatives, thresholds=None, multiclass=False, target_id=2, negative_class=1):
    """ROC of K keyword heads over shared clips.  probs [K, N, C] float32, CUDA tensor or numpy array: head k's class probabilities of
    all N clips; positives / negatives: K lists of row indices, head k's target clips and its non-target clips (a row listed twice
    counts twice, as a file listed twice does in the reference); thresholds: any order, default the reference's 101.
    -> K tuples (tprs, fprs, threshs), each equal to roc_single_target(probs[k][positives[k], target_id], probs[k][negatives[k],
    target_id]) -- or, with multiclass=True, to roc_sc on the evaluate_files_multiclass dicts of the same rows (target clips against
    target_id, non-target clips against negative_class) -- at these thresholds.  An empty side raises ZeroDivisionError.
    CUDA input, and numpy input on a host with a GPU, are counted on the device in one launch (..roc.roc_counts_on_device) and the
    rates are count / total in Python on those integers; numpy input on a host without a GPU loops over the host functions."""
    import torch
    from ..roc import pack_rows
    on_device = torch.is_tensor(probs)
    if not on_device:
        probs = np.asarray(probs)
    if probs.ndim != 3:
        raise ValueError("probs must be [heads, rows, classes]")
    if probs.dtype != (torch.float32 if on_device else np.float32):
        raise ValueError("probs must be float32: the comparison widens float32 probabilities, as the reference's arrays are")
    K, N, C = (int(x) for x in probs.shape)
    if not 0 <= int(target_id) < C:
        raise ValueError(f"target_id {target_id} outside [0, {C})")
    if multiclass and not 0 <= int(negative_class) < C:
        raise ValueError(f"negative_class {negative_class} outside [0, {C})")
    threshs = default_thresholds() if thresholds is None else np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if threshs.size < 1:
        raise ValueError("at least one threshold")
    pos, pos_off = pack_rows(positives, K, N, "positives")
    neg, neg_off = pack_rows(negatives, K, N, "negatives")
    out = []
    if not on_device and not torch.cuda.is_available():
        for k in range(K):
            p, n = probs[k][pos[pos_off[k]:pos_off[k + 1]]], probs[k][neg[neg_off[k]:neg_off[k + 1]]]
            if multiclass:
                tprs, fprs = _sc_curve(split_confidences(p, target_id), split_confidences(n, negative_class), threshs)
            else:
                tprs, fprs = _curve(p[:, target_id], len(p), n[:, target_id], len(n), threshs)
            out.append((tprs, fprs, threshs.copy()))
        return out
    from ..roc import roc_counts_on_device
    counts, totals = roc_counts_on_device(probs, positives, negatives, threshs, target_id=target_id, multiclass=multiclass,
                                          negative_class=negative_class)
    counts, totals = counts.tolist(), totals.tolist()
    for k in range(K):
        total_positives, unknown_total = totals[k]
        tprs = [c[0] / total_positives for c in counts[k]]
        fprs = [c[1] / unknown_total for c in counts[k]]
        out.append((tprs, fprs, threshs.copy()))
    return out
