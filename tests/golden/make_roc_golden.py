"""Generates tests/golden/roc_golden.json: the REFERENCE's own roc_single_target, roc_sc and calc_roc run on seeded inputs.

    python tests/golden/make_roc_golden.py <checkout of the reference>

multilingual_kws/embedding/transfer_learning_analysis.py imports TensorFlow and runs a script body, so it cannot be imported: the
three function definitions are lifted out of its syntax tree and compiled on their own, with numpy as their only global.  Only inputs
and outputs are committed; no test reads the reference.

Every case is a probability table [rows, classes] of float32 values plus lists of row indices (duplicates on purpose), so that the same
case can be fed to the host functions and to mkws_roc_count.  The winning score of most rows is the float32 rounding of one of the 101
thresholds or its neighbour one ulp below / above -- where a float32 comparison and the float64 one the reference makes disagree."""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WANTED = ("roc_single_target", "roc_sc", "calc_roc")


def lift(reference_root):
    path = os.path.join(reference_root, "multilingual_kws", "embedding", "transfer_learning_analysis.py")
    tree = ast.parse(open(path).read(), path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(d.name for d in defs) == sorted(WANTED)
    ns = {"np": np}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in WANTED]


def near_thresholds(rng, n):
    """n float32 scores: float32(thr), one ulp below or one ulp above, thr drawn from the 101 default thresholds."""
    thr = np.arange(0, 1.01, 0.01)[rng.integers(0, 101, n)].astype(np.float32)
    step = rng.integers(-1, 2, n)
    out = np.where(step < 0, np.nextafter(thr, np.float32(-1)), np.where(step > 0, np.nextafter(thr, np.float32(2)), thr))
    return out.astype(np.float32)


def table(rng, n, classes):
    """[n, classes] float32: one winning class per row with a near-threshold score, the others a fraction of it."""
    win = near_thresholds(rng, n)
    p = (win[:, None] * rng.uniform(0, 0.9, (n, classes))).astype(np.float32)
    p[np.arange(n), rng.integers(0, classes, n)] = win
    return p


def split(preds, class_id):
    """evaluate_files_multiclass's dict (reference transfer_learning.py: argmax per row, "correct" when it is class_id)."""
    correct, incorrect = [], []
    for row, col in enumerate(np.argmax(preds, axis=1) if len(preds) else []):
        (correct if col == class_id else incorrect).append(preds[row][col])
    return dict(correct=correct, incorrect=incorrect)


def rows(rng, n, count):
    return [int(r) for r in rng.integers(0, n, count)]


def main():
    roc_single_target, roc_sc, calc_roc = lift(sys.argv[1])
    rng = np.random.default_rng(2024)
    cases = []
    # roc_single_target: the target column of both lists
    for i, (n, classes, target, n_pos, n_neg) in enumerate([(1, 1, 0, 1, 1), (40, 3, 2, 25, 60), (64, 3, 2, 64, 7), (90, 1, 0, 100, 33),
                                                           (33, 8, 5, 12, 90)]):
        p = table(rng, n, classes)
        pos, neg = rows(rng, n, n_pos), rows(rng, n, n_neg)
        tprs, fprs, threshs = roc_single_target(p[pos, target], p[neg, target])
        assert np.array_equal(threshs, np.arange(0, 1.01, 0.01))
        cases.append(dict(function="roc_single_target", probs=p.tolist(), target_id=target, positives=pos, negatives=neg, tprs=tprs, fprs=fprs))
    # roc_sc: argmax dicts; exact ties between the winning classes in both orders, and (one case) rows holding a NaN
    for i, (n, classes, target, unknown, n_pos, n_neg) in enumerate([(30, 2, 1, 0, 40, 40), (50, 3, 2, 1, 30, 80), (50, 3, 0, 2, 70, 20),
                                                                    (40, 8, 7, 3, 45, 45), (45, 3, 2, 1, 50, 60)]):
        p = table(rng, n, classes)
        for r in range(0, n, 5):                          # ties: the maximum twice, the target class first or last of the pair
            a, b = (target, unknown) if (r // 5) % 2 else (unknown, target)
            p[r, a] = p[r, b] = p[r].max()
        if i == 4:
            p[3, 0] = p[17, classes - 1] = np.nan
        pos, neg = rows(rng, n, n_pos), rows(rng, n, n_neg)
        if i == 4:
            pos[0], neg[0], neg[1] = 3, 17, 3
        tprs, fprs, threshs = roc_sc(split(p[pos], target), split(p[neg], unknown))
        cases.append(dict(function="roc_sc", probs=p.tolist(), target_id=target, negative_class=unknown, positives=pos, negatives=neg,
                          tprs=tprs, fprs=fprs))
    # calc_roc: three groups of non-target clips, pooled
    for n, classes, target, unknown in [(60, 2, 1, 0), (48, 3, 2, 1)]:
        p = table(rng, n, classes)
        pos = rows(rng, n, 35)
        groups = {"oov": rows(rng, n, 30), "unknown_training": rows(rng, n, 11), "original_embedding": rows(rng, n, 50)}
        res = {"target_keywords": split(p[pos], target)}
        res.update({k: split(p[v], unknown) for k, v in groups.items()})
        tprs, fprs = calc_roc(res)
        cases.append(dict(function="calc_roc", probs=p.tolist(), target_id=target, negative_class=unknown, positives=pos, groups=groups,
                          tprs=tprs, fprs=fprs))
    doc = {"source": "roc_single_target, roc_sc and calc_roc of multilingual_kws/embedding/transfer_learning_analysis.py run on seeded inputs",
           "cases": cases}
    with open(os.path.join(HERE, "roc_golden.json"), "w") as f:
        json.dump(doc, f)
    print(len(cases), "cases,", os.path.getsize(os.path.join(HERE, "roc_golden.json")), "bytes")


if __name__ == "__main__":
    main()
