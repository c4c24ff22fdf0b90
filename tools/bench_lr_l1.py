"""The DataPerf selection harness with the reference's `logistic_regression_with_l1_regularization`
(notebooks/dataperf_test_harness.py:277-280): every split fitted and scored with sklearn's LogisticRegression(penalty="l1",
solver="liblinear") on the host, as the reference does it, against selection_eval.experiment_run_many(classifier="lr_l1") with all
splits of all experiments in one mkws_lr_l1_fit and two mkws_logreg_score launches.  One process, one MI355X.

Workload: that of tools/bench_selection_eval.py -- --experiments 20 x --splits 10 = 200 problems of 200 rows (5 words x 20 target rows +
100 unknown rows), 6 classes, on the 1024-D embeddings one synthetic handle makes of seeded tone-plus-noise clips.  Alternated run by
run, one warm-up each, medians of --repeats runs (min and max beside them):

  (a) the route before: the bank copied to the host, then per split LogisticRegression(penalty="l1", solver="liblinear").fit and .score,
      per experiment the best split's .score on the dev rows (one process)
  (b) one experiment_run_many(classifier="lr_l1") on the bank where the embedding left it: ends in the device-to-host copy of the dev counts

Both routes use the same rows and the same splits.  Printed, not asserted: the device's iteration counts and stop reasons, the float64
objective gap (f - f*) / f* of both routes summed over the classes of the first --gap-problems problems (f* from lr_l1.lr_l1_host), and
the number of experiments whose chosen split or score differ.  Without sklearn route (a) is reported as NOT MEASURED.

  python tools/bench_lr_l1.py [--experiments 20] [--splits 10] [--repeats 3] [--gap-problems 2] [--commit HASH] [--out profiles/lr_l1_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_WORDS, N_TAKES, N_WORD_TRAIN, N_UNKNOWN, WORDS_PER_EXPERIMENT, TARGET_ROWS = 30, 40, 30, 100, 5, 20


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--experiments", type=int, default=20)
    ap.add_argument("--splits", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--gap-problems", type=int, default=2)
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from multilingual_kws_amd import lr_l1, synth, weights
    from multilingual_kws_amd.embedding import selection_eval as se
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    from multilingual_kws_amd.frontend import Frontend
    assert torch.cuda.is_available(), "bench_lr_l1.py measures on a GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    try:
        import sklearn.linear_model
        import sklearn.model_selection
    except ImportError:
        sklearn = None
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    # ---- the bank of tools/bench_selection_eval.py: word w = tone w in N_TAKES noisy takes, then 2 * N_UNKNOWN clips of tones no word has
    takes = [w + 128 * j for w in range(N_WORDS) for j in range(N_TAKES)] + [N_WORDS + (u % 90) + 128 * (50 + u // 90) for u in range(2 * N_UNKNOWN)]
    batch = 200
    em, fe = EmbeddingModel(weights.synthetic_blob(), max_batch=batch, device=dev), Frontend()
    d_bank = torch.empty((len(takes), 1024), dtype=torch.float32, device=dev)
    for s in range(0, len(takes), batch):
        audio = np.concatenate([synth.clips_float32(1, first_clip=t) for t in takes[s:s + batch]])
        em.forward(fe.forward(torch.from_numpy(audio).to(dev)), out=d_bank[s:s + len(audio)])
    torch.cuda.synchronize()
    word_rows = [np.arange(w * N_TAKES, (w + 1) * N_TAKES) for w in range(N_WORDS)]
    ut = N_WORDS * N_TAKES + np.arange(N_UNKNOWN)
    ue = ut + N_UNKNOWN
    rng = np.random.RandomState(0)
    exps, splits = [], []
    for e in range(args.experiments):
        ws = rng.choice(N_WORDS, WORDS_PER_EXPERIMENT, replace=False)
        exps.append(dict(words=[f"word{w}" for w in ws], train_rows=[word_rows[w][:N_WORD_TRAIN] for w in ws], dev_rows=[word_rows[w][N_WORD_TRAIN:] for w in ws]))
        y = np.repeat(np.arange(1, WORDS_PER_EXPERIMENT + 1), N_WORD_TRAIN)
        if sklearn is not None:
            sel = sklearn.model_selection.StratifiedShuffleSplit(n_splits=args.splits, train_size=WORDS_PER_EXPERIMENT * TARGET_ROWS, random_state=e)
            splits.append(list(sel.split(np.zeros((len(y), 1)), y)))
        else:
            splits.append(se.stratified_shuffle_splits(y, args.splits, WORDS_PER_EXPERIMENT * TARGET_ROWS, seed=e))
    K, fit_l, val_l, dev_l, _ = se._lists(exps, ut, ue, splits)
    n_problems = len(fit_l[2]) - 1
    say(f"bench_lr_l1 @ {commit}: {args.experiments} experiments x {args.splits} splits = {n_problems} problems of "
        f"{int(np.diff(fit_l[2]).max())} rows, {K} classes, dim 1024; bank of {len(takes)} vectors; sklearn "
        f"{sklearn.__version__ if sklearn is not None else 'absent'}; {torch.cuda.get_device_name(0)}")

    models = {}

    def route_a():
        """The reference's loop on the lists of route (b): ends on the host, starts with the bank's device-to-host copy."""
        bank = d_bank.cpu().numpy()
        out = []
        for e in range(args.experiments):
            scores, clfs = [], []
            for s in range(args.splits):
                p = e * args.splits + s
                a, b, va, vb = fit_l[2][p], fit_l[2][p + 1], val_l[2][p], val_l[2][p + 1]
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    clf = sklearn.linear_model.LogisticRegression(penalty="l1", solver="liblinear").fit(bank[fit_l[0][a:b]], fit_l[1][a:b])
                clfs.append(clf)
                scores.append(clf.score(bank[val_l[0][va:vb]], val_l[1][va:vb]))
                if p < args.gap_problems:
                    models[p] = clf
            best = int(np.argmax(scores))
            da, db = dev_l[2][e], dev_l[2][e + 1]
            out.append(dict(words=exps[e]["words"], score=clfs[best].score(bank[dev_l[0][da:db]], dev_l[1][da:db]), crossfold_scores=scores, best_split=best))
        return out

    def route_b():
        return se.experiment_run_many(d_bank, exps, ut, ue, splits, classifier="lr_l1")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    routes = [("b", route_b)] + ([("a", route_a)] if sklearn is not None else [])
    times, results = {name: [] for name, _ in routes}, {}
    for name, fn in routes:
        _, results[name] = timed(fn)                                  # the warm-up
    for _ in range(args.repeats):
        for name, fn in routes:
            t, _ = timed(fn)
            times[name].append(t)
    fmt = lambda ts: f"{statistics.median(ts) * 1e3:10.1f} ms  (min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f}, {len(ts)} runs)"
    if sklearn is not None:
        say(f"  (a) sklearn LogisticRegression(penalty=l1, liblinear) per split on the host: {fmt(times['a'])}")
    else:
        say("  (a) sklearn LogisticRegression(penalty=l1, liblinear) per split on the host: NOT MEASURED (sklearn is not installed here)")
    say(f"  (b) experiment_run_many(classifier=lr_l1), one fit and two score launches  : {fmt(times['b'])}")
    if sklearn is not None:
        say(f"      (a) / (b) = {statistics.median(times['a']) / statistics.median(times['b']):.1f}")

    # ---- how converged either route is, and whether they choose alike (printed, not asserted)
    fit_times = []
    for _ in range(1 + args.repeats):                                 # (the first is a warm-up)
        t, fit = timed(lambda: lr_l1.fit_on_device(d_bank, *fit_l, K))
        fit_times.append(t)
    say(f"      of (b), fit_on_device alone (upload, launch, copy back of {n_problems} x {K} x 1024 coefficients): {fmt(fit_times[1:])}")
    n_iter = fit.info[:, :, 1]
    say(f"  device iterations per class: min {int(n_iter.min())}, median {int(np.median(n_iter))}, max {int(n_iter.max())} (max_iter {lr_l1.MAX_ITER}); stopped on the "
        f"violation: {int((fit.info[:, :, 2] == 0).sum())} of {n_iter.size}; violation at the stop: median {np.median(fit.stats[:, :, 1]):.2e}, max "
        f"{fit.stats[:, :, 1].max():.2e}; non-zero weights per class: median {int(np.median(fit.info[:, :, 3]))}, max {int(fit.info[:, :, 3].max())} of 1024")
    bank = d_bank.cpu().numpy()
    gaps_a, gaps_b = [], []
    for p in range(min(args.gap_problems, n_problems)):
        a, b = fit_l[2][p], fit_l[2][p + 1]
        rows, y = fit_l[0][a:b], fit_l[1][a:b]
        star = lr_l1.lr_l1_host(bank, rows, y, K)
        gaps_b.append((lr_l1.objective(bank, rows, y, K, 1.0, fit.coef[p], fit.intercept[p])[0].sum() - star.f.sum()) / star.f.sum())
        if p in models and len(models[p].classes_) == K:
            gaps_a.append((lr_l1.objective(bank, rows, y, K, 1.0, models[p].coef_, models[p].intercept_)[0].sum() - star.f.sum()) / star.f.sum())
    if gaps_b:
        say(f"  (f - f*) / f* summed over the classes, first {len(gaps_b)} problems: (b) max {max(gaps_b):.3e}" + (f"; (a) max {max(gaps_a):.3e}" if gaps_a else ""))
    if sklearn is not None:
        differ = sum(1 for ra, rb in zip(results["a"], results["b"]) if ra["best_split"] != rb["best_split"] or ra["score"] != rb["score"])
        say(f"  experiments whose chosen split or score differ between (a) and (b): {differ} of {args.experiments}")
        say(f"  mean score: (a) {np.mean([r['score'] for r in results['a']]):.4f}, (b) {np.mean([r['score'] for r in results['b']]):.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
