"""The DataPerf selection harness with the classifier its experiment_run really fits (notebooks/dataperf_test_harness.py:386-393):
VotingClassifier([SVC(probability=True), LogisticRegression()], voting="soft") per split on the host, as the reference does it, against
selection_eval.experiment_run_many(classifier="vote") with all splits of all experiments side by side on the device.  One process, one
MI355X.

Workload (that of tools/bench_svc.py): --experiments 20 x --splits 10 = 200 problems of 200 rows (5 words x 20 target rows + 100 unknown
rows), 6 classes = 15 pairwise machines each, every machine fitted once on all rows and once per fold, on the 1024-D embeddings one
synthetic handle makes of seeded tone-plus-noise clips.  Alternated run by run, one warm-up each, medians of --repeats runs:

  (a) the route before: the bank copied to the host, then per split VotingClassifier.fit and .score, per experiment the best split's
      .score on the dev rows (one process; the reference spreads this loop over a multiprocessing.Pool of 8)
  (b) one experiment_run_many(classifier="vote") on the bank where the embedding left it

Both routes use the same rows and splits; the folds of Platt scaling's cross-validation are libsvm's own unseeded draw in (a) and
svc.cv_folds(seed 0) in (b).  The phases of (b) are timed apart with device events in runs of their own.  Printed, not asserted: the
device's iteration counts, and the number of experiments whose chosen split or score differ.  Without sklearn route (a) is reported as
NOT MEASURED.  No threshold is fixed in advance: the baseline is route (a) in the same run.

  python tools/bench_vote.py [--experiments 20] [--splits 10] [--repeats 3] [--commit HASH] [--out profiles/vote.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_svc import N_TAKES, N_UNKNOWN, N_WORD_TRAIN, N_WORDS, TARGET_ROWS, WORDS_PER_EXPERIMENT  # noqa: E402

N_FOLDS = 5


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--experiments", type=int, default=20)
    ap.add_argument("--splits", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from multilingual_kws_amd import logreg, svc, synth, weights
    from multilingual_kws_amd.embedding import selection_eval as se
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    from multilingual_kws_amd.frontend import Frontend
    assert torch.cuda.is_available(), "bench_vote.py measures on a GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    try:
        import sklearn.ensemble
        import sklearn.linear_model
        import sklearn.model_selection
        import sklearn.svm
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

    # ---- the bank and the lists of tools/bench_svc.py
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
    n_problems, npairs = len(fit_l[2]) - 1, K * (K - 1) // 2
    say(f"bench_vote @ {commit}: {args.experiments} experiments x {args.splits} splits = {n_problems} problems of "
        f"{int(np.diff(fit_l[2]).max())} rows, {K} classes, {N_FOLDS} folds, dim 1024; bank of {len(takes)} vectors; sklearn "
        f"{sklearn.__version__ if sklearn is not None else 'absent'}; {torch.cuda.get_device_name(0)}")

    def route_a():
        """The reference's loop on the lists of route (b): ends on the host, starts with the bank's device-to-host copy."""
        bank = d_bank.cpu().numpy()
        out = []
        for e in range(args.experiments):
            scores, clfs = [], []
            for s in range(args.splits):
                p = e * args.splits + s
                a, b, va, vb = fit_l[2][p], fit_l[2][p + 1], val_l[2][p], val_l[2][p + 1]
                clf = sklearn.ensemble.VotingClassifier(estimators=[("svm", sklearn.svm.SVC(probability=True)), ("lr", sklearn.linear_model.LogisticRegression())],
                                                        voting="soft", weights=None)
                clf.fit(bank[fit_l[0][a:b]], fit_l[1][a:b])
                clfs.append(clf)
                scores.append(clf.score(bank[val_l[0][va:vb]], val_l[1][va:vb]))
            best = int(np.argmax(scores))
            da, db = dev_l[2][e], dev_l[2][e + 1]
            out.append(dict(words=exps[e]["words"], score=clfs[best].score(bank[dev_l[0][da:db]], dev_l[1][da:db]), crossfold_scores=scores, best_split=best))
        return out

    def route_b():
        return se.experiment_run_many(d_bank, exps, ut, ue, splits, classifier="vote", n_folds=N_FOLDS)

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
    fmt = lambda ts: f"{statistics.median(ts) * 1e3:10.2f} ms  (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}, {len(ts)} runs)"
    if sklearn is not None:
        say(f"  (a) sklearn VotingClassifier per split on the host     : {fmt(times['a'])}")
    else:
        say("  (a) sklearn VotingClassifier per split on the host     : NOT MEASURED (sklearn is not installed here)")
    say(f"  (b) experiment_run_many(classifier=\"vote\")              : {fmt(times['b'])}")
    if sklearn is not None:
        say(f"      (a) / (b) = {statistics.median(times['a']) / statistics.median(times['b']):.1f}")

    # ---- the phases of (b), by device events, in runs of their own
    names = ("logreg", "prepare", "gram", "smo", "cv", "platt", "lr_score", "score", "couple", "vote")
    phases = {k: [] for k in names}

    def span(t, key, fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        ev[1].synchronize()
        t[key] = ev[0].elapsed_time(ev[1])
        return out

    for r in range(1 + args.repeats):                                 # (the first is a warm-up)
        t = {}
        lr = span(t, "logreg", lambda: logreg.fit_on_device(d_bank, *fit_l, K))
        fit = svc.fit_proba_on_device(d_bank, *fit_l, K, n_folds=N_FOLDS, tol=1e-5, timings=t)
        p_lr = span(t, "lr_score", lambda: logreg.score_on_device(d_bank, *val_l, lr.d_coef, lr.d_intercept, want_probs=True)[2])
        dec = svc.score_on_device(d_bank, *val_l, *fit_l, K, fit.d_coef, fit.d_rho, fit.d_gamma, fit.d_centre, fit.d_inv_scale, want_decision=True,
                                  timings=t)[2]
        p_sv = span(t, "couple", lambda: svc.couple_on_device(dec, val_l[1], val_l[2], fit.d_probA, fit.d_probB, fit.d_present)[2])
        span(t, "vote", lambda: svc.soft_vote_on_device(p_sv, p_lr, val_l[1], val_l[2]))
        if r:
            for k in phases:
                phases[k].append(t[k] * 1e-3)
    what = dict(logreg=f"logreg.fit_on_device ({n_problems} problems, with its copy back)", prepare="mkws_svc_prepare (centre, scale, gamma)",
                gram=f"mkws_svc_kernel ({n_problems} Gram matrices)", smo=f"mkws_svc_fit ({n_problems} x {npairs} pairs)",
                cv=f"mkws_svc_fit_cv ({n_problems} x {npairs} x {N_FOLDS} sub-fits)", platt=f"mkws_svc_platt ({n_problems} x {npairs} sigmoids)",
                lr_score=f"mkws_logreg_score ({len(val_l[0])} validation rows)", score=f"mkws_svc_score ({len(val_l[0])} validation rows)",
                couple="mkws_svc_couple (with its list uploads)", vote="mkws_soft_vote (with its list uploads)")
    for k in names:
        say(f"      of (b), {what[k]:<58}: {fmt(phases[k])}")
    say(f"  device sub-fits solved {int(fit.cv_info[:, 1].sum())}, cut at max_iter {int(fit.cv_info[:, 2].sum())}; SMO iterations of the slowest sub-fit of a "
        f"problem: median {int(np.median(fit.cv_info[:, 3]))}, max {int(fit.cv_info[:, 3].max())} (whole-pair fits: median {int(np.median(fit.info[:, 3]))}, "
        f"max {int(fit.info[:, 3].max())})")
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
