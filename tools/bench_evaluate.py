"""The point scorer (multilingual_kws_amd/scoring.py) against the torch compositions the package's scoring loops
use today, and model.evaluate against a loop in the shape of transfer_learning._validate.  One process, one MI355X, everything resident on
the device.

  (a) [64, 8192, 3] probabilities, shared labels: Scorer.add against gather -> clamp -> log -> sum; argmax -> eq -> sum; one
      torch.bincount per model
  (b) [1, 8192, 761] logits: Scorer.add against cross_entropy(reduction="sum") + argmax + bincount
  (c) TransferLearnedModel.evaluate over 4096 device-resident clips at batch_size 32 (128 batches, one copy to the host at the end)
      against the _validate loop (the same forwards; gather, clamp, log, argmax in torch and a float() synchronisation per batch)

The integers of both routes are compared before anything is timed.  Then warm-up and device-synchronised windows of --calls calls each,
the routes alternating in the same process, --windows windows of each: medians, spread (min .. max of the windows), ratio of the medians.
The comparators are written as the loops are; they are not tuned.

  python tools/bench_evaluate.py [--calls 50] [--windows 9] [--out profiles/evaluate_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50, help="calls per synchronised window of (a) and (b)")
    ap.add_argument("--evaluate-calls", type=int, default=5, help="evaluate passes per synchronised window of (c)")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--clips", type=int, default=4096, help="clips of (c)")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from multilingual_kws_amd import scoring, synth
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.frontend import Frontend
    from multilingual_kws_amd.head import Head, glorot_uniform_params
    assert torch.cuda.is_available(), "bench_evaluate.py measures on a GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
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

    say(f"# tools/bench_evaluate.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")

    def measure(title, routes, calls, unit="us"):
        scale = 1e6 if unit == "us" else 1e3

        def window(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / calls * scale

        for fn in routes.values():                # warm-up: code objects, the allocator's blocks
            for _ in range(3 if unit == "ms" else 10):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in routes}
        for _ in range(args.windows):             # the routes alternate, window by window
            for name, fn in routes.items():
                times[name].append(window(fn))
        say(f"{title}; {args.windows} windows of {calls} calls each, alternating; {unit} per call")
        med = {}
        for name, ts in times.items():
            med[name] = statistics.median(ts)
            say(f"  {name:22s} median {med[name]:10.2f}   min {min(ts):10.2f}   max {max(ts):10.2f}")
        return med

    def verdict(what, med, ours, theirs, expect):
        ratio = med[theirs] / med[ours]
        ok = ratio > 1.0 if expect == "faster" else ratio >= 0.95
        say(f"{what}: {ours} vs {theirs}: {ratio:.2f}x (medians); {'PASS' if ok else 'MISS'}: expected "
            f"{'faster than' if expect == 'faster' else 'no slower than'} the comparator")
        say()

    rng = np.random.default_rng(0)

    # (a) 64 models x 8192 rows x 3 probabilities
    K, N, C = 64, 8192, 3
    z = rng.standard_normal((K, N, C)).astype(np.float32) * 3
    probs = torch.softmax(torch.from_numpy(z).to(dev), dim=2).contiguous()
    labels = torch.from_numpy(rng.integers(0, C, N).astype(np.int32)).to(dev)
    idx = labels.long()
    scorer_a = scoring.Scorer(K, C, 0, device=dev)
    scorer_a.reserve(N)

    def torch_a():
        picked = probs.gather(2, idx.view(1, N, 1).expand(K, N, 1)).squeeze(2)
        loss = -torch.log(torch.clamp(picked, min=1e-7)).sum(1)
        pred = probs.argmax(2)
        correct = (pred == idx).sum(1)
        cms = [torch.bincount(idx * C + pred[k], minlength=C * C) for k in range(K)]
        return loss, correct, cms

    scorer_a.add(probs, labels)
    got = scorer_a.result()
    loss, correct, cms = torch_a()
    assert got.correct.tolist() == correct.cpu().tolist() and np.array_equal(got.confusion_matrix.reshape(K, -1), torch.stack(cms).cpu().numpy())
    assert np.allclose(got.loss_sum, loss.double().cpu().numpy(), rtol=1e-4), "the routes' losses differ: nothing is timed"
    med = measure(f"(a) {K} x {N} x {C} probabilities", {"Scorer.add": lambda: scorer_a.add(probs, labels), "torch composition": torch_a}, args.calls)
    verdict("(a)", med, "Scorer.add", "torch composition", "faster")

    # (b) 1 model x 8192 rows x 761 logits
    K, N, C = 1, 8192, 761
    logits = torch.from_numpy(rng.standard_normal((N, C)).astype(np.float32) * 4).to(dev)
    labels_b = torch.from_numpy(rng.integers(0, C, N).astype(np.int32)).to(dev)
    idx_b = labels_b.long()
    scorer_b = scoring.Scorer(K, C, 1, device=dev)
    scorer_b.reserve(N)

    def torch_b():
        loss = torch.nn.functional.cross_entropy(logits, idx_b, reduction="sum")
        pred = logits.argmax(1)
        return loss, (pred == idx_b).sum(), torch.bincount(idx_b * C + pred, minlength=C * C)

    scorer_b.add(logits, labels_b)
    got = scorer_b.result()
    loss, correct, cm = torch_b()
    assert int(got.correct[0]) == int(correct.cpu()) and np.array_equal(got.confusion_matrix.reshape(-1), cm.cpu().numpy())
    assert abs(got.loss_sum[0] - float(loss.cpu())) <= 1e-4 * got.loss_sum[0], "the routes' losses differ: nothing is timed"
    med = measure(f"(b) {K} x {N} x {C} logits", {"Scorer.add": lambda: scorer_b.add(logits, labels_b), "torch composition": torch_b}, args.calls)
    verdict("(b)", med, "Scorer.add", "torch composition", "no slower")

    # (c) model.evaluate over device-resident clips at .batch(32)
    n = args.clips
    base = Frontend().forward(torch.from_numpy(synth.clips_float32(64)).to(dev))
    specs = base.repeat((n + 63) // 64, 1, 1)[:n].contiguous()
    labels_c = torch.from_numpy(rng.integers(0, 3, n).astype(np.int64)).to(dev)
    emb, blob = tl.load_base_model("synthetic", max_batch=64)
    model = tl.TransferLearnedModel(emb, Head(1024, 18, 3, max_batch=64, params=glorot_uniform_params(1024, 18, 3, 1), device=dev), blob, "synthetic")

    def validate_loop():
        vstats, vseen = np.zeros(2), 0
        for s in range(0, n, 32):
            probs_c, lab = model.predict_device(specs[s:s + 32]), labels_c[s:s + 32]
            vstats[0] += float(-torch.log(torch.clamp(probs_c[torch.arange(len(lab)), lab], min=1e-7)).sum())
            vstats[1] += float((probs_c.argmax(1) == lab).sum())
            vseen += len(lab)
        return (vstats / max(vseen, 1)).tolist()

    ours, theirs = model.evaluate(specs, labels_c, batch_size=32), validate_loop()
    assert ours[1] == theirs[1] and abs(ours[0] - theirs[0]) <= 1e-5 * theirs[0], (ours, theirs)
    med = measure(f"(c) evaluate over {n} device-resident clips at batch_size 32 ({(n + 31) // 32} batches)",
                  {"model.evaluate": lambda: model.evaluate(specs, labels_c, batch_size=32), "_validate loop": validate_loop}, args.evaluate_calls, unit="ms")
    verdict("(c)", med, "model.evaluate", "_validate loop", "faster")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
