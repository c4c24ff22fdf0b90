"""From WAV files to every keyword's classification ROC (roc_single_target's tprs / fprs at the reference's 101 thresholds): one model at a
time, as before, against one shared embedding pass with the counts taken on the device.  One process, one MI355X: 50 synthetic keyword
heads on one shared synthetic embedding, --targets one-second clips per keyword and ONE non-target pool of --pool clips that every
keyword is scored against (the reference's batch_transfer_learning_analysis.py samples about 24 000).  Seeded synthetic clips are
written to a temporary directory first.  Alternated run by run:

  (a) the route before: per keyword evaluate_files_single_target on its target clips and on the pool (each decodes, featurises and
      embeds its list: the pool 50 times), then roc_single_target on the two confidence vectors on the host
  (b) classification_curves: every distinct clip decoded, featurised and embedded once, all heads in one launch per batch, the counts on
      the device; the count kernel alone by device events

(a) == (b) is asserted, list for list, before any time is printed.  Both routes use the same files and the same embedding handle, end in
a device-to-host copy and are warmed up once; medians of --repeats runs (min and max beside them).

  python tools/bench_classification_roc.py [--pool 3000] [--targets 20] [--repeats 3] [--commit HASH] [--out profiles/classification_roc.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K = 50


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pool", type=int, default=3000, help="clips of the shared non-target pool")
    ap.add_argument("--targets", type=int, default=20, help="target clips per keyword")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from multilingual_kws_amd import _lib, synth
    from multilingual_kws_amd.embedding import input_data, transfer_learning as tl
    from multilingual_kws_amd.embedding.transfer_learning_analysis import default_thresholds, roc_single_target
    from multilingual_kws_amd.head import Head
    from multilingual_kws_amd.roc import pack_rows
    from oracle import head_oracle as ho
    assert torch.cuda.is_available(), "bench_classification_roc.py measures on a GPU; there is nothing to report without one"
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

    def ms(ts):
        return f"{statistics.median(ts) * 1e3:10.1f} ms  (min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f}, n={len(ts)})"

    B = 1024
    settings = input_data.standard_microspeech_model_settings(3)
    emb, blob = tl.load_base_model("synthetic", max_batch=B)
    models = []
    for k in range(K):
        p = 6 * ho.glorot_uniform_params(seed=3000 + k)          # scaled up: confidences spread over the thresholds
        models.append(tl.TransferLearnedModel(emb, Head(max_batch=B, params=p, device=dev), blob, "synthetic"))

    with tempfile.TemporaryDirectory() as tmp:
        n_files = args.pool + K * args.targets
        files = []
        for s in range(0, n_files, 256):
            for i, pcm in enumerate(synth.clips_int16(min(256, n_files - s), first_clip=s)):
                files.append(os.path.join(tmp, f"c{s + i:06d}.wav"))
                with open(files[-1], "wb") as fh:
                    fh.write(synth.wav_bytes(pcm))
        pool = files[:args.pool]
        targets = [files[args.pool + k * args.targets:args.pool + (k + 1) * args.targets] for k in range(K)]
        unknown = [pool] * K

        def route_a():
            out = []
            for k, m in enumerate(models):
                t = tl.evaluate_files_single_target(targets[k], 2, m, settings)[0]
                u = tl.evaluate_files_single_target(pool, 2, m, settings)[0]
                out.append(roc_single_target(t, u))
            return out

        def route_b():
            return tl.classification_curves(models, targets, unknown, settings)

        say(f"# tools/bench_classification_roc.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
        say(f"# {K} heads on one embedding handle (max_batch {B}); {args.targets} target clips per keyword, one pool of {args.pool} non-target clips, "
            f"{n_files} distinct files; 101 thresholds; medians of {args.repeats} repeats after one warm-up each, the two routes alternated")
        want, got = route_a(), route_b()                         # also the warm-up of every shape
        for k in range(K):
            assert got[k]["tprs"] == want[k][0] and got[k]["fprs"] == want[k][1], "the two routes disagree: nothing below would mean anything"
        say(f"# {len({tuple(c['fprs']) for c in got})} distinct false-positive curves among the {K} keywords")
        series = dict(a=[], b=[])
        for _ in range(args.repeats):                            # alternated: a, b, a, b, ...
            for name, fn in (("a", route_a), ("b", route_b)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                series[name].append(time.perf_counter() - t0)
        # the count kernel alone: device events around back-to-back launches on the predictions of all files
        preds = tl.evaluate_files_many(files, models, settings, as_device=True)
    index = {f: i for i, f in enumerate(files)}
    (p_rows, p_off), (n_rows, n_off) = (pack_rows([[index[f] for f in fs] for fs in lists], K, len(files), "rows") for lists in (targets, unknown))
    d_p, d_po, d_n, d_no = (torch.from_numpy(x).to(dev) for x in (p_rows, p_off, n_rows, n_off))
    d_thr = torch.from_numpy(default_thresholds()).to(dev)
    d_counts = torch.empty((K, 101, 2), dtype=torch.int32, device=dev)
    d_invalid = torch.empty(K, dtype=torch.int32, device=dev)
    L = _lib.lib()

    def launch():
        _lib.check(L.mkws_roc_count(preds.data_ptr(), K, len(files), 3, d_p.data_ptr(), d_po.data_ptr(), d_n.data_ptr(), d_no.data_ptr(), d_thr.data_ptr(),
                                    101, 0, 2, 1, d_counts.data_ptr(), d_invalid.data_ptr(), _lib.current_stream_ptr()))
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    kernel_us = e0.elapsed_time(e1) * 1e3 / reps
    counts = d_counts.cpu().numpy().tolist()
    for k in range(K):
        assert [c[0] / args.targets for c in counts[k]] == want[k][0] and [c[1] / args.pool for c in counts[k]] == want[k][1]
    a, b = statistics.median(series["a"]), statistics.median(series["b"])
    say(f"(a) evaluate_files_single_target per keyword + roc_single_target ({K * (args.pool + args.targets)} clips embedded): {ms(series['a'])}")
    say(f"(b) classification_curves, equal to (a) ({n_files} clips embedded):                                  {ms(series['b'])}")
    say(f"(b) count kernel alone, {K} heads x {args.targets + args.pool} entries x 101 thresholds (device events):            {kernel_us:10.1f} us")
    say(f"(a) / (b) = {a / b:.1f}x")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
