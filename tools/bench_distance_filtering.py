"""From WAV files to every keyword's outlier ranking (distance_filtering.cluster_and_sort: k-means on the embeddings of n_train clips, the
remaining clips sorted by the L2 distance to their nearest centre): one keyword at a time with sklearn on the host, as before, against
cluster_and_sort_many with the clustering and the distances on the device.  One process, one MI355X: --keywords synthetic keywords x
--clips one-second clips on one synthetic embedding handle, (n_train, n_clusters) = (50, 5) as in the reference's notebook.  Seeded
synthetic clips are written to a temporary directory first.  Alternated run by run:

  (a) the route before: per keyword cluster_and_sort (embed the train clips, copy them to the host, sklearn KMeans.fit, embed the eval
      clips, copy every vector to the host, norms / minimum / sort in NumPy)
  (b) cluster_and_sort_many: the train clips of all keywords embedded and kept on the device, one mkws_kmeans_fit, mkws_kmeans_nearest on
      every batch of eval embeddings, 8 bytes per eval clip copied back; the two kernels alone by device events

The train_clips lists of the two routes are asserted equal before any time is printed.  The sorted lists are compared and the number of
keywords whose order differs is printed, not asserted: sklearn clusters in float32, (b) in float64, and near-ties may sort differently.
Both routes use the same files and the same embedding handle, end in a device-to-host copy and are warmed up once; medians of --repeats
runs (min and max beside them).

  python tools/bench_distance_filtering.py [--keywords 64] [--clips 150] [--repeats 3] [--commit HASH] [--out profiles/distance_filtering.txt]"""
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

N_TRAIN, N_CLUSTERS, SEED = 50, 5, 123


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keywords", type=int, default=64)
    ap.add_argument("--clips", type=int, default=150, help="clips per keyword")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from multilingual_kws_amd import _lib, kmeans, synth
    from multilingual_kws_amd.embedding import distance_filtering as dfl
    assert torch.cuda.is_available(), "bench_distance_filtering.py measures on a GPU; there is nothing to report without one"
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

    K = args.keywords
    emb = dfl.embedding_model("synthetic", max_batch=1024)
    with tempfile.TemporaryDirectory() as tmp:
        n_files = K * args.clips
        files = []
        for s in range(0, n_files, 256):
            for i, pcm in enumerate(synth.clips_int16(min(256, n_files - s), first_clip=s)):
                files.append(os.path.join(tmp, f"c{s + i:06d}.wav"))
                with open(files[-1], "wb") as fh:
                    fh.write(synth.wav_bytes(pcm))
        keywords = [np.array(files[k * args.clips:(k + 1) * args.clips]) for k in range(K)]

        def route_a():
            return [dfl.cluster_and_sort(kw, emb, seed=SEED, n_train=N_TRAIN, n_clusters=N_CLUSTERS) for kw in keywords]

        def route_b():
            return dfl.cluster_and_sort_many(keywords, emb, seed=SEED, n_train=N_TRAIN, n_clusters=N_CLUSTERS)

        say(f"# tools/bench_distance_filtering.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
        say(f"# {K} keywords x {args.clips} clips on one embedding handle (max_batch 1024); n_train {N_TRAIN}, n_clusters {N_CLUSTERS}, seed {SEED}; "
            f"medians of {args.repeats} repeats after one warm-up each, the two routes alternated")
        want, got = route_a(), route_b()                         # also the warm-up of every shape
        for k in range(K):
            assert list(got[k]["train_clips"]) == list(want[k]["train_clips"]), "the two routes split differently: nothing below would mean anything"
        differ = sum(list(got[k]["sorted_clips"]) != list(want[k]["sorted_clips"]) for k in range(K))
        say(f"# keywords whose sorted order differs between the routes: {differ} of {K}; sklearn fallbacks in (b): {sum(r['fallback'] for r in got)}")
        series = dict(a=[], b=[])
        for _ in range(args.repeats):                            # alternated: a, b, a, b, ...
            for name, fn in (("a", route_a), ("b", route_b)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                series[name].append(time.perf_counter() - t0)
        # the two kernels alone: device events around back-to-back launches on the embeddings of all files
        vec = torch.from_numpy(dfl.embed_files(files, emb)).to(dev)
    train_rows = np.concatenate([np.arange(k * args.clips, k * args.clips + N_TRAIN) for k in range(K)])
    eval_rows = np.concatenate([np.arange(k * args.clips + N_TRAIN, (k + 1) * args.clips) for k in range(K)])
    d_train, d_eval = vec[torch.from_numpy(train_rows).to(dev)].contiguous(), vec[torch.from_numpy(eval_rows).to(dev)].contiguous()
    d_group = torch.from_numpy(np.repeat(np.arange(K, dtype=np.int32), args.clips - N_TRAIN)).to(dev)
    T = kmeans.n_local_trials(N_CLUSTERS)
    d_off = torch.from_numpy((np.arange(K + 1) * N_TRAIN).astype(np.int32)).to(dev)
    d_draws = torch.from_numpy(np.stack([kmeans.kmeans_draws(SEED, N_CLUSTERS)] * K)).to(dev)
    d_centers = torch.empty((K, N_CLUSTERS, 1024), dtype=torch.float32, device=dev)
    d_labels = torch.empty(K * N_TRAIN, dtype=torch.int32, device=dev)
    d_info = torch.empty((K, 4), dtype=torch.int32, device=dev)
    out = (torch.empty(len(eval_rows), dtype=torch.float32, device=dev), torch.empty(len(eval_rows), dtype=torch.int32, device=dev),
           torch.empty(1, dtype=torch.int32, device=dev))
    L = _lib.lib()

    def fit():
        _lib.check(L.mkws_kmeans_fit(d_train.data_ptr(), 1024, d_off.data_ptr(), K, N_CLUSTERS, d_draws.data_ptr(), T, 300, 1e-4, d_centers.data_ptr(),
                                     None, d_labels.data_ptr(), None, d_info.data_ptr(), _lib.current_stream_ptr()))

    def nearest():
        kmeans.nearest_on_device(d_eval, d_group, d_centers, out=out)

    def device_us(launch, reps=50):
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    fit_us, nearest_us = device_us(fit), device_us(nearest)
    info = d_info.cpu().numpy()
    a, b = statistics.median(series["a"]), statistics.median(series["b"])
    say(f"(a) cluster_and_sort per keyword (sklearn KMeans on the host, every vector copied back): {ms(series['a'])}")
    say(f"(b) cluster_and_sort_many (one fit launch, 8 bytes per eval clip copied back):          {ms(series['b'])}")
    say(f"(b) mkws_kmeans_fit alone, {K} groups x {N_TRAIN} x 1024, k = {N_CLUSTERS}, iterations {int(info[:, 1].min())}..{int(info[:, 1].max())} (device events): {fit_us:10.1f} us")
    say(f"(b) mkws_kmeans_nearest alone, {len(eval_rows)} rows x {N_CLUSTERS} centres x 1024 (device events):              {nearest_us:10.1f} us")
    say(f"(a) / (b) = {a / b:.1f}x")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
