"""K (keyword, recording) pairs from wav files to per-threshold detections: one eval_stream_test after the other against one
eval_stream_tests pass.  One process, one MI355X.  K = 64 synthetic targets, a 20 s recording each (950 one-second windows), 64 distinct
heads on one synthetic embedding handle of 1024 windows per batch (the max_batch TransferLearnedModel.load and load_models_shared give a
model, so a recording is one ragged eager batch in route (a); with full batches inside a recording route (a) replays several serving
lanes whose workgroup shapes differ from the eager path's by round-off, and the equality below could not be asked for), 20 thresholds;
the heads are biased as in tests/test_detector_stream_gpu.py so that keywords fire.  Nothing is written (no destination paths) and nothing is stored between runs:
both routes read the wav files, window them, run the embedding and the heads, detect, and build the Python lists.

  (a) [eval_stream_test(st, live_model=m) for st, m in ...]: per target an embedding pass that ends in a ragged batch, every head call,
      an upload, a detector launch and a synchronising copy
  (b) eval_stream_tests(targets, live_models=models): the recordings' windows packed into full batches regardless of recording
      boundaries, each row under its own recording's head (mkws_head_group_forward_segments), ONE segmented detector launch and copy

(a) == (b) is asserted, dict for dict, before any time is printed.  Every shape is warmed up; every timed region ends in a device-to-host
copy; medians of --repeats runs (min and max beside them), the two routes alternated run by run.  The condition DESIGN.md section 18
states is printed as a PASS / MISS line: the median of (b) below the median of (a), (a) being measured in the same run.

  python tools/bench_stream_batch.py [--repeats 20] [--targets 64] [--seconds 20] [--commit HASH] [--out profiles/stream_batch.txt]"""
import argparse
import contextlib
import io
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--targets", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from multilingual_kws_amd import synth
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa, transfer_learning as tl
    from multilingual_kws_amd.head import Head
    from oracle import head_oracle as ho
    assert torch.cuda.is_available(), "bench_stream_batch.py measures on a GPU; there is nothing to report without one"
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
        return f"{statistics.median(ts) * 1e3:9.3f} ms  (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f}, n={len(ts)})"

    K, B = args.targets, 1024
    thresholds = [round(0.05 * i, 2) for i in range(1, 21)]
    emb, blob = tl.load_base_model("synthetic", max_batch=B)
    with tempfile.TemporaryDirectory() as tmp:
        targets, models = [], []
        for k in range(K):
            pcm = np.concatenate([synth.clips_int16(1, first_clip=(7 * k + i) % 200)[0] for i in range(args.seconds)])
            wav = os.path.join(tmp, f"kw{k:02d}.wav")
            with open(wav, "wb") as fh:
                fh.write(synth.wav_bytes(pcm))
            p = ho.glorot_uniform_params(seed=2000 + k)
            p[-1] += 0.5 + 0.1 * (k % 7)
            models.append(tl.TransferLearnedModel(emb, Head(max_batch=B, params=p, device=dev), blob, "synthetic"))
            flags = sa.StreamFlags(wav=wav, ground_truth=None, target_keyword=f"kw{k:02d}", detection_thresholds=thresholds)
            targets.append(sa.StreamTarget("xx", f"kw{k:02d}", "unused: live models", [flags]))
        W = len(sa.window_offsets(args.seconds * 16000, 16000, 320))

        def route_a():
            with contextlib.redirect_stdout(io.StringIO()):
                return [sa.eval_stream_test(st, live_model=m) for st, m in zip(targets, models)]

        def route_b():
            with contextlib.redirect_stdout(io.StringIO()):
                return sa.eval_stream_tests(targets, live_models=models)

        say(f"# tools/bench_stream_batch.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
        say(f"# {K} targets x {args.seconds} s ({W} windows each, {K * W} in all), {K} heads on one embedding handle of {B} windows per batch, "
            f"{len(thresholds)} thresholds; medians of {args.repeats} repeats, the two routes alternated")
        want, got = route_a(), route_b()
        assert got == want, "eval_stream_tests and the loop of eval_stream_test disagree: nothing below would mean anything"
        n_det = sum(len(found[0]) for r, st in zip(got, targets) for _, by_thr in r[st.target_word] for found in by_thr.values())
        for _ in range(2):                                               # every shape warmed up (graphs captured, tables built)
            route_a()
            route_b()
        torch.cuda.synchronize()
        series = dict(a=[], b=[])
        for _ in range(args.repeats):                                    # alternated: a, b, a, b, ...
            for name, fn in (("a", route_a), ("b", route_b)):
                t0 = time.perf_counter()
                fn()                                                     # ends in the device-to-host copy of its last detector call
                series[name].append(time.perf_counter() - t0)
        say(f"(a) loop of eval_stream_test, {K} targets ({n_det} detections over all thresholds):   {ms(series['a'])}")
        say(f"(b) eval_stream_tests, equal to (a):                                             {ms(series['b'])}")
        # where (b)'s time goes: the wav decode alone, and the device pass without the detector
        prep = []
        for _ in range(max(3, args.repeats // 4)):
            t0 = time.perf_counter()
            _, prepared = sa._prepare(targets, models, skip_done=True)
            t1 = time.perf_counter()
            sa._batch_inferences(prepared)
            prep.append((t1 - t0, time.perf_counter() - t1))
        say(f"(b) breakdown: reading and decoding {K} wav files                                  {ms([p[0] for p in prep])}")
        say(f"(b) breakdown: windowing, embedding, segmented heads, copy of {K * W * 12 / 1024:.0f} KB             {ms([p[1] for p in prep])}")
    med_a, med_b = statistics.median(series["a"]), statistics.median(series["b"])
    ok = med_b < med_a
    say(f"{'PASS' if ok else 'MISS'}: (b) = {med_b * 1e3:.3f} ms {'<' if ok else '>='} (a) = {med_a * 1e3:.3f} ms ({med_a / med_b:.2f}x)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
