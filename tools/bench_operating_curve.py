"""From probabilities on the device to every keyword's operating curve (tpr_fpr's dict per threshold): the route through Python lists
against the route that stays on the device.  One process, one MI355X, the shape of `bench.py --config stream` (60 s synthetic stream,
2 950 one-second windows, batches of 256, 50 keyword heads on one shared embedding; heads biased as in tests/test_detector_stream_gpu.py
so that keywords fire).  Ground truth per keyword: that keyword's own fires at the middle threshold, every second one shifted by 700 ms,
plus decoys.  For 20 and for 101 thresholds (the reference's roc_sc resolution), alternated run by run:

  (a) the route before: detect_many (upload, detector launch, copy of the event buffer, the Python lists) followed by tpr_fpr once per
      (keyword, threshold); `to_copy` is detect_on_device alone, as tools/bench_detect.py reports it
  (b) operating_curves: score_on_device (one upload, detector + score launches, copy of 16 bytes per lane = `to_copy`) and the host
      arithmetic on three integers per lane; the score kernel alone by device events

(a) == (b) is asserted, dict for dict, before any time is printed.  Every timed region ends in a device-to-host copy; every shape is
warmed up first; medians of --repeats runs (min and max beside them).  The two conditions DESIGN.md section 15 states are printed as
PASS / MISS lines, both against the other route measured in the same run: (b) total below (a) total at 50 x 20, and (b) to_copy not
above (a) to_copy by more than the larger max - min spread of the two series.

  python tools/bench_operating_curve.py [--repeats 20] [--commit HASH] [--out profiles/operating_curve.txt]"""
import argparse
import contextlib
import io
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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from multilingual_kws_amd import _lib, synth
    from multilingual_kws_amd.detector import detect_on_device, event_capacity, pack_groundtruth, score_on_device
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa, input_data, transfer_learning as tl
    from multilingual_kws_amd.embedding.tpr_fpr import tpr_fpr
    from multilingual_kws_amd.head import Head
    from oracle import head_oracle as ho
    assert torch.cuda.is_available(), "bench_operating_curve.py measures on a GPU; there is nothing to report without one"
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

    B = 256
    settings = input_data.standard_microspeech_model_settings(3)
    pcm = np.concatenate([synth.clips_int16(1, first_clip=i)[0] for i in range(60)])
    audio = pcm.astype(np.float32) / np.float32(32768.0)
    emb, blob = tl.load_base_model("synthetic", max_batch=B)
    keywords = [f"kw{k:02d}" for k in range(50)]
    heads = []
    for k in range(50):
        p = ho.glorot_uniform_params(seed=2000 + k)
        p[-1] += 0.5 + 0.1 * (k % 7)
        heads.append(Head(max_batch=B, params=p, device=dev))
    flags = sa.StreamFlags(wav="stream.wav", ground_truth=None, target_keyword="kw", detection_thresholds=[])
    offsets = sa.window_offsets(audio.shape[0], 16000, 320)
    t_ms = [int(o * 1000 / 16000) for o in offsets]
    W = len(offsets)
    duration_s = audio.shape[0] / 16000
    probs = sa.serve_spectrograms(emb, heads, sa.stream_spectrograms(settings, torch.from_numpy(audio).to(dev), 16000, 320), B)
    torch.cuda.synchronize()

    say(f"# tools/bench_operating_curve.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
    say(f"# stream: 60 s, {W} windows, 50 heads; detector: average 100 ms, suppression 500 ms, minimum count 4; tolerance {flags.time_tolerance_ms} ms; "
        f"medians of {args.repeats} repeats, the two routes alternated")

    # ground truth: each keyword's own fires at the middle threshold, every second one 700 ms late, and decoys nothing need fire near
    rng = np.random.default_rng(5)
    fired = sa.detect_many(probs, flags, [0.5], 16000, data_samples=audio.shape[0], keywords=keywords)
    gt = {}
    for n, kw in enumerate(keywords):
        own = [float(t) + 700.0 * (i % 2) for i, (_, t) in enumerate(fired[n][0.5][0])]
        gt[kw] = sorted(own + [float(x) for x in rng.integers(0, 60000, 4)])
    n_gt = sum(len(g) for g in gt.values())

    def route_a(thresholds):
        many = sa.detect_many(probs, flags, thresholds, 16000, data_samples=audio.shape[0], keywords=keywords)
        with contextlib.redirect_stdout(io.StringIO()):
            return [[tpr_fpr(kw, thr, many[n][thr][0], gt[kw], duration_s, flags.time_tolerance_ms) for thr in thresholds] for n, kw in enumerate(keywords)]

    def route_b(thresholds):
        with contextlib.redirect_stdout(io.StringIO()):
            return sa.operating_curves(probs, flags, thresholds, gt, keywords=keywords, data_samples=audio.shape[0])

    gt_lists = [gt[kw] for kw in keywords]
    res = {}
    for T in (20, 101):
        thresholds = [round(0.05 * i, 2) for i in range(1, 21)] if T == 20 else [round(0.01 * i, 2) for i in range(101)]
        want, got = route_a(thresholds), route_b(thresholds)
        assert got == want, "operating_curves and detect_many + tpr_fpr disagree: nothing below would mean anything"
        n_det = sum(d["true_positives"] + d["false_positives"] for c in got for d in c)
        series = dict(a_total=[], b_total=[], a_copy=[], b_copy=[])
        calls = dict(a_total=lambda: route_a(thresholds), b_total=lambda: route_b(thresholds),
                     a_copy=lambda: detect_on_device(probs, t_ms, thresholds, 100, 500, 4, fired_only=True),
                     b_copy=lambda: score_on_device(probs, t_ms, thresholds, gt_lists, flags.time_tolerance_ms, 100, 500, 4))
        for fn in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.repeats):                                 # alternated: a, b, a, b, ...
            for name, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                series[name].append(time.perf_counter() - t0)
        # the score kernel alone: device events around back-to-back launches on the detector's own output
        cap = event_capacity(t_ms, 500, fired_only=True)
        d_times = torch.tensor(t_ms, dtype=torch.int64, device=dev)
        d_thr = torch.tensor(thresholds, dtype=torch.float64, device=dev)
        d_events = torch.empty(50 * T * cap * 2, dtype=torch.int64, device=dev)
        d_counts = torch.empty(50 * T, dtype=torch.int32, device=dev)
        d_tally = torch.empty((50, T, 4), dtype=torch.int32, device=dev)
        values, offs = pack_groundtruth(gt_lists, 50)
        d_gt, d_off = torch.from_numpy(values).to(dev), torch.from_numpy(offs).to(dev)
        L = _lib.lib()
        _lib.check(L.mkws_detect_stream(probs.data_ptr(), 0, 50, W, 3, 2, d_times.data_ptr(), d_thr.data_ptr(), T, 100.0, 500.0, 4, 1,
                                        d_events.data_ptr(), cap, d_counts.data_ptr(), None, None, _lib.current_stream_ptr()))

        def launch():
            _lib.check(L.mkws_detect_score(d_events.data_ptr(), d_counts.data_ptr(), 50, T, cap, d_times.data_ptr(), W, d_gt.data_ptr(), d_off.data_ptr(),
                                           float(flags.time_tolerance_ms), d_tally.data_ptr(), _lib.current_stream_ptr()))
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = max(20, args.repeats)
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        kernel_us = e0.elapsed_time(e1) * 1e3 / reps
        assert np.array_equal(d_tally.cpu().numpy()[:, :, :3], score_on_device(probs, t_ms, thresholds, gt_lists, flags.time_tolerance_ms, 100, 500, 4))
        res[T] = dict(series=series, kernel_us=kernel_us)
        say(f"(a) 50 x {T:3d} thr, detect_on_device to_copy (upload, launch, {50 * T * cap * 16 / 1024:.0f} KB copy):      {ms(series['a_copy'])}")
        say(f"(a) 50 x {T:3d} thr, total: detect_many + tpr_fpr per lane ({n_det} det., {n_gt} gt):  {ms(series['a_total'])}")
        say(f"(b) 50 x {T:3d} thr, score_on_device to_copy (upload, 2 launches, {50 * T * 16 / 1024:.0f} KB copy):   {ms(series['b_copy'])}")
        say(f"(b) 50 x {T:3d} thr, total: operating_curves, equal to (a):                       {ms(series['b_total'])}")
        say(f"(b) 50 x {T:3d} thr, score kernel alone (device events):                        {kernel_us:9.1f} us")

    s20 = res[20]["series"]
    med = {k: statistics.median(v) for k, v in s20.items()}
    ok1 = med["b_total"] < med["a_total"]
    say(f"{'PASS' if ok1 else 'MISS'}: (b) total at 50 x 20 = {med['b_total'] * 1e3:.3f} ms {'<' if ok1 else '>='} (a) total = {med['a_total'] * 1e3:.3f} ms "
        f"({med['a_total'] / med['b_total']:.1f}x; at 50 x 101: {statistics.median(res[101]['series']['a_total']) / statistics.median(res[101]['series']['b_total']):.1f}x)")
    spread = max(max(s20["a_copy"]) - min(s20["a_copy"]), max(s20["b_copy"]) - min(s20["b_copy"]))
    ok2 = med["b_copy"] <= med["a_copy"] + spread
    say(f"{'PASS' if ok2 else 'MISS'}: (b) to_copy at 50 x 20 = {med['b_copy'] * 1e3:.3f} ms {'<=' if ok2 else '>'} (a) to_copy = {med['a_copy'] * 1e3:.3f} ms "
        f"+ spread {spread * 1e3:.3f} ms (score kernel {res[20]['kernel_us']:.0f} us)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok1 and ok2 else 1


if __name__ == "__main__":
    sys.exit(main())
