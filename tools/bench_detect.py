"""Where the stream row's time goes once the detector runs on the device.  One process, one MI355X, the shape of `bench.py --config stream`
(60 s synthetic stream, 2 950 one-second windows, batches of 256, 50 keyword heads on one shared embedding; heads biased as in
tests/test_detector_stream_gpu.py so that keywords fire):

  (a) the host detector as it ran before: detect() looped over the 50 keywords, for 1 threshold and for 20
  (b) the device detector stage, same two cases: detect_on_device (upload of times and thresholds, launch, the one device-to-host
      copy = `to_copy`) and detect_many (the same plus building the Python lists = `total`); the kernel alone by device events
  (c) serve_spectrograms for the same stream, fenced, as `bench.py --config stream` times it
  (d) run.inference, wav -> detections dict, warm: with the host detector (detect_many replaced by a detect() loop over the host
      copies, which is what multi_keyword_detections did before) and with the device detector, alternated

Every timed region ends in torch.cuda.synchronize() or in a device-to-host copy; every shape is warmed up first; medians of --repeats
runs (min and max beside them).  The two conditions the device detector is held to are printed as PASS / MISS lines:
(b) total at 50 x 1 takes less time than (c), and (b) to_copy at 20 thresholds takes less than twice (b) to_copy at one.

  python tools/bench_detect.py [--repeats 20] [--host-repeats-20 5] [--commit HASH] [--out profiles/detector_e2e.txt]"""
import argparse
import contextlib
import io
import os
import shutil
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
    ap.add_argument("--host-repeats-20", type=int, default=5, help="repeats of the 50 x 20 host loop (a pure host loop of several seconds per run)")
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from multilingual_kws_amd import _lib, run, synth
    from multilingual_kws_amd.detector import detect_on_device, event_capacity
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa, input_data, transfer_learning as tl
    from multilingual_kws_amd.head import Head
    from oracle import head_oracle as ho
    assert torch.cuda.is_available(), "bench_detect.py measures on a GPU; there is nothing to report without one"
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

    def timed(fn, repeats, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    def ms(ts):
        return f"{statistics.median(ts) * 1e3:9.3f} ms  (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f}, n={len(ts)})"

    B, THR = 256, 0.5
    thresholds20 = [round(0.05 * i, 2) for i in range(1, 21)]
    settings = input_data.standard_microspeech_model_settings(3)
    pcm = np.concatenate([synth.clips_int16(1, first_clip=i)[0] for i in range(60)])
    tmp = tempfile.mkdtemp(prefix="bench_detect_")
    wav = os.path.join(tmp, "stream.wav")
    with open(wav, "wb") as fh:
        fh.write(synth.wav_bytes(pcm))
    audio = pcm.astype(np.float32) / np.float32(32768.0)
    emb, blob = tl.load_base_model("synthetic", max_batch=B)
    keywords = [f"kw{k:02d}" for k in range(50)]
    models = []
    for k in range(50):
        p = ho.glorot_uniform_params(seed=2000 + k)
        p[-1] += 0.5 + 0.1 * (k % 7)
        models.append(tl.TransferLearnedModel(emb, Head(max_batch=B, params=p, device=dev), blob, "synthetic"))
    heads = [m.head for m in models]
    stream = torch.from_numpy(audio).to(dev)
    flags = sa.StreamFlags(wav=wav, ground_truth=None, target_keyword="kw", detection_thresholds=[THR])
    offsets = sa.window_offsets(audio.shape[0], 16000, 320)
    t_ms = [int(o * 1000 / 16000) for o in offsets]
    W = len(offsets)

    say(f"# tools/bench_detect.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
    say(f"# stream: 60 s, {W} windows, batch {B}, 50 heads; detector: average 100 ms, suppression 500 ms, minimum count 4; medians of {args.repeats} repeats")

    # (c) the device pass the detector follows
    def serve():
        out = sa.serve_spectrograms(emb, heads, sa.stream_spectrograms(settings, stream, 16000, 320), B)
        torch.cuda.synchronize()
        return out
    t_c = timed(serve, args.repeats, warm=4)
    probs = serve()                                                   # CUDA [50, W, 3]: what the detector stage reads
    host = probs.cpu().numpy()
    say(f"(c) serve_spectrograms, {W} windows x 50 heads, fenced:            {ms(t_c)}")

    # (a) the host detector
    def host_loop(thresholds):
        return [{t: sa.detect(host[n], flags, t, 16000, data_samples=audio.shape[0]) for t in thresholds} for n in range(50)]
    t_a1 = timed(lambda: host_loop([THR]), args.repeats, warm=1)
    t_a20 = timed(lambda: host_loop(thresholds20), args.host_repeats_20, warm=0)
    say(f"(a) host detect() x 50 keywords x  1 threshold:                     {ms(t_a1)}")
    say(f"(a) host detect() x 50 keywords x 20 thresholds:                    {ms(t_a20)}")

    # (b) the device detector stage
    res = {}
    for name, thresholds in (("1", [THR]), ("20", thresholds20)):
        want = host_loop(thresholds)
        got = sa.detect_many(probs, flags, thresholds, 16000, data_samples=audio.shape[0])
        assert got == want, "the device detector and detect() disagree: nothing below would mean anything"
        n_det = sum(len(g[t][0]) for g in got for t in thresholds)
        t_copy = timed(lambda: detect_on_device(probs, t_ms, thresholds, 100, 500, 4, fired_only=True), args.repeats)
        t_total = timed(lambda: sa.detect_many(probs, flags, thresholds, 16000, data_samples=audio.shape[0]), args.repeats)
        # the kernel alone: device events around back-to-back launches into preallocated buffers
        T = len(thresholds)
        cap = event_capacity(t_ms, 500, fired_only=True)
        d_times = torch.tensor(t_ms, dtype=torch.int64, device=dev)
        d_thr = torch.tensor(thresholds, dtype=torch.float64, device=dev)
        d_events = torch.empty(50 * T * cap * 2, dtype=torch.int64, device=dev)
        d_counts = torch.empty(50 * T, dtype=torch.int32, device=dev)
        L = _lib.lib()

        def launch():
            _lib.check(L.mkws_detect_stream(probs.data_ptr(), 0, 50, W, 3, 2, d_times.data_ptr(), d_thr.data_ptr(), T, 100.0, 500.0, 4, 1,
                                            d_events.data_ptr(), cap, d_counts.data_ptr(), None, None, _lib.current_stream_ptr()))
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
        res[name] = dict(copy=statistics.median(t_copy), total=statistics.median(t_total), kernel_us=kernel_us)
        pad = " " if name == "1" else ""
        say(f"(b) device detector, 50 x {pad}{name} thr, to_copy (upload, launch, copy):   {ms(t_copy)}")
        say(f"(b) device detector, 50 x {pad}{name} thr, total (+ Python lists, {n_det:5d} det.): {ms(t_total)}")
        say(f"(b) device detector, 50 x {pad}{name} thr, kernel alone (device events):     {kernel_us:9.1f} us  event buffer {50 * T * cap * 16 / 1024:.0f} KB (capacity {cap} per lane)")

    # (d) run.inference wall clock, warm, host detector vs device detector, alternated
    device_detect_many = sa.detect_many

    def host_detect_many(inferences, flags_, thresholds, sample_rate=16000, data_samples=None, keywords=None):
        import dataclasses
        rows = inferences.cpu().numpy() if torch.is_tensor(inferences) else inferences
        return [{t: sa.detect(rows[n], dataclasses.replace(flags_, target_keyword=keywords[n]), t, sample_rate, data_samples) for t in thresholds}
                for n in range(len(keywords))]

    def inference(which):
        sa.detect_many = which
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                return run.inference(keywords, models, wav, detection_threshold=THR)
        finally:
            sa.detect_many = device_detect_many
    before, after = inference(host_detect_many), inference(device_detect_many)
    assert before == after and len(after["detections"]) > 10, "run.inference differs between the host and the device detector"
    t_before, t_after = [], []
    for _ in range(args.repeats):
        for which, ts in ((host_detect_many, t_before), (device_detect_many, t_after)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inference(which)
            ts.append(time.perf_counter() - t0)
    say(f"(d) run.inference wav -> dict, host detector (before):             {ms(t_before)}")
    say(f"(d) run.inference wav -> dict, device detector (after):            {ms(t_after)}   {len(after['detections'])} detections, equal to (before)")

    c = statistics.median(t_c)
    a1, a20 = statistics.median(t_a1), statistics.median(t_a20)
    say(f"speed-up of the detector stage over (a): {a1 / res['1']['total']:.0f}x at 1 threshold, {a20 / res['20']['total']:.0f}x at 20; "
        f"run.inference {statistics.median(t_before) / statistics.median(t_after):.1f}x")
    ok1 = res["1"]["total"] < c
    say(f"{'PASS' if ok1 else 'MISS'}: (b) total at 50 x 1 = {res['1']['total'] * 1e3:.3f} ms {'<' if ok1 else '>='} (c) = {c * 1e3:.3f} ms "
        f"(kernel {res['1']['kernel_us']:.0f} us, upload + launch + copy {res['1']['copy'] * 1e3:.3f} ms, lists {(res['1']['total'] - res['1']['copy']) * 1e3:.3f} ms)")
    ok2 = res["20"]["copy"] < 2 * res["1"]["copy"]
    say(f"{'PASS' if ok2 else 'MISS'}: (b) to_copy at 20 thresholds = {res['20']['copy'] * 1e3:.3f} ms {'<' if ok2 else '>='} 2 x to_copy at 1 = {2 * res['1']['copy'] * 1e3:.3f} ms "
        f"(kernel {res['20']['kernel_us']:.0f} us vs {res['1']['kernel_us']:.0f} us)")
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok1 and ok2 else 1


if __name__ == "__main__":
    sys.exit(main())
