"""A live stream hop by hop, from 20 ms of new audio to the detections on the host: the window loop a caller builds from StreamingSession
against LiveSession.  One process, one MI355X.  The README's streaming configuration: a 60 s synthetic stream, 50 keyword heads (seeds
2000 .. 2049, their target class biased as in tools/bench_stream_batch.py) on one synthetic embedding handle of one window, one
threshold 0.9 -- which these synthetic heads do not reach on this stream: the timed configuration reports no detection.

  (a) baseline, from code unchanged by this change: a host ring of the last second, StreamingSession.infer(ring) (64 000 B up, all 49
      frames of the window again), .cpu() of the [50, 1, 3] probabilities, 50 SingleTargetRecognizeCommands stepped in Python
  (b) LiveSession.feed(hop): 1 280 B up, one graph replay (frontend push of the one new frame, embedding, heads, detector step), one
      copy of counts and events back

(a) == (b), detection for detection with bit-equal scores, is asserted at the timed size before any time is printed.  At the timed
threshold that compares two empty lists, so the assertion that carries weight is the second pass with --check-thresholds beside 0.9
(several hundred detections).  Both routes walk
the same stream; blocks of --block pushes alternate between them after a warm-up pass; every timed push ends with its events on the host.
Only pushes that complete a window are timed (the first second fills the window).  Reported: median and p99 wall time per push, device
time per graph replay (from events), host-to-device bytes per push (from shapes).  The condition DESIGN.md section 19 states is printed
as a PASS / MISS line: the median of (b) not above the median of (a).

  python tools/bench_live.py [--seconds 60] [--heads 50] [--block 200] [--check-thresholds 0.3,0.5,0.7] [--commit HASH] [--out profiles/live_session.txt]"""
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
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--heads", type=int, default=50)
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--check-thresholds", default="0.3,0.5,0.7", help="further thresholds of the equality pass (not timed)")
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from multilingual_kws_amd import synth
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa, input_data, transfer_learning as tl
    from multilingual_kws_amd.embedding.single_target_recognize_commands import RecognizeResult, SingleTargetRecognizeCommands
    from multilingual_kws_amd.head import Head
    from oracle import head_oracle as ho
    assert torch.cuda.is_available(), "bench_live.py measures on a GPU; there is nothing to report without one"
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

    K, thr, hop, clip = args.heads, 0.9, 320, 16000
    ms = input_data.standard_microspeech_model_settings(3)
    emb, blob = tl.load_base_model("synthetic", max_batch=1)
    models, keywords = [], [f"kw{k:02d}" for k in range(K)]
    for k in range(K):
        p = ho.glorot_uniform_params(seed=2000 + k)
        p[-1] += 0.5 + 0.1 * (k % 7)
        models.append(tl.TransferLearnedModel(emb, Head(max_batch=1, params=p, device=dev), blob, "synthetic"))
    pcm = np.concatenate([synth.clips_int16(1, first_clip=i % 200)[0] for i in range(args.seconds)])
    audio = pcm.astype(np.float32) / 32768
    hops = audio.size // hop
    flags = sa.default_live_flags([thr])
    window_loop = sa.StreamingSession(models, ms, batch=1)
    live = sa.LiveSession(models, [thr], flags=flags, keywords=keywords)

    class Baseline:
        """What a caller of StreamingSession writes to get detections: the audio ring and one detector per keyword and threshold on the host."""

        def __init__(self, thresholds):
            self.ring, self.n = np.zeros(clip, np.float32), 0
            self.lanes = [[(t, SingleTargetRecognizeCommands(flags.labels()[:2] + [kw], flags.average_window_duration_ms, t, flags.suppression_ms,
                                                             flags.minimum_count, 2)) for t in thresholds] for kw in keywords]
            self.el = RecognizeResult()

        def feed(self, chunk):
            self.ring[:-hop] = self.ring[hop:]
            self.ring[-hop:] = chunk
            self.n += hop
            if self.n < clip:
                return []
            t_ms = int((self.n - clip) * 1000 / 16000)
            probs = window_loop.infer(self.ring).cpu().numpy()
            out, el = [], self.el
            for k, lanes in enumerate(self.lanes):
                for t, rc in lanes:
                    rc.process_latest_result(probs[k, 0], t_ms, el)
                    if el.is_new_command and el.found_command != "_silence_":
                        out.append([el.found_command, t_ms, el.score, t])
            return out

    def walk(timed, session, thresholds):
        base, found, series = Baseline(thresholds), dict(a=[], b=[]), dict(a=[], b=[])
        session.reset()
        routes = (("a", base.feed), ("b", session.feed))
        for b0 in range(0, hops, args.block):
            order = routes if (b0 // args.block) % 2 == 0 else routes[::-1]
            for name, feed in order:
                for i in range(b0, min(hops, b0 + args.block)):
                    chunk = audio[i * hop:(i + 1) * hop]
                    t0 = time.perf_counter()
                    found[name] += feed(chunk)
                    if timed and (i + 1) * hop >= clip:
                        series[name].append(time.perf_counter() - t0)
        return found, series

    say(f"# tools/bench_live.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
    say(f"# {args.seconds} s stream, {hops} pushes of {hop} samples, {K} heads on one embedding handle of one window, threshold {thr}; "
        f"blocks of {args.block} pushes alternate between the two routes")
    found, _ = walk(False, live, [thr])                              # warm-up pass = the equality check at the timed size
    assert found["b"] == found["a"], "LiveSession and the StreamingSession loop disagree: nothing below would mean anything"
    assert live.windows_seen == 1 + (hops * hop - clip) // hop and live.recaptures == 0
    more = sorted(set(float(t) for t in args.check_thresholds.split(",") if t) | {thr})
    wide = sa.LiveSession(models, more, flags=flags, keywords=keywords)
    found_wide, _ = walk(False, wide, more)
    assert found_wide["b"] == found_wide["a"], "LiveSession and the StreamingSession loop disagree at the further thresholds"
    wide.close()
    found2, series = walk(True, live, [thr])
    assert found2 == found
    torch.cuda.synchronize()

    def line(ts):
        ts = sorted(ts)
        return f"median {statistics.median(ts) * 1e3:7.3f} ms   p99 {ts[min(len(ts) - 1, int(0.99 * len(ts)))] * 1e3:7.3f} ms   (min {ts[0] * 1e3:.3f}, n={len(ts)})"
    say(f"{len(found['a'])} detections over the {K} keywords at {thr}, {len(found_wide['a'])} at {more}: equal in both routes, scores bit for bit")
    say(f"(a) ring + StreamingSession.infer + .cpu() + {K} host detectors, per push:   {line(series['a'])}")
    say(f"(b) LiveSession.feed, per push:                                          {line(series['b'])}")

    def replay_ms(graph, n=200):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(20):
            graph.replay()
        start.record()
        for _ in range(n):
            graph.replay()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / n
    say(f"device time per graph replay (events, 200 back to back):  (a) {replay_ms(window_loop.graph):.4f} ms   (b) {replay_ms(live.graph):.4f} ms")
    say(f"host-to-device bytes per push (from shapes):              (a) {4 * clip}   (b) {4 * live.push_samples}")
    med_a, med_b = statistics.median(series["a"]), statistics.median(series["b"])
    ok = med_b <= med_a
    say(f"{'PASS' if ok else 'MISS'}: (b) = {med_b * 1e3:.3f} ms {'<=' if ok else '>'} (a) = {med_a * 1e3:.3f} ms ({med_a / med_b:.2f}x)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
