"""Audio that is not at 16 kHz: the device resampler (multilingual_kws_amd/resample.py) against what a caller had
before it.  One process, one MI355X.  Two comparisons:

  1. batch -- 1 024 one-second clips at 48 kHz, and one 20-minute recording at 44.1 kHz, from host memory to 16 kHz audio in device memory:
       (a) scipy.signal.resample_poly on the host (single-threaded), then the upload of the converted audio
       (b) the upload of the audio as it is, then Resampler.forward
     (median and the slowest of --reps runs each; the upload alone is timed beside them, since most of (b) is that upload)
     with the device time of (b)'s launch (events) and its achieved bytes per second, input plus output, beside the 6.29 TB/s copy figure
     of SURVEY.md section 8d.
  2. live -- LiveSessionGroup at S = 1, 16, 64 with 50 heads (the workload of tools/bench_live_group.py):
       (a) fed 16 kHz audio: the route of the parent commit
       (b) fed 48 kHz audio with input_rate=48000: three times the upload and one more launch at the head of the chain
     with the median and p99 tick of both, the device time of the added launch (events), host-to-device bytes per tick, and the largest
     measured S whose p99 stays under the 20 ms hop.

Before any time is printed the routes are compared: (b)'s batch output against the float32 restatement of the specification
(tests/util_resample.py) at sampled outputs, bit for bit; the live route (a) is fed Resampler.forward(centred=False) of (b)'s 48 kHz audio, so
the two must return the same rows with bit-equal scores, and do before they are timed.  Blocks alternate between the routes.  The one
condition that comes from the project is printed as a PASS / MISS line: at S = 64 the 48 kHz group's p99 tick is under the 20 ms hop, if
the 16 kHz group's is.

  python tools/bench_resample.py [--clips 1024] [--minutes 20] [--reps 9] [--seconds 10] [--heads 50] [--sizes 1,16,64] [--block 50]
                                 [--commit HASH] [--out profiles/resample.txt]"""
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

COPY_TBS = 6.29          # device-to-device copy, read plus write


def p99(ts):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, int(0.99 * len(ts)))]


def line(ts):
    ts = sorted(ts)
    return f"median {statistics.median(ts) * 1e3:9.3f} ms   p99 {p99(ts) * 1e3:9.3f} ms   (min {ts[0] * 1e3:.3f}, n={len(ts)})"


def few(ts):
    """The batch routes are timed a few times each: median and the slowest, not a percentile."""
    ts = sorted(ts)
    return f"median {statistics.median(ts) * 1e3:9.3f} ms   max {ts[-1] * 1e3:9.3f} ms   (min {ts[0] * 1e3:.3f}, n={len(ts)})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--minutes", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=9, help="timed repetitions of each batch route")
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--heads", type=int, default=50)
    ap.add_argument("--sizes", default="1,16,64")
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from scipy.signal import resample_poly
    from multilingual_kws_amd import synth
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa, transfer_learning as tl
    from multilingual_kws_amd.head import Head
    from multilingual_kws_amd.resample import Resampler
    from oracle import head_oracle as ho
    from tests.util_resample import polyphase
    assert torch.cuda.is_available(), "bench_resample.py measures on a GPU; there is nothing to report without one"
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

    say(f"# tools/bench_resample.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")

    # -- 1. batch ----------------------------------------------------------------------------------------------------------------------
    def device_ms(fn, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            fn()
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / n

    def batch_case(name, rate, x):
        """x: float32 [B, n] on the host."""
        rs = Resampler(rate)
        g, tab = rs.geometry, rs.taps()
        B, n = x.shape
        n_out = rs.out_samples(n)
        d_x = torch.from_numpy(x).to(dev)
        got = rs.forward(d_x)
        # the equality pass: sampled outputs of the first and the last row against the float32 restatement, bit for bit
        rng = np.random.default_rng(0)
        ns = np.unique(np.concatenate([np.arange(min(256, n_out)), np.arange(max(0, n_out - 256), n_out), rng.integers(0, n_out, 2048)]))
        for b in sorted({0, B - 1}):
            want = polyphase(x[b], tab, g["M"], g["half"], np.float32, ns=ns)
            mine = got[b][torch.from_numpy(ns).to(dev)].cpu().numpy()
            assert np.array_equal(mine.view(np.uint32), want.view(np.uint32)), f"{name}: Resampler.forward differs from its specification"
        host = resample_poly(x[:min(B, 2)], g["L"], g["M"], axis=1).astype(np.float32)
        gap = np.abs(host[:, 64:n_out - 64] - got[:host.shape[0], 64:n_out - 64].cpu().numpy()).max()
        out = torch.empty((B, n_out), dtype=torch.float32, device=dev)

        def route_a():
            y = resample_poly(x, g["L"], g["M"], axis=1).astype(np.float32)
            torch.from_numpy(y).to(dev)
            torch.cuda.synchronize()

        def route_b():
            rs.forward(torch.from_numpy(x).to(dev), out=out)
            torch.cuda.synchronize()
        def upload():
            torch.from_numpy(x).to(dev)
            torch.cuda.synchronize()
        series = dict(a=[], b=[], up=[])
        route_b()
        for r in range(args.reps):
            for tag, fn in ((("a", route_a), ("b", route_b), ("up", upload)) if r % 2 == 0 else (("up", upload), ("b", route_b), ("a", route_a))):
                t0 = time.perf_counter()
                fn()
                series[tag].append(time.perf_counter() - t0)
        ms = device_ms(lambda: rs.forward(d_x, out=out), 200)
        nbytes = 4 * B * (n + n_out)
        say(f"{name}: {B} x {n} samples at {rate} Hz -> {n_out} at 16 kHz (L = {g['L']}, M = {g['M']}, T = {g['T']}); (b) equals its specification bit for "
            f"bit at {len(ns)} sampled outputs of the first and last row; largest |(a) - (b)| away from the edges {gap:.2e} (white noise through two different filters: scipy's default cuts at Nyquist with a Kaiser 5.0 window)")
        say(f"  (a) scipy.signal.resample_poly on the host + upload:   {few(series['a'])}")
        say(f"  (b) upload + Resampler.forward:                        {few(series['b'])}")
        up = statistics.median(series["up"])
        say(f"      of which the upload of the {4 * B * n / 1e6:.0f} MB of unconverted audio from pageable host memory alone: {few(series['up'])} "
            f"= {4 * B * n / up / 1e9:.1f} GB/s (both routes upload from pageable memory; (a) uploads a third of it)")
        a, b = statistics.median(series["a"]), statistics.median(series["b"])
        say(f"  (b) / (a) = {b / a:.4f} ({a / b:.1f}x)")
        say(f"  (b) device time of the launch (events, 200 back to back): {ms:.4f} ms = {nbytes / ms / 1e9:.3f} TB/s of input plus output "
            f"({100 * nbytes / ms / 1e9 / COPY_TBS:.1f} % of the {COPY_TBS} TB/s copy figure)")
        rs.close()

    rng = np.random.default_rng(1)
    batch_case("clips", 48000, rng.uniform(-0.5, 0.5, (args.clips, 48000)).astype(np.float32))
    batch_case("recording", 44100, rng.uniform(-0.5, 0.5, (1, int(args.minutes * 60 * 44100))).astype(np.float32))

    # -- 2. live -----------------------------------------------------------------------------------------------------------------------
    K, thr, hop, clip, hop_ms, rate = args.heads, 0.9, 320, 16000, 20.0, 48000
    sizes = [int(v) for v in args.sizes.split(",") if v]
    keywords = [f"kw{k:02d}" for k in range(K)]
    params = []
    for k in range(K):
        p = ho.glorot_uniform_params(seed=2000 + k)
        p[-1] += 0.5 + 0.1 * (k % 7)
        params.append(p)
    ticks = args.seconds * 16000 // hop
    flags = sa.default_live_flags([thr])
    up, down = Resampler(16000, rate), Resampler(rate)
    in_hop = down.live_in_samples(hop)

    def streams(S):
        """Per slot the 48 kHz source (synthetic clips brought up to 48 kHz) and its causal conversion, which is what route (a) is fed."""
        src = np.stack([np.concatenate([synth.clips_int16(1, first_clip=(s * args.seconds + i) % 200)[0] for i in range(args.seconds)]) for s in range(S)])
        hi = up.forward(src.astype(np.float32) / 32768)
        return hi, down.forward(hi, centred=False)

    def walk(S, audio, groups, timed):
        found, series = dict(a=[], b=[]), dict(a=[], b=[])
        for g in groups.values():
            g.reset()

        def feed(tag, i):
            n = hop if tag == "a" else in_hop
            got = groups[tag].feed([a[i * n:(i + 1) * n] for a in audio[tag]])
            return [[s] + r for s in range(S) for r in got[s]]
        for b0 in range(0, ticks, args.block):
            for tag in ("a", "b") if (b0 // args.block) % 2 == 0 else ("b", "a"):
                for i in range(b0, min(ticks, b0 + args.block)):
                    t0 = time.perf_counter()
                    found[tag] += feed(tag, i)
                    if timed and (i + 1) * hop >= clip:
                        series[tag].append(time.perf_counter() - t0)
        return found, series

    def replay_ms(graph, n=200):
        return device_ms(graph.replay, n)

    say(f"# live: per slot a {args.seconds} s stream, {ticks} ticks, {K} heads, threshold {thr}; (a) LiveSessionGroup fed 16 kHz audio, (b) the same "
        f"group with input_rate={rate} fed the 48 kHz source; blocks of {args.block} ticks alternate between the routes")
    under, at64 = dict(a=0, b=0), {}
    more = [0.3, 0.5, 0.7, thr]
    for S in sizes:
        emb, blob = tl.load_base_model("synthetic", max_batch=S)
        models = [tl.TransferLearnedModel(emb, Head(max_batch=S, params=p, device=dev), blob, "synthetic") for p in params]
        hi, lo = streams(S)
        audio = dict(a=list(lo), b=list(hi))
        # the equality pass, at further thresholds so that there is something to compare: the same rows, scores bit for bit
        wide = dict(a=sa.LiveSessionGroup(models, streams=S, thresholds=more, flags=flags, keywords=keywords),
                    b=sa.LiveSessionGroup(models, streams=S, thresholds=more, flags=flags, keywords=keywords, input_rate=rate))
        found_wide, _ = walk(S, audio, wide, False)
        assert found_wide["a"] == found_wide["b"], f"S = {S}: the two routes disagree: nothing below would mean anything"
        for g in wide.values():
            g.close()
        groups = dict(a=sa.LiveSessionGroup(models, streams=S, thresholds=[thr], flags=flags, keywords=keywords),
                      b=sa.LiveSessionGroup(models, streams=S, thresholds=[thr], flags=flags, keywords=keywords, input_rate=rate))
        found, _ = walk(S, audio, groups, False)
        assert found["a"] == found["b"] and groups["b"].recaptures == 0
        found2, series = walk(S, audio, groups, True)
        assert found2 == found
        torch.cuda.synchronize()
        say(f"S = {S}: {len(found_wide['a'])} detections at {more}, {len(found['a'])} at {thr}: the same rows in both routes, scores bit for bit")
        say(f"  (a) LiveSessionGroup.feed at 16 kHz, per tick:          {line(series['a'])}")
        say(f"  (b) LiveSessionGroup.feed at 48 kHz, per tick:          {line(series['b'])}")
        ma, mb = statistics.median(series["a"]), statistics.median(series["b"])
        say(f"  (b) / (a) = {mb / ma:.4f} (median tick)")
        gb = groups["b"]
        scratch = gb.rstates.clone()
        added = device_ms(lambda: down.live_push_many(scratch, gb.raw, hop, active=None, out=gb.audio), 200)
        say(f"  device time per graph replay (events, 200 back to back):  (a) {replay_ms(groups['a'].graph):.4f} ms   (b) {replay_ms(gb.graph):.4f} ms;   "
            f"the added launch alone, all {S} slots active: {added:.4f} ms")
        say(f"  host-to-device bytes per tick (from shapes):              (a) {4 * (S * hop + S)}   (b) {4 * (S * in_hop + S)}")
        for tag in ("a", "b"):
            if p99(series[tag]) * 1e3 < hop_ms:
                under[tag] = max(under[tag], S)
        if S == 64:
            at64 = {tag: p99(series[tag]) * 1e3 for tag in ("a", "b")}
        for g in groups.values():
            g.close()
    say(f"largest measured S whose p99 tick stays under the {hop_ms:.0f} ms hop:  (a) {under['a']}   (b) {under['b']}   of {sizes}")
    ok = True
    if at64:
        if at64["a"] < hop_ms:
            ok = at64["b"] < hop_ms
            say(f"{'PASS' if ok else 'MISS'}: S = 64: the 48 kHz group's p99 tick {at64['b']:.3f} ms {'<' if ok else '>='} the {hop_ms:.0f} ms hop "
                f"(the 16 kHz group's: {at64['a']:.3f} ms)")
        else:
            say(f"S = 64: the 16 kHz group's own p99 tick {at64['a']:.3f} ms is not under the {hop_ms:.0f} ms hop: no condition on the 48 kHz group")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
