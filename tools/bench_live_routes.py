"""S live streams whose slots each spot keywords of their own, from 20 ms of new audio each to their detections on the host: one
LiveSessionGroup that serves every keyword to every slot against one LiveRoutedGroup with a route per (slot, keyword of that slot).  One
process, one MI355X.  The workload of tools/bench_live_group.py per slot: a 10 s synthetic stream (distinct clips per slot), 320-sample
pushes, one threshold 0.9 (which these synthetic heads do not reach: the timed configuration reports no detection); slot s owns the
--per-slot heads s * per .. s * per + per - 1 of S * per synthetic heads (seeds 2000 ..., their target class biased as there).

  (a) what a caller of the parent commit writes: one LiveSessionGroup with all S * per heads shared -- every head on every slot's rows,
      every (slot, head) lane stepped and downloaded -- and the host discarding the events of keywords a slot does not own
  (b) one LiveRoutedGroup with S * per routes: heads and detectors do work per route, the download is one count per route

Both run on ONE embedding handle of S windows and the same Head objects.  The timed unit is a tick: all S slots' events on the host.
Before any time is printed the two routes are compared at the timed size, at 0.9 and again with --check-thresholds beside it (where there
are detections to compare): the same (slot, keyword, time, threshold) lists with bit-equal scores (the same handle, the same embedding
batch, the same head kernel per row, the same detector per lane).  Blocks of --block ticks alternate between the routes after the warm-up
passes; only ticks that complete a window are timed.  Reported: median and p99 wall time per tick, device time per graph replay (events),
bytes downloaded per tick (from shapes).  The condition DESIGN.md section 21 states is printed as a PASS / MISS line: at the paired size the
median tick of (b) is not above that of (a).  --routed-only SxP measures (b) alone at S slots of P routes each; with --shared-too route
(a) is tried there as well, and a refusal of its own limits is reported instead of a time.

  python tools/bench_live_routes.py [--seconds 10] [--slots 64] [--per-slot 2] [--routed-only 256x4] [--shared-too] [--block 50]
                                    [--check-thresholds 0.3,0.5,0.7] [--commit HASH] [--out profiles/live_routes.txt]"""
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
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--slots", type=int, default=64, help="slots of the paired measurement")
    ap.add_argument("--per-slot", type=int, default=2, help="keywords of its own per slot there")
    ap.add_argument("--routed-only", default="256x4", help="SxP: further sizes measured on the routed group alone (comma-separated, may be empty)")
    ap.add_argument("--shared-too", action="store_true", help="try route (a) at the --routed-only sizes as well")
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--check-thresholds", default="0.3,0.5,0.7", help="further thresholds of the equality pass (not timed)")
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from multilingual_kws_amd import synth
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa, transfer_learning as tl
    from multilingual_kws_amd.head import Head
    from oracle import head_oracle as ho
    assert torch.cuda.is_available(), "bench_live_routes.py measures on a GPU; there is nothing to report without one"
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

    thr, hop, clip, hop_ms = 0.9, 320, 16000, 20.0
    more = sorted(set(float(t) for t in args.check_thresholds.split(",") if t) | {thr})
    ticks = args.seconds * 16000 // hop
    sizes = [(args.slots, args.per_slot, True)]
    for item in args.routed_only.split(","):
        if item:
            S, P = (int(x) for x in item.lower().split("x"))
            sizes.append((S, P, args.shared_too))

    def streams(S):
        return [np.concatenate([synth.clips_int16(1, first_clip=(s * args.seconds + i) % 200)[0] for i in range(args.seconds)]).astype(np.float32) / 32768
                for s in range(S)]

    def p99(ts):
        ts = sorted(ts)
        return ts[min(len(ts) - 1, int(0.99 * len(ts)))]

    def line(ts):
        ts = sorted(ts)
        return f"median {statistics.median(ts) * 1e3:8.3f} ms   p99 {p99(ts) * 1e3:8.3f} ms   (min {ts[0] * 1e3:.3f}, n={len(ts)})"

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

    def walk(S, audio, routes, timed):
        """One pass over the streams, blocks alternating between the routes -> (found per route: sorted-per-tick [(slot, keyword, time_ms,
        score, threshold)], tick times per route)."""
        found, series = {name: [] for name, _, _ in routes}, {name: [] for name, _, _ in routes}
        for _, group, _ in routes:
            group.reset()
        for b0 in range(0, ticks, args.block):
            order = routes if (b0 // args.block) % 2 == 0 else routes[::-1]
            for name, group, own in order:
                for i in range(b0, min(ticks, b0 + args.block)):
                    t0 = time.perf_counter()
                    got = group.feed([a[i * hop:(i + 1) * hop] for a in audio])
                    # (a): the host discards what a slot does not own; (b): every row is the slot's own
                    rows = [[s] + r for s in range(S) for r in got[s] if own is None or r[0] in own[s]]
                    if timed and (i + 1) * hop >= clip:
                        series[name].append(time.perf_counter() - t0)
                    found[name] += sorted(rows, key=lambda r: (r[2], r[0], r[1], r[4]))
        return found, series

    say(f"# tools/bench_live_routes.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
    say(f"# per slot a {args.seconds} s stream, {ticks} ticks of {hop} samples, threshold {thr}; (a) one LiveSessionGroup with every head shared, the host "
        f"discarding foreign keywords, (b) one LiveRoutedGroup with a route per owned keyword; one embedding handle; blocks of {args.block} ticks alternate")
    verdict = None
    for S, P, shared in sizes:
        K = S * P
        audio = streams(S)
        emb, _ = tl.load_base_model("synthetic", max_batch=S)
        heads = []
        for k in range(K):
            p = ho.glorot_uniform_params(seed=2000 + k)
            p[-1] += 0.5 + 0.1 * (k % 7)
            heads.append(Head(max_batch=S, params=p, device=dev))
        keywords = [f"kw{k:04d}" for k in range(K)]
        own = [set(keywords[s * P:(s + 1) * P]) | {"_silence_"} for s in range(S)]
        flags = sa.default_live_flags([thr])

        def routed(thresholds):
            g = sa.LiveRoutedGroup(emb, heads, S, max_routes=K, n_thresholds=len(thresholds), flags=flags)
            for s in range(S):
                for k in range(s * P, (s + 1) * P):
                    g.attach(s, k, keywords[k], thresholds)
            return g

        def shared_group(thresholds):
            return sa.LiveSessionGroup(streams=S, thresholds=thresholds, flags=flags, embedding=emb, heads=heads, keywords=keywords)
        say(f"S = {S} slots x {P} keywords of their own = {K} heads / routes")
        b = routed([thr])
        a = None
        if shared:
            try:
                a = shared_group([thr])
            except Exception as e:                                         # its own limits (memory, sizes): reported, (b) is measured alone
                say(f"  (a) cannot be built at this size: {type(e).__name__}: {str(e)[:200]}")
        routes = ([("a", a, own)] if a is not None else []) + [("b", b, None)]
        found, _ = walk(S, audio, routes, False)                           # warm-up pass = the comparison at the timed size
        assert all(b.windows_seen(s) == 1 + (ticks * hop - clip) // hop for s in range(S)) and b.recaptures == 0
        wide_b = routed(more)
        wide_a = shared_group(more) if a is not None else None
        wide, _ = walk(S, audio, ([("a", wide_a, own)] if wide_a is not None else []) + [("b", wide_b, None)], False)
        if a is not None:
            assert found["a"] == found["b"], f"S = {S}: the shared group and the routed group disagree: nothing below would mean anything"
            assert wide["a"] == wide["b"], f"S = {S}: the shared group and the routed group disagree at the further thresholds"
            assert len(wide["b"]) > 0, "the comparison at the further thresholds is empty"
            say(f"  {len(found['b'])} detections at {thr}, {len(wide['b'])} at {more}: the same (slot, keyword, time, threshold) in both routes, scores bit for bit")
            wide_a.close()
        else:
            say(f"  {len(found['b'])} detections at {thr}, {len(wide['b'])} at {more} (routed group alone)")
        wide_b.close()
        found2, series = walk(S, audio, routes, True)
        assert found2 == found
        torch.cuda.synchronize()
        if a is not None:
            say(f"  (a) LiveSessionGroup.feed + discard, per tick: {line(series['a'])}")
        say(f"  (b) LiveRoutedGroup.feed, per tick:           {line(series['b'])}")
        say(f"  device time per graph replay (events, 200 back to back):  (b) {replay_ms(b.graph):.4f} ms" +
            (f"   (a) {replay_ms(a.graph):.4f} ms" if a is not None else ""))
        say(f"  bytes downloaded per tick (from shapes):                  (b) {8 * b.out.numel()}" + (f"   (a) {8 * a.out.numel()}" if a is not None else ""))
        if a is not None and (S, P) == (args.slots, args.per_slot):
            ma, mb = statistics.median(series["a"]), statistics.median(series["b"])
            verdict = mb <= ma
            say(f"{'PASS' if verdict else 'MISS'}: S = {S} x {P}: (b) = {mb * 1e3:.3f} ms {'<=' if verdict else '>'} (a) = {ma * 1e3:.3f} ms ({ma / mb:.2f}x)")
        for g in (a, b):
            if g is not None:
                g.close()
        for hd in heads:
            hd.close()
        emb.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if verdict in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
