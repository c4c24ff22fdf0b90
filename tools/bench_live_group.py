"""S live streams from 20 ms of new audio each to their detections on the host: S LiveSessions fed one after the other against one
LiveSessionGroup.  One process, one MI355X.  The workload of tools/bench_live.py per slot: a 10 s synthetic stream (distinct clips per
slot), 50 keyword heads (seeds 2000 .. 2049, their target class biased as there), 320-sample pushes, one threshold 0.9 -- which these
synthetic heads do not reach: the timed configuration reports no detection.

  (a) what a caller of the parent commit writes: S LiveSessions on ONE shared one-window embedding handle (the handle a single live stream
      is fastest on), fed one after the other every tick: S uploads of 1 280 B, S graph replays, S copies back, S synchronisations
  (b) one LiveSessionGroup.feed on a handle of S windows: one upload of the [S, 320] audio and the active mask, one graph replay (frontend
      push of all slots, the embedding at batch S, the heads, the detector step of all slots), one copy of the packed counts and events back

The timed unit is a tick: all S slots' events on the host.  Before any time is printed the two routes are compared at the timed size, at
0.9 and again with --check-thresholds beside it (where there are detections to compare): for S = 1 on the same handle the lists are equal
with bit-equal scores, which LiveSessionGroup promises; for S > 1 the embedding runs another plan at batch S, so the lists must name the
same (slot, keyword, time, threshold) with scores equal to rtol 1e-4 -- and the largest difference between the probabilities of the two
routes is printed, as is whether slot 0's probabilities are bit-identical when the other slots are fed zeros instead of their streams.
Blocks of --block ticks alternate between the routes after the warm-up passes; only ticks that complete a window are timed.  Reported per
S: median and p99 wall time per tick, device time per graph replay (events), host-to-device bytes per tick (from shapes), and the largest
measured S whose p99 tick stays under the 20 ms hop.  S in --group-only is measured for (b) alone.  The condition DESIGN.md section 20
states is printed as a PASS / MISS line: at S = 64 the median tick of (b) is at most a quarter of (a)'s.

  python tools/bench_live_group.py [--seconds 10] [--heads 50] [--sizes 1,16,64] [--group-only 256] [--block 50] [--check-thresholds 0.3,0.5,0.7]
                                   [--commit HASH] [--out profiles/live_group.txt]"""
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
    ap.add_argument("--heads", type=int, default=50)
    ap.add_argument("--sizes", default="1,16,64", help="numbers of slots measured on both routes")
    ap.add_argument("--group-only", default="256", help="numbers of slots measured on the group alone")
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
    assert torch.cuda.is_available(), "bench_live_group.py measures on a GPU; there is nothing to report without one"
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

    K, thr, hop, clip, hop_ms = args.heads, 0.9, 320, 16000, 20.0
    both = [int(x) for x in args.sizes.split(",") if x]
    alone = [int(x) for x in args.group_only.split(",") if x]
    more = sorted(set(float(t) for t in args.check_thresholds.split(",") if t) | {thr})
    keywords = [f"kw{k:02d}" for k in range(K)]
    params = []
    for k in range(K):
        p = ho.glorot_uniform_params(seed=2000 + k)
        p[-1] += 0.5 + 0.1 * (k % 7)
        params.append(p)
    handles = {}

    def models_for(max_batch):
        if max_batch not in handles:
            emb, blob = tl.load_base_model("synthetic", max_batch=max_batch)
            handles[max_batch] = [tl.TransferLearnedModel(emb, Head(max_batch=max_batch, params=p, device=dev), blob, "synthetic") for p in params]
        return handles[max_batch]
    ticks = args.seconds * 16000 // hop
    flags = sa.default_live_flags([thr])

    def streams(S):
        return [np.concatenate([synth.clips_int16(1, first_clip=(s * args.seconds + i) % 200)[0] for i in range(args.seconds)]).astype(np.float32) / 32768
                for s in range(S)]

    def walk(S, audio, sessions, group, timed, probe=None):
        """One pass over the streams, blocks alternating between the routes -> (found per route: [(slot, keyword, time_ms, score, threshold)],
        tick times per route).  probe(i): called after both routes have run tick i's block (untimed passes only)."""
        found, series = dict(a=[], b=[]), dict(a=[], b=[])
        for s in sessions or []:
            s.reset()
        group.reset()

        def feed_a(i):
            out = []
            for s in range(S):
                out += [[s] + r for r in sessions[s].feed(audio[s][i * hop:(i + 1) * hop])]
            return out

        def feed_b(i):
            got = group.feed([a[i * hop:(i + 1) * hop] for a in audio])
            return [[s] + r for s in range(S) for r in got[s]]
        routes = (("a", feed_a), ("b", feed_b)) if sessions else (("b", feed_b),)
        block = 1 if probe else args.block                                  # the probe compares the two routes' buffers tick by tick
        for b0 in range(0, ticks, block):
            order = routes if (b0 // block) % 2 == 0 else routes[::-1]
            for name, feed in order:
                for i in range(b0, min(ticks, b0 + block)):
                    t0 = time.perf_counter()
                    found[name] += feed(i)
                    if timed and (i + 1) * hop >= clip:
                        series[name].append(time.perf_counter() - t0)
            if probe and (b0 + 1) * hop >= clip:
                probe(b0)
        return found, series

    def line(ts):
        ts = sorted(ts)
        return f"median {statistics.median(ts) * 1e3:8.3f} ms   p99 {p99(ts) * 1e3:8.3f} ms   (min {ts[0] * 1e3:.3f}, n={len(ts)})"

    def p99(ts):
        ts = sorted(ts)
        return ts[min(len(ts) - 1, int(0.99 * len(ts)))]

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

    def same(S, a, b):
        if S == 1:
            return a == b                                                   # same handle, same batch, same plan: bit for bit
        key = lambda r: (r[2], r[0], r[1], r[4])                            # noqa: E731  (time, slot, keyword, threshold)
        a, b = sorted(a, key=key), sorted(b, key=key)
        return [key(r) for r in a] == [key(r) for r in b] and np.allclose([r[3] for r in a], [r[3] for r in b], rtol=1e-4, atol=0)

    say(f"# tools/bench_live_group.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
    say(f"# per slot a {args.seconds} s stream, {ticks} ticks of {hop} samples, {K} heads, threshold {thr}; (a) S LiveSessions on one one-window "
        f"handle, (b) one LiveSessionGroup on a handle of S windows; blocks of {args.block} ticks alternate between the routes")
    medians, under = {}, dict(a=0, b=0)
    for S in both + alone:
        audio = streams(S)
        paired = S in both
        group_models = models_for(S)
        sessions = [sa.LiveSession(models_for(1), [thr], flags=flags, keywords=keywords) for _ in range(S)] if paired else None
        group = sa.LiveSessionGroup(group_models, streams=S, thresholds=[thr], flags=flags, keywords=keywords)
        found, _ = walk(S, audio, sessions, group, False)                   # warm-up pass = the comparison at the timed size
        assert all(group.windows_seen(s) == 1 + (ticks * hop - clip) // hop for s in range(S)) and group.recaptures == 0
        wide_group = sa.LiveSessionGroup(group_models, streams=S, thresholds=more, flags=flags, keywords=keywords)
        notes = ""
        if paired:
            assert same(S, found["a"], found["b"]), f"S = {S}: the LiveSessions and the group disagree: nothing below would mean anything"
            wide = [sa.LiveSession(models_for(1), more, flags=flags, keywords=keywords) for _ in range(S)]
            gap = torch.zeros((), dtype=torch.float32, device=dev)
            mine = []

            def probe(i):
                theirs = torch.stack([w.probs[:, 0] for w in wide], dim=1)                      # [K, S, 3]
                gap.copy_(torch.maximum(gap, (wide_group.probs - theirs).abs().max()))
                mine.append(wide_group.probs[:, 0].clone())
            found_wide, _ = walk(S, audio, wide, wide_group, False, probe if S == max(both) else None)
            assert same(S, found_wide["a"], found_wide["b"]), f"S = {S}: the LiveSessions and the group disagree at the further thresholds"
            notes = f"{len(found['a'])} detections at {thr}, {len(found_wide['a'])} at {more}: the same in both routes" + \
                    (", scores bit for bit" if S == 1 else ", scores to rtol 1e-4")
            if S == max(both) and S > 1:
                # slot 0 again with every other slot fed zeros: are its probability rows the same bits?
                zeros = [audio[0]] + [np.zeros_like(audio[0])] * (S - 1)
                wide_group.reset()
                alone_rows = []
                for i in range(ticks):
                    wide_group.feed([a[i * hop:(i + 1) * hop] for a in zeros])
                    if (i + 1) * hop >= clip:
                        alone_rows.append(wide_group.probs[:, 0].clone())
                isolated = len(alone_rows) == len(mine) and all(torch.equal(x, y) for x, y in zip(alone_rows, mine))
                say(f"S = {S}: largest |probability in the group - probability in the slot's own batch-1 LiveSession| over all slots and windows: "
                    f"{float(gap.cpu()):.3e} (another embedding plan at batch {S}; reported, not asserted)")
                say(f"S = {S}: slot 0's probability rows with the other {S - 1} slots fed zeros instead of their streams: "
                    f"{'bit-identical' if isolated else 'NOT bit-identical'}")
            for w in wide:
                w.close()
        else:
            found_wide, _ = walk(S, audio, None, wide_group, False)
            notes = f"{len(found['b'])} detections at {thr}, {len(found_wide['b'])} at {more} (group alone)"
        wide_group.close()
        found2, series = walk(S, audio, sessions, group, True)
        assert found2 == found
        torch.cuda.synchronize()
        say(f"S = {S}: {notes}")
        if paired:
            say(f"  (a) {S:3d} x LiveSession.feed, per tick:     {line(series['a'])}")
        say(f"  (b) LiveSessionGroup.feed, per tick:      {line(series['b'])}")
        rep = f"(b) {replay_ms(group.graph):.4f} ms" + (f"   (a) {replay_ms(sessions[0].graph):.4f} ms per session, x {S}" if paired else "")
        say(f"  device time per graph replay (events, 200 back to back):  {rep}")
        say(f"  host-to-device bytes per tick (from shapes):              (b) {4 * (S * hop + S)}" + (f"   (a) {S} x {4 * hop} = {4 * hop * S}" if paired else ""))
        for name in series:
            if series[name]:
                medians[(name, S)] = statistics.median(series[name])
                if p99(series[name]) * 1e3 < hop_ms:
                    under[name] = max(under[name], S)
        for s in sessions or []:
            s.close()
        group.close()
    say(f"largest measured S whose p99 tick stays under the {hop_ms:.0f} ms hop:  (a) {under['a']} of {both}   (b) {under['b']} of {both + alone}")
    ok = True
    if ("a", 1) in medians:
        say(f"S = 1: (b) = {medians[('b', 1)] * 1e3:.3f} ms beside (a) = {medians[('a', 1)] * 1e3:.3f} ms (the group carries a mask upload and per-slot bookkeeping)")
    if ("a", 64) in medians:
        a, b = medians[("a", 64)], medians[("b", 64)]
        ok = b <= a / 4
        say(f"{'PASS' if ok else 'MISS'}: S = 64: (b) = {b * 1e3:.3f} ms {'<=' if ok else '>'} (a) / 4 = {a / 4 * 1e3:.3f} ms ({a / b:.1f}x)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
