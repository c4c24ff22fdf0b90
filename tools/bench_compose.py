"""Test streams strung together from sentences in device memory and written as 16-bit WAV images: the device route
(embedding/generate_stream_sentences.write_streams: mkws_stream_power, mkws_stream_bed_gain, mkws_stream_mix, mkws_pcm_encode, one
download) against the host route a caller had before it, measured in the same run.  One process, one MI355X.

  (a) R streams of S target + S non-target sentences of 2-6 s (seeded synthetic audio, drawn from a pool) over a 60 s bed at 10 dB:
      .cpu() of the pieces + np.concatenate + numpy mix at the device's gains + numpy quantise + the stdlib `wave` writer
      against   write_streams(..., background=bed, snr_db=10)
  (b) the mkws_stream_mix launch of the largest shape alone, by device events, 100 back to back: bytes read plus written over time.

Equality is asserted before anything is timed: the images of both routes are the same bytes (the host route is handed the gains the
device found; it does not compute them).  The routes are timed in alternating order after one warm-up each, every call starts from
audio in device memory and ends with the images as bytes objects on the host; medians and the slowest run are reported.  No
threshold: the numbers are the result, whichever route they favour.

  python tools/bench_compose.py [--shapes 64x40,8x10,1x2] [--pool 512] [--reps 9] [--commit HASH] [--out profiles/compose.txt]"""
import argparse
import ctypes
import io
import os
import statistics
import subprocess
import sys
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RATE = 16000


def few(ts):
    ts = sorted(ts)
    return f"median {statistics.median(ts) * 1e3:9.3f} ms   max {ts[-1] * 1e3:9.3f} ms   (min {ts[0] * 1e3:.3f}, n={len(ts)})"


def wav_image(q):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(RATE)
        w.writeframes(q.tobytes())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="64x40,8x10,1x2", help="streams x target sentences (as many non-target ones), the largest first")
    ap.add_argument("--pool", type=int, default=512, help="distinct sentences the streams draw from")
    ap.add_argument("--reps", type=int, default=9, help="timed repetitions of each route")
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from multilingual_kws_amd import _lib, compose, synth
    from multilingual_kws_amd.embedding import generate_stream_sentences as gss
    from multilingual_kws_amd.embedding.generate_stream_sentences import StreamPiece
    assert torch.cuda.is_available(), "bench_compose.py measures on a GPU; there is nothing to report without one"
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

    def timed(routes, reps):
        """routes: {tag: fn}.  One warm-up each, then reps rounds in alternating order."""
        series = {tag: [] for tag in routes}
        for fn in routes.values():
            fn()
        tags = list(routes)
        for r in range(reps):
            for tag in tags if r % 2 == 0 else tags[::-1]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                routes[tag]()
                series[tag].append(time.perf_counter() - t0)
        return series

    say(f"# tools/bench_compose.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
    say(f"# sentences in device memory -> streams over a bed at 10 dB -> 16-bit WAV images as bytes on the host; routes alternate; "
        f"{args.reps} timed runs each after one warm-up")
    rng = np.random.default_rng(25)
    lengths = rng.integers(2 * RATE, 6 * RATE + 1, args.pool)
    clips = synth.clips_float32(args.pool, 6 * RATE) * np.float32(0.5)
    pool = [torch.from_numpy(np.ascontiguousarray(clips[i, :lengths[i]])).to(dev) for i in range(args.pool)]
    bed = torch.from_numpy(synth.clips_float32(1, 60 * RATE, seed=0x5EED0025)[0] * np.float32(0.3)).to(dev)
    biggest = None

    for shape in args.shapes.split(","):
        R, S = (int(v) for v in shape.split("x"))
        streams, picks = [], []
        for r in range(R):
            idx = rng.integers(0, args.pool, 2 * S)
            picks.append(idx)
            streams.append([StreamPiece(pool[i], is_target=k % 2 == 0, keyword="kw", start_s=0.5, end_s=1.0) for k, i in enumerate(idx)])
        kw = dict(background=bed, snr_db=10.0)
        images, labels, gains = gss.write_streams(streams, format="s16", **kw)
        g_host = gains.cpu().numpy()

        def device_route():
            return gss.write_streams(streams, format="s16", **kw)[0]

        def host_route():
            host_pool = {int(i): pool[int(i)].cpu().numpy() for i in set(np.concatenate(picks).tolist())}
            b = bed.cpu().numpy()
            out = []
            for r in range(R):
                fg = np.concatenate([host_pool[int(i)] for i in picks[r]])
                y = fg + b[np.arange(fg.size) % b.size] * g_host[r]
                y = np.clip(y, np.float32(-1), np.float32(1))
                out.append(wav_image(np.clip(np.rint(y * np.float32(32768.0)), -32768, 32767).astype("<i2")))
            return out
        assert host_route() == images == device_route(), f"{shape}: the two routes write different files"
        s = timed(dict(h=host_route, d=device_route), args.reps)
        frames = sum(len(im) - 44 for im in images) // 2
        say(f"(a) {R} streams of {S} target + {S} non-target sentences ({frames} frames, {frames / RATE:.0f} s of audio in all; "
            f"{len(set(np.concatenate(picks).tolist()))} distinct sentences): both routes write the same bytes")
        say(f"  .cpu() + concatenate + numpy mix + quantise + wave writer:   {few(s['h'])}")
        say(f"  write_streams (power, gain, mix, encode, one download):     {few(s['d'])}")
        say(f"  write_streams / host = {statistics.median(s['d']) / statistics.median(s['h']):.4f};  device-to-host bytes: host route "
            f"{4 * (sum(int(lengths[i]) for i in set(np.concatenate(picks).tolist())) + bed.numel())}, write_streams about {2 * frames}")
        if biggest is None:
            biggest = (shape, streams, kw, frames)

    # -- (b) the mix launch alone -----------------------------------------------------------------------------------------------------
    shape, streams, kw, frames = biggest
    c = gss._compose(streams, RATE, **kw)
    src = c.src
    keep, p_items, p_descs = compose.upload_tables(c.items, c.descs, dev)
    out = torch.empty(max(sum(c.lengths), 1), dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L, max_out = _lib.lib(), max(c.lengths)

    def launch():
        _lib.check(L.mkws_stream_mix(ctypes.c_void_p(src.data_ptr()), src.numel(), ctypes.c_void_p(p_items), len(c.items), ctypes.c_void_p(p_descs),
                                     len(c.descs), ctypes.c_void_p(c.bed_gain.data_ptr()), 1, max_out, ctypes.c_void_p(out.data_ptr()), out.numel(),
                                     ctypes.c_void_p(flag.data_ptr()), _lib.current_stream_ptr()))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    assert flag.item() == 0 and torch.equal(out[:sum(c.lengths)], c.audio), "(b): the bare launch differs from compose_streams"
    start.record()
    for _ in range(100):
        launch()
    stop.record()
    stop.synchronize()
    ms = start.elapsed_time(stop) / 100
    nbytes = 12 * frames                                     # per position: a source float and a bed float read, a float written
    say(f"(b) the mkws_stream_mix launch of {shape} alone (events, 100 back to back): {ms:.4f} ms for {nbytes / 1e6:.1f} MB read plus written "
        f"= {nbytes / ms / 1e9:.3f} TB/s   ({len(c.items)} items, {len(c.descs)} streams, {sum((n + 1023) // 1024 for n in c.lengths)} tiles with work "
        f"of {len(c.descs) * ((max_out + 1023) // 1024)} launched)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
