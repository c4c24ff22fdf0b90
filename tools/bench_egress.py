"""Float32 audio in device memory to WAV file images in host memory: the device encode (multilingual_kws_amd/pcm.py,
input_data.encode_wav, batch_streaming_analysis.extract_detections) against the host route a caller had before
it, measured in the same run.  One process, one MI355X.

  (a) 1 024 one-second clips [1024, 16000] -> 1 024 16-bit WAV images:
      .cpu() of the float audio + numpy quantise + the stdlib `wave` writer   against   encode_wav
  (b) 64 detections cut as [t - 1 s, t + 1 s] from a 60 s recording -> 64 16-bit WAV images:
      .cpu() of the recording + numpy slices + numpy quantise + `wave`        against   extract_detections

Equality is asserted before anything is timed: the images of both routes are the same bytes.  The routes are timed in alternating
order after one warm-up each, every call starts from audio in device memory and ends with the images as bytes objects on the host;
medians and the slowest run are reported, and the device time of the encode launch alone from events.  No threshold: the numbers are
the result, whichever route they favour.

  python tools/bench_egress.py [--clips 1024] [--detections 64] [--seconds 60] [--reps 9] [--commit HASH] [--out profiles/egress.txt]"""
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


def few(ts):
    ts = sorted(ts)
    return f"median {statistics.median(ts) * 1e3:9.3f} ms   max {ts[-1] * 1e3:9.3f} ms   (min {ts[0] * 1e3:.3f}, n={len(ts)})"


def host_images(rows, rate):
    """float32 rows on the host -> 16-bit WAV images: numpy quantise (round half to even, clamped), the stdlib writer."""
    images = []
    for row in rows:
        q = np.clip(np.rint(row * np.float32(32768.0)), -32768, 32767).astype("<i2")
        buf = io.BytesIO()
        with wave.open(buf, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(rate)
            w.writeframes(q.tobytes())
        images.append(buf.getvalue())
    return images


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--detections", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=9, help="timed repetitions of each route")
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from multilingual_kws_amd import _lib, pcm, synth
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa
    from multilingual_kws_amd.embedding import input_data
    assert torch.cuda.is_available(), "bench_egress.py measures on a GPU; there is nothing to report without one"
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

    def launch_ms(src, items, out_bytes, reps=100):
        """Device time of one mkws_pcm_encode launch over this table (events, the table uploaded once, back to back)."""
        d_items = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
        out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L, width = _lib.lib(), int(items["n_frames"].max())

        def launch():
            _lib.check(L.mkws_pcm_encode(ctypes.c_void_p(src.data_ptr()), src.numel(), ctypes.c_void_p(d_items.data_ptr()), len(items), width,
                                         ctypes.c_void_p(out.data_ptr()), out_bytes, ctypes.c_void_p(flag.data_ptr()), _lib.current_stream_ptr()))
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            launch()
        stop.record()
        stop.synchronize()
        assert flag.item() == 0
        return start.elapsed_time(stop) / reps

    say(f"# tools/bench_egress.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
    say(f"# device float32 audio -> 16-bit WAV images as bytes on the host; routes alternate; {args.reps} timed runs each after one warm-up")
    N, RATE = 16000, 16000
    # -- (a) a batch of clips ---------------------------------------------------------------------------------------------------------
    x = torch.from_numpy(synth.clips_float32(args.clips, N)).to(dev)
    x = (x * torch.linspace(0.5, 1.5, args.clips, device=dev)[:, None]).contiguous()      # off the 16-bit grid, the loudest rows clipping

    def host_clips():
        return host_images(x.cpu().numpy(), RATE)

    def device_clips():
        return input_data.encode_wav(x, RATE, "s16")
    assert host_clips() == device_clips(), "(a): the two routes write different files"
    s = timed(dict(h=host_clips, d=device_clips), args.reps)
    say(f"(a) {args.clips} clips of {N} samples -> {args.clips} WAV images, 16-bit PCM, {RATE} Hz, mono: both routes write the same bytes")
    say(f"  .cpu() + numpy quantise + wave writer:   {few(s['h'])}")
    say(f"  encode_wav (one launch, one download):   {few(s['d'])}")
    say(f"  encode_wav / host = {statistics.median(s['d']) / statistics.median(s['h']):.4f};  device-to-host bytes: host route {4 * args.clips * N}, "
        f"encode_wav {args.clips * ((2 * N + 48 + 15) & ~15)}")
    items = pcm.make_encode_items([(r * N, N, 0, N, 48 + r * ((2 * N + 48 + 15) & ~15), 0, 0, 1.0, "s16") for r in range(args.clips)])
    ms = launch_ms(x.view(-1), items, args.clips * ((2 * N + 48 + 15) & ~15) + 48)
    nbytes = 6 * args.clips * N
    say(f"  the mkws_pcm_encode launch alone (events, 100 back to back): {ms:.4f} ms for {nbytes / 1e6:.1f} MB of input plus output = {nbytes / ms / 1e9:.3f} TB/s")

    # -- (b) detections cut from one recording ----------------------------------------------------------------------------------------
    n_rec = int(args.seconds * RATE)
    rng = np.random.default_rng(7)
    rec = torch.from_numpy((0.5 * np.sin(2 * np.pi * 180 * np.arange(n_rec) / RATE) + 0.3 * rng.uniform(-1, 1, n_rec)).astype(np.float32)).to(dev)
    times = sorted(int(t) for t in rng.integers(0, int(args.seconds * 1000), args.detections))
    times[0], times[-1] = 300, int(args.seconds * 1000) - 100                      # one window clamped at either end
    detections = [("keyword", t) for t in times]

    def host_detections():
        a = rec.cpu().numpy()
        return host_images([a[s0:s0 + nf] for s0, nf in sa.detection_windows(times, n_rec, RATE)], RATE)

    def device_detections():
        return sa.extract_detections(detections, rec, sample_rate=RATE)
    assert host_detections() == device_detections(), "(b): the two routes write different files"
    s = timed(dict(h=host_detections, d=device_detections), args.reps)
    frames = sum(nf for _, nf in sa.detection_windows(times, n_rec, RATE))
    say(f"(b) {args.detections} detections, [t - 1 s, t + 1 s] of a {args.seconds:g} s recording ({n_rec} samples) -> {args.detections} WAV images, "
        f"16-bit PCM ({frames} frames in all): both routes write the same bytes")
    say(f"  .cpu() of the recording + slices + numpy quantise + wave writer:   {few(s['h'])}")
    say(f"  extract_detections (one launch, one download):                     {few(s['d'])}")
    say(f"  extract_detections / host = {statistics.median(s['d']) / statistics.median(s['h']):.4f};  device-to-host bytes: host route {4 * n_rec}, "
        f"extract_detections about {2 * frames + 64 * args.detections}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
