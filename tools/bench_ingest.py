"""WAV files from the disk to model-rate float32 audio in device memory: the device decode (multilingual_kws_amd/pcm.py,
input_data.read_clips / read_recording) against what a caller had before it.  One process, one MI355X.

  (a) 1 024 one-second 16-bit 16 kHz clip files:   np.stack([_read_wav ...]) + upload   against   read_clips,
      once with the files read from the disk inside the timed call and once from file images already in memory
  (b) one 20-minute 44.1 kHz stereo 16-bit recording:   decode_wav + to_sample_rate   against   read_recording
  (c) 1 024 one-second clips at 48 kHz, 24-bit, stereo: the parent refuses these, so the time reference is
      scipy.io.wavfile.read + scipy.signal.resample_poly + upload (as tools/bench_resample.py), against read_clips

Equality is asserted before anything is timed: (a) and (b) bit for bit against the parent's route, (c) against the numpy restatement
of the decode (tests/util_pcm.py) fed through the same resampler (scipy's pipeline has another filter: a time reference only).  The routes
are timed in alternating order, every call ends in a device synchronise; medians and the slowest run are reported, and the device time of
the decode launch alone from events.  No threshold: the numbers are the result.

  python tools/bench_ingest.py [--clips 1024] [--minutes 20] [--reps 9] [--commit HASH] [--out profiles/ingest.txt]"""
import argparse
import ctypes
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


def few(ts):
    ts = sorted(ts)
    return f"median {statistics.median(ts) * 1e3:9.3f} ms   max {ts[-1] * 1e3:9.3f} ms   (min {ts[0] * 1e3:.3f}, n={len(ts)})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--minutes", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=9, help="timed repetitions of each route")
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    from multilingual_kws_amd import _lib, pcm, synth
    from multilingual_kws_amd.embedding import input_data
    from tests import util_pcm as up
    assert torch.cuda.is_available(), "bench_ingest.py measures on a GPU; there is nothing to report without one"
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

    def bits(t):
        return (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.uint32)

    def timed(routes, reps):
        """routes: {tag: fn}; every fn ends in a synchronise.  One warm-up each, then reps rounds in alternating order."""
        series = {tag: [] for tag in routes}
        for fn in routes.values():
            fn()
        tags = list(routes)
        for r in range(reps):
            for tag in tags if r % 2 == 0 else tags[::-1]:
                t0 = time.perf_counter()
                routes[tag]()
                series[tag].append(time.perf_counter() - t0)
        return series

    def decode_launch_ms(images, sample_rate, n, reps=100):
        """Device time of the one mkws_pcm_decode launch read_clips makes for these files (events, back to back), and its bytes."""
        infos = [pcm.wav_info(b) for b in images]
        takes = []
        for info in infos:
            if info.rate == sample_rate:
                takes.append(min(info.frames, n))
            else:
                g = input_data._resampler_for(info.rate, sample_rate, dev).geometry
                takes.append(min(info.frames, ((n - 1) * g["M"] + g["half"]) // g["L"] + 1))
        d_bytes, offsets = input_data._upload_sample_bytes(images, infos, takes, dev)
        width = max(takes)
        items = pcm.make_items([(offsets[i], takes[i], i * width, width, infos[i].format, infos[i].channels, 0) for i in range(len(images))])
        out = torch.empty(len(images) * width, dtype=torch.float32, device=dev)
        d_items = torch.from_numpy(items.view(np.uint8).copy()).to(dev)          # the table uploaded once: the events bracket launches only
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L = _lib.lib()

        def launch():
            _lib.check(L.mkws_pcm_decode(ctypes.c_void_p(d_bytes.data_ptr()), d_bytes.numel(), ctypes.c_void_p(d_items.data_ptr()), len(items), width,
                                         ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(flag.data_ptr()), _lib.current_stream_ptr()))
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
        nbytes = sum(t * i.frame_bytes for t, i in zip(takes, infos)) + 4 * out.numel()
        return start.elapsed_time(stop) / reps, nbytes

    say(f"# tools/bench_ingest.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
    say(f"# every route ends in a device synchronise; routes alternate; {args.reps} timed runs each after one warm-up")
    N, RATE = 16000, 16000
    with tempfile.TemporaryDirectory() as root:
        # -- (a) canonical clips ------------------------------------------------------------------------------------------------------
        x = synth.clips_int16(args.clips, N, seed=0x1A6E5700)
        files = []
        for i in range(args.clips):
            files.append(os.path.join(root, f"a{i}.wav"))
            with open(files[-1], "wb") as fh:
                fh.write(synth.wav_bytes(x[i]))
        images = [open(f, "rb").read() for f in files]

        def parent_files():
            t = torch.from_numpy(np.stack([input_data._read_wav(f, N) for f in files])).to(dev)
            torch.cuda.synchronize()
            return t

        def parent_memory():
            t = torch.from_numpy(np.stack([input_data.decode_wav(b, N)[0] for b in images])).to(dev)
            torch.cuda.synchronize()
            return t

        def new_files():
            t = input_data.read_clips(files, RATE, N)
            torch.cuda.synchronize()
            return t

        def new_memory():
            t = input_data.read_clips(images, RATE, N)
            torch.cuda.synchronize()
            return t
        want = bits(parent_files())
        assert np.array_equal(bits(new_files()), want) and np.array_equal(bits(new_memory()), want) and np.array_equal(bits(parent_memory()), want)
        s = timed(dict(pf=parent_files, nf=new_files, pm=parent_memory, nm=new_memory), args.reps)
        say(f"(a) {args.clips} clip files, 16-bit PCM, 16 kHz, mono, {N} samples: read_clips equals np.stack([_read_wav ...]) bit for bit")
        say(f"  files read inside the call:   parent np.stack([_read_wav ...]) + upload:   {few(s['pf'])}")
        say(f"                                read_clips(paths):                          {few(s['nf'])}")
        say(f"                                read_clips / parent = {statistics.median(s['nf']) / statistics.median(s['pf']):.4f}")
        say(f"  file images in memory:        parent np.stack([decode_wav ...]) + upload: {few(s['pm'])}")
        say(f"                                read_clips(images):                         {few(s['nm'])}")
        say(f"                                read_clips / parent = {statistics.median(s['nm']) / statistics.median(s['pm']):.4f}")
        ms, nbytes = decode_launch_ms(images, RATE, N)
        say(f"  the mkws_pcm_decode launch alone (events, 100 back to back): {ms:.4f} ms for {nbytes / 1e6:.1f} MB of input plus output "
            f"= {nbytes / ms / 1e9:.3f} TB/s;  host-to-device bytes: parent {4 * args.clips * N}, read_clips {2 * args.clips * N}")

        # -- (b) one long recording ---------------------------------------------------------------------------------------------------
        frames = int(args.minutes * 60 * 44100)
        rng = np.random.default_rng(2)
        rec = rng.integers(-12000, 12000, (frames, 2), dtype=np.int16)
        rec_path = os.path.join(root, "recording.wav")
        with open(rec_path, "wb") as fh:
            fh.write(up.wav_image("s16", 2, 44100, rec.tobytes()))
        del rec

        def parent_rec():
            with open(rec_path, "rb") as fh:
                a, rate = input_data.decode_wav(fh.read())
            t = input_data.to_sample_rate(torch.from_numpy(a).to(dev), rate, RATE)
            torch.cuda.synchronize()
            return t

        def new_rec():
            t = input_data.read_recording(rec_path, RATE)
            torch.cuda.synchronize()
            return t
        assert np.array_equal(bits(new_rec()), bits(parent_rec()))
        s = timed(dict(p=parent_rec, n=new_rec), args.reps)
        say(f"(b) one {args.minutes:g}-minute recording, 16-bit PCM, 44.1 kHz, stereo ({frames} frames, {4 * frames / 1e6:.0f} MB of samples): "
            "read_recording equals decode_wav + to_sample_rate bit for bit")
        say(f"  parent decode_wav + upload + to_sample_rate:   {few(s['p'])}")
        say(f"  read_recording:                                {few(s['n'])}")
        say(f"  read_recording / parent = {statistics.median(s['n']) / statistics.median(s['p']):.4f};  host-to-device bytes: parent {4 * frames} "
            f"(float32, first channel), read_recording {4 * frames} (both channels, 16-bit)")
        with open(rec_path, "rb") as fh:
            ms, nbytes = decode_launch_ms([fh.read()], 44100, frames, reps=20)
        say(f"  the mkws_pcm_decode launch alone (events, 20 back to back): {ms:.4f} ms for {nbytes / 1e6:.1f} MB of input plus output = {nbytes / ms / 1e9:.3f} TB/s")
        os.remove(rec_path)

        # -- (c) 48 kHz, 24-bit, stereo clips -------------------------------------------------------------------------------------------
        n_c = min(args.clips, 1024)
        files_c = []
        for i0 in range(0, n_c, 64):                       # generated 64 files at a time: the synthesis works in float64
            hi = synth.clips_int16(2 * min(64, n_c - i0), 48000, seed=0x1A6E5C00, first_clip=2 * i0)
            for i in range(i0, min(n_c, i0 + 64)):
                files_c.append(os.path.join(root, f"c{i}.wav"))
                pair = np.stack([hi[2 * (i - i0)], hi[2 * (i - i0) + 1]], axis=1)
                with open(files_c[-1], "wb") as fh:
                    fh.write(up.wav_image("s24", 2, 48000, up.from_int16("s24", pair), extensible=True))
        del hi

        def scipy_route():
            rows = []
            for f in files_c:
                _, a = wavfile.read(f)
                rows.append(a[:, 0].astype(np.float32) / np.float32(2147483648.0))
            y = resample_poly(np.stack(rows), 1, 3, axis=1).astype(np.float32)[:, :N]
            t = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
            torch.cuda.synchronize()
            return t

        def new_c():
            t = input_data.read_clips(files_c, RATE, N)
            torch.cuda.synchronize()
            return t
        # the gate: the numpy restatement of the decode through the same resampler, for the first, a middle and the last file
        got = bits(new_c())
        for i in sorted({0, n_c // 2, n_c - 1}):
            image = open(files_c[i], "rb").read()
            info = pcm.wav_info(image)
            a = up.decode_frames(info.format, info.channels, image[info.data_offset:info.data_offset + info.frames * info.frame_bytes], 0)
            assert np.array_equal(got[i], input_data.to_sample_rate(a, 48000, RATE)[:N].view(np.uint32)), f"(c): file {i} differs from the restatement"
        try:
            input_data._read_wav(files_c[0], N)
            raise AssertionError("the parent's reader took a 24-bit file")
        except ValueError:
            pass
        s = timed(dict(p=scipy_route, n=new_c), max(3, args.reps // 3))
        say(f"(c) {n_c} clip files, 24-bit PCM (extensible header), 48 kHz, stereo, 48000 frames: the parent's readers refuse them; read_clips equals "
            "the numpy restatement of the decode fed through the same resampler, bit for bit (3 files)")
        say(f"  scipy.io.wavfile.read + resample_poly + upload (a time reference: another filter):   {few(s['p'])}")
        say(f"  read_clips:                                                                          {few(s['n'])}")
        say(f"  read_clips / scipy = {statistics.median(s['n']) / statistics.median(s['p']):.4f}")
        ms, nbytes = decode_launch_ms([open(f, "rb").read() for f in files_c], RATE, N)
        say(f"  the mkws_pcm_decode launch alone (events, 100 back to back): {ms:.4f} ms for {nbytes / 1e6:.1f} MB of input plus output = {nbytes / ms / 1e9:.3f} TB/s")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
