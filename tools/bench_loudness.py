"""Level normalisation on the device (multilingual_kws_amd/loudness.py) against what a caller had before it.  One
process, one MI355X.  Two workloads, both float32 at 16 kHz and already in device memory, as read_clips / read_recording leave them:

  bank       --rows x --samples clips (1 024 x 16 000)
  recording  one row of --seconds seconds (600 s)

and on each, `measure` (the statistics and the gains, left on the device) and `normalize` (measure, then the levelled audio), by three routes:

  device   LoudnessMeter.measure / .normalize(out=...)
  host     the path a user has today: .cpu(), scipy.signal.lfilter in float64 (both biquads), the gating in numpy, the gains uploaded
           (normalize: and one multiply on the device).  The true peak is left out of this route: it has nothing to compute it with.
  torch    the same measurement composed from torch operators on the same device: torchaudio.functional.lfilter where importable,
           else the rfft of the row times the K-filter's frequency response and the irfft (float64, zero-padded by --pad samples: the
           recursion's tail, cut there); hop sums, unfolded block sums and masked means for the gates; conv1d with the four phases of
           the true-peak filter and a maximum.

Device events around --reps calls make a window; every route gets --windows windows, the routes alternating after a warm-up of each, and
the median window is reported (the host route, which ends in a synchronising copy, is timed by the host clock, one call a window).
Before any time is printed the routes' loudness readings are compared with the device's.  The achieved bytes per second of `measure` are
the bytes the measurement needs (every sample once, 4 bytes) over its time, beside the 6.29 TB/s streaming figure of SURVEY.md section 8d.

  python tools/bench_loudness.py [--rows 1024] [--samples 16000] [--seconds 600] [--reps 20] [--windows 7] [--pad 8192]
                                 [--commit HASH] [--out profiles/loudness_bench.txt]"""
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
RATE = 16000


def gate(z):
    """numpy float64 block mean squares [B, nb] -> integrated loudness [B] (the two gates of BS.1770)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
        a = l > -70.0
        gamma = -0.691 + 10.0 * np.log10((z * a).sum(1) / a.sum(1)) - 10.0
        r = a & (l > gamma[:, None])
        return -0.691 + 10.0 * np.log10((z * r).sum(1) / r.sum(1))


def nice(n):
    """The smallest 2^a 3^b 5^c that is at least n: a length the FFT library has radix kernels for."""
    best = 1 << (n - 1).bit_length()
    p5 = 1
    while p5 < best:
        p35 = p5
        while p35 < best:
            m = p35
            while m < n:
                m *= 2
            best = min(best, m)
            p35 *= 3
        p5 *= 5
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window of a device route")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--pad", type=int, default=8192, help="zero padding of the rfft route: where the recursion's tail is cut")
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from scipy.signal import lfilter
    from multilingual_kws_amd import loudness, resample
    from tests.util_loudness import ramp_noise
    assert torch.cuda.is_available(), "bench_loudness.py measures on a GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    try:
        from torchaudio.functional import lfilter as ta_lfilter
    except ImportError:
        ta_lfilter = None
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"bench_loudness  commit {commit}  device {torch.cuda.get_device_name(dev)}  torch {torch.__version__}  "
        f"torch route: {'torchaudio.functional.lfilter' if ta_lfilter else 'rfft x K-response x irfft (float64)'}")
    hop, block = RATE // 10, 4 * (RATE // 10)
    coef = loudness.coeffs(RATE)
    tab = torch.from_numpy(np.ascontiguousarray(resample.host_taps(resample.make_cfg(1, 4)).T[:, None, ::-1])).to(dev)      # [4, 1, T] for conv1d
    zc = (tab.shape[2] - 1) // 2

    def k_response(n_fft):
        w = torch.exp(-2j * torch.pi * torch.arange(n_fft // 2 + 1, dtype=torch.float64, device=dev) / n_fft)
        h = torch.ones_like(w)
        for b0, b1, b2, a1, a2 in coef:
            h = h * (b0 + b1 * w + b2 * w * w) / (1.0 + a1 * w + a2 * w * w)
        return h

    for name, B, n in (("bank", args.rows, args.samples), ("recording", 1, args.seconds * RATE)):
        host_x = np.stack([ramp_noise(n, RATE, 7 + b, lo_db=-45.0 + (b % 30), hi_db=-20.0 + (b % 15)) for b in range(min(B, 32))])
        host_x = np.ascontiguousarray(np.tile(host_x, (-(-B // len(host_x)), 1))[:B])
        x = torch.from_numpy(host_x).to(dev)
        out = torch.empty_like(x)
        meter = loudness.LoudnessMeter(RATE, max_rows=B, max_samples=n)
        hops = n // hop
        n_fft = nice(n + args.pad)
        resp = k_response(n_fft) if ta_lfilter is None else None
        a_co = torch.tensor([[1.0, c[3], c[4]] for c in coef], dtype=torch.float64, device=dev)
        b_co = torch.tensor([[c[0], c[1], c[2]] for c in coef], dtype=torch.float64, device=dev)

        def host_gains():
            h = x.cpu().numpy().astype(np.float64)
            for b0, b1, b2, a1, a2 in coef:
                h = lfilter([b0, b1, b2], [1.0, a1, a2], h, axis=1)
            e = (h[:, :hops * hop] ** 2).reshape(B, hops, hop).sum(2)
            z = (e[:, :-3] + e[:, 1:-2] + e[:, 2:-1] + e[:, 3:]) / block
            L = gate(z)
            g = torch.from_numpy((10.0 ** ((-16.0 - L) / 20.0)).astype(np.float32)).to(dev)
            return L, g

        def torch_stats():
            if ta_lfilter is not None:
                y = x.to(torch.float64)
                for i in range(2):
                    y = ta_lfilter(y, a_co[i], b_co[i], clamp=False)
            else:
                y = torch.fft.irfft(torch.fft.rfft(x.to(torch.float64), n_fft) * resp, n_fft)[:, :n]
            e = y[:, :hops * hop].reshape(B, hops, hop).square().sum(2)
            z = e.unfold(1, 4, 1).sum(2) / block
            l = -0.691 + 10.0 * torch.log10(z)
            a = l > -70.0
            gamma = -0.691 + 10.0 * torch.log10((z * a).sum(1) / a.sum(1)) - 10.0
            r = a & (l > gamma[:, None])
            L = -0.691 + 10.0 * torch.log10((z * r).sum(1) / r.sum(1))
            tp = torch.nn.functional.conv1d(x[:, None, :], tab, padding=zc).abs().amax(dim=(1, 2))
            g_db = torch.minimum(-16.0 - L, -1.5 - 20.0 * torch.log10(tp.to(torch.float64)))
            return L, tp, torch.pow(10.0, g_db / 20.0).to(torch.float32)

        routes = {
            "measure": {"device": lambda: meter.measure(x), "host": lambda: host_gains(), "torch": lambda: torch_stats()},
            "normalize": {"device": lambda: meter.normalize(x, out=out), "host": lambda: torch.mul(x, host_gains()[1][:, None], out=out),
                          "torch": lambda: torch.mul(x, torch_stats()[2][:, None], out=out)},
        }
        # the routes agree before they are timed
        stats, counts = meter.measure(x)
        L_dev = stats[:, 0].cpu().numpy()
        L_host, L_torch = host_gains()[0], torch_stats()[0].cpu().numpy()
        tp_err = float((torch_stats()[1].to(torch.float64) - stats[:, 1]).abs().max())
        say()
        say(f"{name}: {B} x {n} float32 at {RATE} Hz ({B * n * 4 / 1e6:.1f} MB); blocks per row {int(counts[0, 0])}; loudness {L_dev.min():.2f} .. {L_dev.max():.2f} LUFS")
        say(f"  host  route: max |L - device| = {np.abs(L_host - L_dev).max():.3e} LU")
        say(f"  torch route: max |L - device| = {np.abs(L_torch - L_dev).max():.3e} LU; max |true peak - device| = {tp_err:.3e}")
        assert np.abs(L_host - L_dev).max() <= 1e-6, "the host route and the device disagree"

        def window(fn, reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / 1e3 / reps

        def host_window(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t

        for what, by in routes.items():
            times = {r: [] for r in by}
            for r, fn in by.items():                     # warm-up of every route
                fn()
                if r != "host":
                    window(fn, 3)
            for _ in range(args.windows):
                for r, fn in by.items():                 # the routes alternate
                    times[r].append(host_window(fn) if r == "host" else window(fn, args.reps))
            med = {r: statistics.median(ts) for r, ts in times.items()}
            for r, ts in times.items():
                say(f"  {what:9s} {r:6s} median {med[r] * 1e3:10.3f} ms   min {min(ts) * 1e3:10.3f}   max {max(ts) * 1e3:10.3f}   (windows {len(ts)}"
                    f"{'' if r == 'host' else f' of {args.reps} calls'})   {med[r] / med['device']:8.1f} x device")
            if what == "measure":
                tbs = B * n * 4 / med["device"] / 1e12
                say(f"  measure   device: {tbs:.3f} TB/s of input read once, {100.0 * tbs / COPY_TBS:.1f} % of the {COPY_TBS} TB/s streaming rate")
            for r in by:
                if r != "device" and med[r] < med["device"]:
                    say(f"  LOSS: the device route is slower than the {r} route on {name} {what}")
        meter.close()
        del x, out
        torch.cuda.empty_cache()

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
