"""The mfcc features of a batch of clips (multilingual_kws_amd/spectral.py) against the same pipeline composed from
torch operators on the same device.  One process, one MI355X, audio resident on the device.

  (a) torch      frames (unfold) x periodic Hann -> torch.fft.rfft(n = fft size) -> re^2 + im^2 -> sqrt -> matmul with the dense
                 [bins, channels] filterbank -> log(clamp(1e-12)) -> matmul with the DCT; every table built by tests/spectral_cases.py
  (b) the kernel SpectralFrontend.forward, one launch

Both are checked against the float64 reference (tests/spectral_cases.py) on the first clips before anything is timed: the kernel at
T_FEAT, the composition at 10 x T_FEAT (its sums run in another order, through a dense filterbank).  Then warm-up and
device-synchronised windows of --calls calls each, the two alternating in the same process, --windows windows of each: the medians, the
spread (min .. max of the windows) and the ratio of the medians.  For orientation: the micro frontend on the same batch, and the HBM
floor -- 64 000 B of audio in and 49 x 40 x 4 = 7 840 B of features out per clip, 71 840 B -- as a share of the kernel's time at the
8.0 TB/s peak and at the 6.29 TB/s a copy reaches.

  python tools/bench_spectral.py [--clips 1024] [--calls 50] [--windows 9] [--out profiles/spectral_bench.txt]"""
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

PEAK_TBS, COPY_TBS = 8.0, 6.29


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=50, help="calls per synchronised window (at least 50)")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls must be at least 50")

    import torch
    from multilingual_kws_amd import synth
    from multilingual_kws_amd.frontend import Frontend
    from multilingual_kws_amd.spectral import SpectralFrontend
    from tests import spectral_cases as sc
    assert torch.cuda.is_available(), "bench_spectral.py measures on a GPU; there is nothing to report without one"
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

    say(f"# tools/bench_spectral.py  commit {commit}  device {torch.cuda.get_device_properties(dev).name}  torch {torch.__version__}")
    B, n, window, stride, fft, C, F = args.clips, 16000, 480, 320, 512, 40, 40
    cfg = sc.cfg_of("w480", "mfcc40")
    audio_np = synth.clips_float32(B, n)
    audio = torch.from_numpy(audio_np).to(dev)

    # (a) the torch composition
    weights, band, start, end = sc.mel_tables(fft // 2 + 1, 16000, C, 20.0, 4000.0)
    fb = np.zeros((fft // 2 + 1, C))
    for i in range(start, end + 1):
        if band[i] >= 0:
            fb[i, band[i]] += weights[i]
        if band[i] + 1 < C:
            fb[i, band[i] + 1] += 1.0 - weights[i]
    t_win = torch.from_numpy(sc.hann_periodic(window).astype(np.float32)).to(dev)
    t_fb = torch.from_numpy(fb.astype(np.float32)).to(dev)
    t_dct = torch.from_numpy(sc.dct_matrix(F, C).T.astype(np.float32).copy()).to(dev)

    def torch_mfcc(x):
        z = torch.fft.rfft(x.unfold(1, window, stride) * t_win, n=fft)
        mag = torch.sqrt(z.real * z.real + z.imag * z.imag)
        return torch.log(torch.clamp(mag @ t_fb, min=1e-12)) @ t_dct

    # (b) the kernel, and the micro frontend for orientation
    fe = SpectralFrontend(max_samples=n, **cfg)
    micro = Frontend(max_samples=n)
    out = torch.empty((B, 49, F), dtype=torch.float32, device=dev)
    micro_out = torch.empty((B, 49, 40), dtype=torch.float32, device=dev)
    routes = {"torch composition": lambda: torch_mfcc(audio), "spectral kernel": lambda: fe.forward(audio, out=out),
              "micro frontend": lambda: micro.forward(audio, out=micro_out)}

    k = min(B, 8)
    want = sc.reference(cfg, audio_np[:k])["feat"]
    e_kernel = sc.abs_err(fe.forward(audio[:k]).cpu().numpy(), want)
    e_torch = sc.abs_err(torch_mfcc(audio[:k]).cpu().numpy(), want)
    say(f"against float64 on {k} clips: kernel {e_kernel:.3e} (T_FEAT {sc.T_FEAT}), torch composition {e_torch:.3e}")
    assert e_kernel <= sc.T_FEAT and e_torch <= 10 * sc.T_FEAT, "a route differs from the float64 reference: nothing is timed"

    def window_us(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.calls * 1e6

    for fn in routes.values():                # warm-up: code objects, rocFFT plans, the allocator's blocks
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(args.windows):             # the routes alternate, window by window
        for name, fn in routes.items():
            times[name].append(window_us(fn))
    say(f"{B} clips x {n} samples -> mfcc 49 x {F}; {args.windows} windows of {args.calls} calls each, alternating; us per call")
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        say(f"  {name:18s} median {med[name]:9.2f}   min {min(ts):9.2f}   max {max(ts):9.2f}")
    ratio = med["torch composition"] / med["spectral kernel"]
    say(f"spectral kernel vs torch composition: {ratio:.2f}x (medians); {'PASS' if ratio > 1.0 else 'MISS'}: the kernel is "
        f"{'faster' if ratio > 1.0 else 'not faster'} than the composition")
    floor_bytes = B * (n * 4 + 49 * F * 4)
    for tbs, what in ((PEAK_TBS, "peak"), (COPY_TBS, "what a copy reaches")):
        floor_us = floor_bytes / (tbs * 1e12) * 1e6
        say(f"HBM floor {floor_bytes / B:.0f} B per clip = {floor_us:.2f} us at {tbs} TB/s ({what}): {100 * floor_us / med['spectral kernel']:.1f} % of the kernel's call")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    fe.close()
    micro.close()


if __name__ == "__main__":
    main()
