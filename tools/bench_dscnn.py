"""The DS-CNN baseline's forward pass (multilingual_kws_amd/dscnn.py, mkws_dscnn_forward): the one-launch kernel
against the route a user has without it -- the same network written with torch.nn.functional ops (conv2d on folded weights, relu,
avg_pool2d, linear, softmax) on the same device -- measured in the same run.  One process, one MI355X.

Both routes start from the spectrograms in device memory and end with the probabilities in device memory.  Agreement with the float64 specification is asserted before
anything is timed (the kernel within 1e-5, the torch route within 1e-3) and printed.  A timed window is `--inner` calls between two device
events; the routes alternate, after warm-up at every batch size; medians and extremes of `--reps` windows are reported.  No threshold:
the numbers are the result, whichever route they favour.

  python tools/bench_dscnn.py [--batches 1024 1] [--reps 15] [--inner 20] [--commit HASH] [--out profiles/dscnn.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLOP_PER_CLIP = 2 * 500 * 64 * (40 + 4 * (9 + 64))          # stem + four depthwise / pointwise blocks; pool and dense are noise


def torch_route(folded, device):
    """The network with torch.nn.functional on the folded float32 weights -> callable(spec [B,49,40]) -> probabilities."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    stem_w, stem_b = t(folded["stem_w"].reshape(10, 4, 1, 64).transpose(3, 2, 0, 1)), t(folded["stem_b"])
    dw = [(t(w.reshape(3, 3, 64, 1).transpose(2, 3, 0, 1)), t(b)) for w, b in zip(folded["dw_w"], folded["dw_b"])]
    pw = [(t(w.reshape(1, 1, 64, 64).transpose(3, 2, 0, 1)), t(b)) for w, b in zip(folded["pw_w"], folded["pw_b"])]
    dense_w, dense_b = t(folded["dense_w"].T), t(folded["dense_b"])

    def run(spec):
        x = F.relu(F.conv2d(F.pad(spec[:, None], (1, 1, 4, 5)), stem_w, stem_b, stride=2))
        for (dww, dwb), (pww, pwb) in zip(dw, pw):
            x = F.relu(F.conv2d(x, dww, dwb, padding=1, groups=64))
            x = F.relu(F.conv2d(x, pww, pwb))
        return torch.softmax(F.linear(F.avg_pool2d(x, (24, 20)).flatten(1), dense_w, dense_b), dim=1)
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 1])
    ap.add_argument("--labels", type=int, default=12)
    ap.add_argument("--reps", type=int, default=15, help="timed windows per route and batch size")
    ap.add_argument("--inner", type=int, default=20, help="forward calls per timed window")
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import torch
    from multilingual_kws_amd import dscnn
    assert torch.cuda.is_available(), "bench_dscnn.py measures on a GPU; there is nothing to report without one"
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

    params = dscnn.synthetic_params(args.labels)
    model = dscnn.DSCNN(params, max_batch=max(args.batches), device=dev)
    other = torch_route(dscnn.fold(params), dev)
    say(f"DS-CNN forward, {args.labels} labels, {torch.cuda.get_device_name(dev)}, commit {commit}: mkws_dscnn_forward (one launch, grid <= {model.grid}) against torch.nn.functional")
    say(f"  a window = {args.inner} calls between two device events; {args.reps} windows per route, alternating; per-call times")

    def window(fn, x):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn(x)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.inner

    for B in args.batches:
        x_np = dscnn.structured_clips(min(B, 64), 4321)
        x_np = np.concatenate([x_np] * ((B + 63) // 64))[:B]
        x = torch.from_numpy(x_np).to(dev)
        want = dscnn.dscnn_host(x_np[:64], params)
        for name, fn in (("device kernel", model.forward), ("torch ops", other)):
            got = fn(x).cpu().numpy()[:64].astype(np.float64)
            err = np.abs(got - dscnn.softmax_host(want)).max()
            say(f"  batch {B:5d}   {name:13s}  max |probability - float64 specification| = {err:.2e}")
            assert err <= (1e-5 if fn is not other else 1e-3) * max(1.0, np.abs(want).max()), (name, B, err)
        for _ in range(3):
            window(model.forward, x), window(other, x)
        ours, theirs = [], []
        for _ in range(args.reps):
            ours.append(window(model.forward, x))
            theirs.append(window(other, x))
        mo, mt = statistics.median(ours), statistics.median(theirs)
        say(f"  batch {B:5d}   device kernel  median {mo:8.4f} ms  (min {min(ours):.4f}, max {max(ours):.4f})   {B / mo * 1e3:12.0f} clips/s   {B * FLOP_PER_CLIP / mo * 1e-9:7.2f} TFLOP/s of the network's {FLOP_PER_CLIP * 1e-6:.1f} MFLOP per clip")
        say(f"  batch {B:5d}   torch ops      median {mt:8.4f} ms  (min {min(theirs):.4f}, max {max(theirs):.4f})   {B / mt * 1e3:12.0f} clips/s")
        say(f"  batch {B:5d}   torch ops / device kernel = {mt / mo:.2f}")
    model.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
