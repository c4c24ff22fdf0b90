"""One optimizer step of the DS-CNN baseline (multilingual_kws_amd/dscnn_trainer.py) -- training-mode forward
with dropout, cross-entropy, backward, L2, Adam -- host-driven ("eager") and as one hipGraph replay ("hipgraph"), against the route a
user has without it: the same network as torch.nn modules in .train() with autograd and torch.optim.Adam on the same device, measured
in the same run.  One process, one MI355X.

All routes start from the spectrograms and labels in device memory.  Before anything is timed, the gradients of one step without dropout
(the two routes draw different masks) are compared and the largest difference is asserted below 2e-2 of each tensor's largest entry: a
check that both routes compute the same step (a float32 route lands single ReLU cells on the other side of zero, which moves a
gradient by up to ~1e-2 of its largest entry; the float64 comparison is tests/test_dscnn_train_gpu.py's).  A timed window is `--inner`
steps between two device events; the routes alternate, after warm-up at every batch size; medians and extremes of `--reps` windows are
reported.  No threshold: the numbers are the result, whichever route they favour.

  python tools/bench_dscnn_train.py [--batches 100 1024] [--reps 15] [--inner 10] [--commit HASH] [--out profiles/dscnn_train.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLOP_PER_CLIP = 3 * 2 * 500 * 64 * (40 + 4 * (9 + 64))      # forward + input gradient + weight gradient of the nine convolutions
LR, WEIGHT_DECAY = 5e-4, 1e-4


def torch_route(params, label_count, rates, device):
    """The network as torch.nn modules holding `params` -> (module, {Keras name: torch parameter}, the nine convolution weights)."""
    import torch
    from multilingual_kws_amd import dscnn, dscnn_trainer
    nn = torch.nn

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.convs, self.bns = nn.ModuleList(), nn.ModuleList()
            for kind, _, _, _ in dscnn_trainer.LAYERS:
                self.convs.append(nn.Conv2d(1, 64, (10, 4), stride=2) if kind == "stem" else
                                  nn.Conv2d(64, 64, 3, padding=1, groups=64) if kind == "dw" else nn.Conv2d(64, 64, 1))
                self.bns.append(nn.BatchNorm2d(64, eps=1e-3, momentum=0.01))
            self.drop0, self.drop1 = nn.Dropout(rates[0]), nn.Dropout(rates[1])
            self.dense = nn.Linear(64, label_count)

        def forward(self, spec):
            x = torch.nn.functional.pad(spec[:, None], (1, 1, 4, 5))
            for i, (conv, bn) in enumerate(zip(self.convs, self.bns)):
                x = torch.relu(bn(conv(x)))
                if i == 0:
                    x = self.drop0(x)
            return self.dense(self.drop1(x)[:, :, :24].mean(dim=(2, 3)))

    net = Net().to(device).train()
    t, named = dscnn.unpack(params), {}
    with torch.no_grad():
        for i, (kind, kernel, bias, bn) in enumerate(dscnn_trainer.LAYERS):
            w = torch.from_numpy(t[kernel].copy())
            net.convs[i].weight.copy_(w.permute(2, 3, 0, 1) if kind == "dw" else w.permute(3, 2, 0, 1))
            net.convs[i].bias.copy_(torch.from_numpy(t[bias].copy()))
            net.bns[i].weight.copy_(torch.from_numpy(t[bn + "/gamma"].copy()))
            net.bns[i].bias.copy_(torch.from_numpy(t[bn + "/beta"].copy()))
            net.bns[i].running_mean.copy_(torch.from_numpy(t[bn + "/moving_mean"].copy()))
            net.bns[i].running_var.copy_(torch.from_numpy(t[bn + "/moving_variance"].copy()))
            named[kernel] = (net.convs[i].weight, (2, 3, 0, 1) if kind == "dw" else (2, 3, 1, 0))
            named[bn + "/gamma"], named[bn + "/beta"] = (net.bns[i].weight, None), (net.bns[i].bias, None)
        net.dense.weight.copy_(torch.from_numpy(t["dense/kernel"].T.copy()))
        net.dense.bias.copy_(torch.from_numpy(t["dense/bias"].copy()))
        named["dense/kernel"], named["dense/bias"] = (net.dense.weight, (1, 0)), (net.dense.bias, None)
    return net, named, [c.weight for c in net.convs]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[100, 1024])
    ap.add_argument("--labels", type=int, default=12)
    ap.add_argument("--reps", type=int, default=15, help="timed windows per route and batch size")
    ap.add_argument("--inner", type=int, default=10, help="optimizer steps per timed window")
    ap.add_argument("--commit", default=None, help="what to stamp the output with (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if args.reps < 15:
        ap.error("--reps must be at least 15")

    import torch
    from multilingual_kws_amd import dscnn, dscnn_trainer
    assert torch.cuda.is_available(), "bench_dscnn_train.py measures on a GPU; there is nothing to report without one"
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
    say(f"DS-CNN optimizer step, {args.labels} labels, {torch.cuda.get_device_name(dev)}, commit {commit}: DSCNNTrainer.step (eager, hipgraph) against torch.nn + autograd + torch.optim.Adam")
    say(f"  a window = {args.inner} steps between two device events; {args.reps} windows per route, alternating; per-step times")

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.inner

    for B in args.batches:
        x_np = dscnn.structured_clips(min(B, 64), 4321)
        x_np = np.concatenate([x_np] * ((B + 63) // 64))[:B]
        x = torch.from_numpy(x_np).to(dev)
        y = torch.from_numpy(((np.arange(B) * 5 + 1) % args.labels).astype(np.int32)).to(dev)
        y64 = y.to(torch.int64)
        # ---- the same step on both routes, without dropout
        tr = dscnn_trainer.DSCNNTrainer(params, max_batch=B, weight_decay=WEIGHT_DECAY, dropout=(0.0, 0.0), device=dev)
        stats = tr.forward_backward(x, y).cpu().tolist()
        net, named, kernels = torch_route(params, args.labels, (0.0, 0.0), dev)
        loss = torch.nn.functional.cross_entropy(net(x), y64)
        (loss + WEIGHT_DECAY * sum((w ** 2).sum() for w in kernels)).backward()
        worst, grads = 0.0, tr.named_grads()
        for name, (p, perm) in named.items():
            theirs = (p.grad.permute(*perm) if perm else p.grad).cpu().numpy().reshape(grads[name].shape).astype(np.float64)
            worst = max(worst, float(np.abs(grads[name] - theirs).max() / np.abs(theirs).max()))
        loss = loss.detach()
        say(f"  batch {B:5d}   loss {stats[0] / B:.6f} (torch {float(loss):.6f}); largest gradient difference / largest entry of its tensor = {worst:.2e}")
        assert worst <= 2e-2 and abs(stats[0] / B - float(loss)) <= 1e-4 * abs(float(loss)), (B, worst, stats, float(loss))
        del tr, net
        # ---- the timed routes
        eager = dscnn_trainer.DSCNNTrainer(params, max_batch=B, weight_decay=WEIGHT_DECAY, device=dev)
        graph = dscnn_trainer.DSCNNTrainer(params, max_batch=B, weight_decay=WEIGHT_DECAY, device=dev, mode="hipgraph")
        net, _, kernels = torch_route(params, args.labels, (0.2, 0.4), dev)
        opt = torch.optim.Adam(net.parameters(), lr=LR, eps=1e-7)

        def torch_step():
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(net(x), y64) + WEIGHT_DECAY * sum((w ** 2).sum() for w in kernels)
            loss.backward()
            opt.step()
        routes = [("device eager", lambda: eager.step(x, y, LR)), ("device hipgraph", lambda: graph.step(x, y, LR)), ("torch autograd", torch_step)]
        for _ in range(3):
            for _, fn in routes:
                window(fn)
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, fn in routes:
                times[name].append(window(fn))
        med = {name: statistics.median(v) for name, v in times.items()}
        for name, v in times.items():
            say(f"  batch {B:5d}   {name:15s}  median {med[name]:8.4f} ms  (min {min(v):.4f}, max {max(v):.4f})   {B / med[name] * 1e3:10.0f} clips/s   "
                f"{B * FLOP_PER_CLIP / med[name] * 1e-9:6.2f} TFLOP/s of the step's {FLOP_PER_CLIP * 1e-6:.1f} MFLOP per clip")
        say(f"  batch {B:5d}   torch autograd / device eager = {med['torch autograd'] / med['device eager']:.2f},  torch autograd / device hipgraph = "
            f"{med['torch autograd'] / med['device hipgraph']:.2f}")
        del eager, graph, net, opt
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
