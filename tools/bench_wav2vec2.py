"""The wav2vec 2.0 baseline's forward pass (multilingual_kws_amd/wav2vec2.py, mkws_w2v2_forward) at the base
configuration on synthetic weights: the device chain against the route a user has without it -- wav2vec2.reference_forward, the same
network in plain torch operators, in float32 on the same device -- measured in the same run.  One process, one MI355X.

Both routes start from the audio in device memory and end with the last hidden state and the pooled embedding in device memory.
Agreement with the float64 specification (CPU) is measured before anything is timed and printed next to the float32 CPU reference's
own error E32.  A timed window is `--inner` calls between two device events; the routes alternate, after warm-up at every batch
size; medians and extremes of `--reps` windows are reported.  The stage table times the chain stopped after a stage (mkws_w2v2_tap)
and reports the differences.  No threshold: the numbers are the result, whichever route they favour.

  python tools/bench_wav2vec2.py [--batches 1 32] [--reps 9] [--inner 5] [--out profiles/wav2vec2_bench.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def flop_per_clip(c, n=16000):
    """Multiply-adds * 2 of the contractions (convolutions, projections, attention products, FFN); norms and activations are noise."""
    from multilingual_kws_amd import wav2vec2
    t, cin, total = n, 1, 0
    for i in range(7):
        t = (t - wav2vec2.CONV_KERNEL[i]) // wav2vec2.CONV_STRIDE[i] + 1
        total += 2 * t * wav2vec2.CONV_KERNEL[i] * cin * c.conv_dim[i]
        cin = c.conv_dim[i]
    H, I, T = c.hidden_size, c.intermediate_size, t
    total += 2 * T * cin * H + 2 * T * H * (H // c.num_conv_pos_embedding_groups) * c.num_conv_pos_embeddings
    total += c.num_hidden_layers * (2 * T * H * 4 * H + 4 * T * T * H + 4 * T * H * I)
    return total


def windows(fn, reps, inner):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from multilingual_kws_amd import wav2vec2
    if not torch.cuda.is_available():
        sys.exit("bench_wav2vec2: no GPU (there is no CPU fallback and no CPU timing)")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    config = wav2vec2.Config.base()
    blob = wav2vec2.synthetic_weights(config, 1234)
    flop = flop_per_clip(config)
    say(f"wav2vec 2.0 base, synthetic weights (seed 1234), 16000 samples -> 49 frames; {flop / 1e9:.2f} GFLOP per clip in the contractions")
    say(f"device: {torch.cuda.get_device_name()}")
    rng = np.random.default_rng(5)
    t = np.arange(16000) / 16000.0
    model = wav2vec2.Wav2Vec2(config, blob, max_batch=max(args.batches))
    layers = config.num_hidden_layers
    weights32 = wav2vec2.reference_weights(config, blob, "cuda", torch.float32)      # the torch route keeps its weights on the device, as the handle does

    # accuracy first: two clips against float64 on the CPU
    audio2 = (0.3 * np.sin(2 * np.pi * rng.uniform(100, 3000, (2, 1)) * t) + 0.1 * rng.standard_normal((2, 16000)) + 0.05).astype(np.float32)
    r64 = wav2vec2.reference_forward(config, blob, audio2, taps=True, dtype=torch.float64)
    r32 = wav2vec2.reference_forward(config, blob, audio2, taps=True, dtype=torch.float32)
    x2 = torch.from_numpy(audio2).cuda()
    rel = lambda got, want: float((got.double().cpu() - want).abs().max() / want.abs().max())
    hidden, embed = model.forward_embed(x2)
    t32 = wav2vec2.reference_forward(config, None, x2, dtype=torch.float32, weights=weights32)
    say()
    say("error against the float64 specification (CPU), relative to max |float64|, B = 2:")
    say(f"  last hidden state   device chain {rel(hidden, r64.last_hidden_state):.3e}   torch float32 on the device {rel(t32.last_hidden_state, r64.last_hidden_state):.3e}"
        f"   E32 (torch float32, CPU) {rel(r32.last_hidden_state, r64.last_hidden_state):.3e}")
    say(f"  embedding           device chain {rel(embed, r64.embedding):.3e}   torch float32 on the device {rel(t32.embedding, r64.embedding):.3e}"
        f"   E32 {rel(r32.embedding, r64.embedding):.3e}")
    say("  per stage (mkws_w2v2_tap): stage, device chain, E32")
    for stage in range(10 + layers):
        say(f"    {stage:2d}  {rel(model.tap(x2, stage), r64.taps[stage]):.3e}  {rel(r32.taps[stage], r64.taps[stage]):.3e}")

    for B in args.batches:
        audio = (0.3 * np.sin(2 * np.pi * rng.uniform(100, 3000, (B, 1)) * t) + 0.1 * rng.standard_normal((B, 16000)) + 0.05).astype(np.float32)
        x = torch.from_numpy(audio).cuda()
        dev_route = lambda: model.forward_embed(x)
        with torch.no_grad():
            torch_route = lambda: wav2vec2.reference_forward(config, None, x, dtype=torch.float32, weights=weights32)
            for _ in range(3):
                dev_route()
                torch_route()
            torch.cuda.synchronize()
            dev_ms, torch_ms = [], []
            for _ in range(args.reps):
                dev_ms += windows(dev_route, 1, args.inner)
                torch_ms += windows(torch_route, 1, args.inner)
        say()
        say(f"batch {B}: ms per forward, median [min, max] of {args.reps} windows of {args.inner} calls, routes alternating")
        for name, ms in (("device chain (mkws_w2v2_forward)", dev_ms), ("torch operators, float32, same device", torch_ms)):
            med = statistics.median(ms)
            say(f"  {name:40s} {med:9.3f} [{min(ms):.3f}, {max(ms):.3f}]   {B / med * 1e3:9.1f} clips/s   {B * flop / med / 1e9:8.2f} TFLOP/s")
        say(f"  stages of the device chain (time of the chain stopped after the stage, and the difference to the row above):")
        prev = 0.0
        for label, stage in (("0 normalise", 0), ("1 conv 0 + GroupNorm + GELU", 1), ("2-7 conv 1..6 (GEMM + GELU)", 7), ("8 LayerNorm + projection", 8),
                             ("9 positional conv + LayerNorm", 9), (f"10-{9 + layers} transformer layers", 9 + layers)):
            fn = lambda: model.tap(x, stage)
            fn()
            torch.cuda.synchronize()
            med = statistics.median(windows(fn, args.reps, args.inner))
            say(f"    {label:36s} {med:9.3f} ms   +{med - prev:8.3f}")
            prev = med
    model.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
