"""Side-by-side few-shot fine-tuning (transfer_learning.FrozenHeadGroupTrainer / head.HeadGroup) against the one-keyword-at-a-time path
(K FrozenHeadTrainers run one after the other in the same process, on the same draws), frozen phase only, on one GPU.

Per K: aggregate clips/s and milliseconds per round of K optimizer steps of both paths (median of --repeats timed runs, with the
min..max of the runs; each run is synchronised at both ends and follows --warmup untimed groups), the hipEvent time of one round's
head launches (HeadGroup.loss_grad + adam_step against K single-head steps) and the host time to enqueue them.

    python tools/bench_finetune_many.py [--batch 64] [--group 48] [--ks 1,2,4,8,16,32] [--repeats 5]      (profiles/finetune_many.txt)"""
import argparse
import math
import os
import statistics
import sys
import tempfile
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multilingual_kws_amd import parallel, synth, weights
from multilingual_kws_amd.embedding import input_data, transfer_learning as tl
from multilingual_kws_amd.embedding_model import EmbeddingModel
from multilingual_kws_amd.head import Head, glorot_uniform_params

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--group", type=int, default=None, help="optimizer steps per forward pass (default: FORWARD_CLIPS // batch)")
ap.add_argument("--ks", default="1,2,4,8,16,32")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2, help="untimed groups before the timed runs of a leg")
ap.add_argument("--clips", type=int, default=800000, help="clips per timed run, rounded up to whole groups of all K heads")
args = ap.parse_args()
B = args.batch
G = args.group or tl.steps_per_forward(B)
KS = [int(k) for k in args.ks.split(",")]
LR = 1e-3
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
em = EmbeddingModel(weights.synthetic_blob(), max_batch=max(B * G, 64), device=dev)
data = synth.write_fewshot_dataset(tempfile.mkdtemp(prefix="mkws_ftm_"))
ms = input_data.standard_microspeech_model_settings(3)
donor = None


def streams(K):
    """K endless training streams with seeds 0 .. K-1 (every leg draws the same batches)."""
    global donor
    out = []
    for i in range(K):
        ds = input_data.AudioDataset(ms, ["target"], data["bg_dir"], data["unknown"], unknown_percentage=50.0,
                                     spec_aug_params=input_data.SpecAugParams(percentage=80), seed=i)
        if donor is None:
            donor = ds
        else:
            ds.share_banks(donor)
        out.append(ds.init_single_target(input_data.AUTOTUNE, data["train"], is_training=True).shuffle(1000).repeat().batch(B))
    return out


def heads(K):
    return [Head(1024, 18, 3, max_batch=max(B, 64), params=glorot_uniform_params(seed=i), device=dev) for i in range(K)]


def timed(legs, n_groups):
    """-> one [seconds] list per leg: args.repeats synchronised runs of n_groups groups each, the legs ALTERNATING run by run (what disturbs
    one disturbs the other), after args.warmup untimed groups of each."""
    for run_groups in legs:
        run_groups(args.warmup)
    torch.cuda.synchronize()
    out = [[] for _ in legs]
    for _ in range(args.repeats):
        for secs, run_groups in zip(out, legs):
            t0 = time.perf_counter()
            run_groups(n_groups)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
    return out


def describe(secs, clips, rounds):
    rates = sorted(clips / s for s in secs)
    med = statistics.median(rates)
    return med, (rates[-1] - rates[0]) / med, f"{med:9.0f} clips/s ({rates[0]:.0f}..{rates[-1]:.0f}), {statistics.median(secs) / rounds * 1e3:.4f} ms per round"


def ev(fn, reps=50):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host(fn, reps=200):
    """Host time of fn() while the GPU runs behind (no synchronisation inside the loop)."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t = (time.perf_counter() - t0) / reps
    torch.cuda.synchronize()
    return t * 1e3


print(f"# {torch.cuda.get_device_name(0)}; {B} clips per optimizer step, {G} steps per forward pass ({B * G} clips); frozen phase; second stream "
      f"{'on' if G >= tl.OVERLAP_FROM_GROUP else 'off'}; medians of {args.repeats} alternating runs of >= {args.clips} clips (min..max of the runs), {args.warmup} warm-up groups")
print("# sequential = K FrozenHeadTrainers one after the other (the path before transfer_learn_many); side by side = FrozenHeadGroupTrainer")
table = []
for K in KS:
    n_groups = max(2, math.ceil(args.clips / (K * G * B)))          # groups of every head per timed run
    clips, rounds = n_groups * K * G * B, n_groups * G
    # sequential: head after head, each through n_groups groups
    hs = heads(K)
    trainers = [tl.FrozenHeadTrainer(em, h, d, B, LR, group=G) for h, d in zip(hs, streams(K))]

    def sequential(n):
        for t in trainers:
            for _ in range(n * G):
                t.step()
            t.finish()
    # side by side
    hg = heads(K)
    many = tl.FrozenHeadGroupTrainer(em, hg, streams(K), B, LR, group=G)

    def side_by_side(n):
        for _ in range(n * G):
            many.step()
        many.finish()
    t_seq, t_sbs = timed([sequential, side_by_side], n_groups)
    seq, sbs = describe(t_seq, clips, rounds), describe(t_sbs, clips, rounds)
    # one round's head launches alone, on rows that stay put
    emb = torch.randn((K, B, 1024), device=dev) * 0.3
    lab = torch.randint(0, 3, (K, B), device=dev, dtype=torch.int32)
    group = many.group

    def round_group():
        group.loss_grad(emb, lab, rows=B)
        group.adam_step(lr=LR)

    def round_single():
        for k in range(K):
            parallel.dp_step(hs[k], emb[k], lab[k], lr=LR)
    dev_g, dev_s, host_g, host_s = ev(round_group), ev(round_single), host(round_group), host(round_single)
    print(f"B={B} G={G} K={K:2d}: side by side {sbs[2]} | sequential {seq[2]} | ratio {sbs[0] / seq[0]:.3f} | head launches of one round (hipEvent) "
          f"{dev_g:.4f} ms vs {dev_s:.4f} ms | host enqueue of one round {host_g:.4f} ms vs {host_s:.4f} ms")
    table.append((K, sbs[0], sbs[1], seq[0], seq[1]))
    many.close()
    for h in hs + hg:
        h.close()

spread = max(max(t[2], t[4]) for t in table)
best = max(table, key=lambda t: t[1])
pick = table[-1][0]
for i, t in enumerate(table):
    if all(u[1] <= t[1] * (1 + spread) for u in table[i + 1:]):
        pick = t[0]
        break
seq_ref = statistics.median(t[3] for t in table)
print(f"# largest run-to-run spread (max - min) / median over all legs: {spread * 100:.1f} %")
print(f"# best K = {best[0]}: {best[1]:.0f} clips/s side by side against {best[3]:.0f} sequential ({best[1] / best[3]:.3f}x; "
      f"{'above' if best[1] > best[3] * (1 + spread) else 'NOT above'} the spread); median sequential rate over K {seq_ref:.0f}")
print(f"# smallest K after which the side-by-side rate rises by no more than the spread: {pick}")
