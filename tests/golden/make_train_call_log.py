#!/usr/bin/env python3
"""Writes tests/golden/train_call_log.json: the sequence of library calls (symbol, arguments) one optimizer step of every trainer over the
mkws_op_* operators makes -- EmbeddingTrainer (default switches, four switch variants, the keep-scales form), DSCNNTrainer (eager, with and
without weight decay) and LogitsLayer -- recorded with embedding_trainer._CallTape in place of the trainer's `.L`.

Run it on the commit whose launch sequence tests/test_train_call_log_gpu.py is to pin (needs a GPU): a refactor of the host code above the
operators must hand the library the same calls with the same arguments.  Only public constructors and `.L` are used, so the file runs on
either side of such a change.  Everything is at batch 2, inside a non-default stream (its handle is neither NULL nor a buffer address).

Arguments are normalised: ints as they are; ctypes integers by .value; Python floats as float.hex(); NULL as None; a stream handle as "main"
or "side"; a pointer into the trainer's params / grads / m / v / d_step / stats or into the main / side arena as "<buffer>+<float offset>";
any other pointer as "buf" (activation addresses follow the allocator; their dataflow is the numerical tests' business).  The one rewrite:
mkws_op_bn_train_fwd(...) is logged as the mkws_op_bn_train_fwd_res(..., None, None, 1, stream) the library defines it as.

Stored: the full logs of the three default cases, a SHA-256 of the log of every other case."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "train_call_log.json")
B, LABELS, LR = 2, 3, 1e-3
FULL = ("embedding", "dscnn", "logits")                  # cases stored call by call; the others as a hash


def _normalise(log, streams, buffers):
    """[(ctypes function, arguments)] -> [[symbol, [normalised arguments]]]; buffers: {name: tensor}, streams: {handle: name}."""
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name) for name, t in buffers.items() if t is not None]

    def one(a):
        if a is None or isinstance(a, int):
            return a
        if isinstance(a, float):
            return float(a).hex()
        if isinstance(a, ctypes.c_void_p):
            if a.value is None:
                return None
            if a.value in streams:
                return streams[a.value]
            for lo, hi, name in spans:
                if lo <= a.value < hi:
                    return f"{name}+{(a.value - lo) // 4}"
            return "buf"
        if hasattr(a, "value"):
            return one(a.value)
        return "buf"                                     # ctypes.byref(...) of a host object

    out = []
    for f, args in log:
        name, args = f.__name__, [one(a) for a in args]
        if name == "mkws_op_bn_train_fwd":
            name, args = "mkws_op_bn_train_fwd_res", args[:-1] + [None, None, 1] + args[-1:]
        out.append([name, args])
    return out


def _record(obj, body, buffers):
    """Runs body() with obj.L logging, on a fresh non-default stream -> the normalised log.  buffers may name attributes that only exist
    after the step (the side arena)."""
    import torch
    from multilingual_kws_amd.embedding_trainer import _CallTape
    log, lib, stream = [], obj.L, torch.cuda.Stream()
    extra = {}
    obj.L = _CallTape(lib, log)
    try:
        with torch.cuda.stream(stream):
            extra = body() or {}
    finally:
        obj.L = lib
    torch.cuda.synchronize()
    streams = {stream.cuda_stream: "main"}
    if getattr(obj, "_side", None) is not None:
        streams[obj._side.cuda_stream] = "side"
    return _normalise(log, streams, {**buffers, **extra})


def record_all():
    """{case: normalised log} of every case."""
    import torch
    from multilingual_kws_amd import dscnn, weights
    from multilingual_kws_amd.dscnn_trainer import DSCNNTrainer
    from multilingual_kws_amd.embedding_trainer import EmbeddingTrainer, drop_connect_rates
    from multilingual_kws_amd.train_multilingual_embedding import LogitsLayer
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(7)
    spec = torch.from_numpy(rng.integers(0, 670, size=(B, 49, 40)).astype(np.float32) * np.float32(10 / 256)).to(dev)
    d_emb = torch.from_numpy(rng.standard_normal((B, 1024)).astype(np.float32)).to(dev)
    labels = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    rates = drop_connect_rates()
    masks = {name: np.array([i % 2 == 0, True]) for i, name in enumerate(rates)}             # every residual block has one
    scales = {name: torch.tensor([1.0 / (1.0 - rate), 0.0], dtype=torch.float32, device=dev) for name, rate in rates.items()}
    blob = weights.synthetic_blob()
    main, side = (torch.empty(16 << 20, dtype=torch.float32, device=dev) for _ in range(2))   # the default sizes
    small = torch.empty(4 << 20, dtype=torch.float32, device=dev)
    out = {}

    def embedding(case, switches=None, keep_scales=False):
        tr = EmbeddingTrainer(blob, scratch=main, scratch_side=side)
        for k, v in (switches or {}).items():
            assert hasattr(tr, k)
            setattr(tr, k, v)

        def body():
            if keep_scales:
                tr.forward_train(spec, keep_scales=scales)
            else:
                tr.forward_train(spec, masks)
            tr.backward(d_emb)
            tr.adam_step(LR)
            tr.adam_step_dev(LR)
        out[case] = _record(tr, body, dict(params=tr.params, grads=tr.grads, m=tr.m, v=tr.v, d_step=tr.d_step, arena=main, side_arena=side))

    embedding("embedding")
    embedding("embedding/no_wgrad_stream", {"overlap_wgrad": False})
    embedding("embedding/fuse_bn_stats_0", {"fuse_bn_stats": 0})
    embedding("embedding/fuse_bn_stats_7", {"fuse_bn_stats": 7})
    embedding("embedding/wgrad_fork_every_2", {"wgrad_fork_every": 2})
    embedding("embedding/keep_scales", keep_scales=True)

    for case, wd in (("dscnn", 1e-4), ("dscnn/no_weight_decay", 0.0)):
        tr = DSCNNTrainer(dscnn.glorot_params(LABELS, seed=3), max_batch=B, seed=5, weight_decay=wd, scratch=small)

        def body(tr=tr):
            tr.forward_backward(spec, labels)
            tr.adam_step(LR)
        out[case] = _record(tr, body, dict(params=tr.params_dev, grads=tr.grads, m=tr.m, v=tr.v, d_step=tr.d_step, stats=tr.stats, arena=small))

    lay = LogitsLayer(LABELS, seed=1)

    def body():
        stats, _ = lay.loss_grad(d_emb, labels)
        lay.adam_step(LR, 1)
        return {"stats": stats}
    out["logits"] = _record(lay, body, dict(params=lay.params, grads=lay.grads, m=lay.m, v=lay.v))
    return out


def digest(log):
    return hashlib.sha256(json.dumps(log, separators=(",", ":")).encode()).hexdigest()


def golden(logs):
    """What the file stores of record_all()'s result."""
    return {"calls": {c: logs[c] for c in FULL}, "sha256": {c: digest(log) for c, log in logs.items() if c not in FULL}}


def main(out=OUT):
    g = golden(record_all())
    with open(out, "w") as f:
        f.write('{"calls": {\n')
        f.write(",\n".join(f'{json.dumps(c)}: [\n' + ",\n".join(json.dumps(call, separators=(",", ":")) for call in log) + "\n]"
                           for c, log in g["calls"].items()))
        f.write('\n},\n"sha256": ' + json.dumps(g["sha256"], indent=1) + "}\n")
    print(out, {c: len(log) for c, log in g["calls"].items()}, g["sha256"])


if __name__ == "__main__":
    main(*sys.argv[1:2])
